// LoRA adapters on the routed experts of a mixture-of-experts block at prefill (aqlm_hip_lora_sgmv_routed), gfx950, wave64: the
// segmented adapter GEMM of lora_sgmv.hip on row tiles gathered through the expert bucket of the grouped launches (moe_bucket.h).
//
// For every pair p of a tile of the bucket, with adapter a = adapter_ids[p / top_k] and e the tile's expert, and every projection
// s < S of the launch (include/aqlm_hip.h states the definition), with the entry [(a * E + e) * S + s] of the table:
//     t[r]    = sum_k A[r, k] * x_row(p)[k]                                  r < rank, fp32
//     hi = round_T(t), lo = round_T(t - float(hi))                           T = the storage type
//     yrow[i] = round_T(float(yrow[i]) + scaling * sum_r B[i, r] * (hi[r] + lo[r]))     yrow = y + (p * S + s) * out_features
// One workgroup row tile is one bucket slot: up to 16 pairs, all of one expert, read through the pair list.  The passes are
// lora_sgmv.hip's: one per distinct valid adapter among the tile's pairs, every row written exactly once.  Pairs stay in
// ascending order inside an expert, so per-sequence adapter ids cost one pass per tile and two at a seam.  Both grids have
// bucket_max_tiles(num_pairs, num_experts, 16) row tiles x S: the sizes only, never the routing; a slot at or past the bucket's
// tile count exits after that one word.  Both ids stay on the device, nothing is synchronised or allocated, and a captured launch
// stays valid when either id tensor is rewritten (the bucket launch is part of the captured step).
//
// What is checked before an address is formed: the tile record (the chain moe_grouped.hip keeps: expert in [0, E), count in
// [1, 16], first in [0, P - count]), every list entry of the tile (in [0, P), else the tile is dropped), each pair's expert id
// (the tile's expert, else the pair has no adapter: a bucket of other ids) and each pair's adapter id.  A pair with an adapter or
// expert id out of range -- such pairs sit in the bucket's tail and belong to no tile -- or with an entry of rank 0 or of a rank
// that is no multiple of 8 in 8..max_rank keeps its y rows, and nothing is loaded through its table slot.
// The arithmetic is lora_sgmv_body.h's, which lora_sgmv.hip runs too, and the K cut is sgmv_splits(in_features): a pair's y row
// has the bits aqlm_hip_lora_sgmv gives for that one row with that entry as a one-slot table -- whatever the other pairs are,
// their number or their order.  No atomics, no inter-workgroup communication.
#include "lora_sgmv_body.h"
#include "lora_routed_tile.h"

namespace aqlm {

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_routed_shrink_kernel(const RoutedSgmvArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.z / a.nseg, s = blockIdx.z % a.nseg;
  if (slot >= a.bucket[0]) return;
  const int4 tile = bucket_tile(a.bucket, slot);
  const int e = tile.x, first = tile.y, count = tile.z;
  if (e < 0 || e >= a.nexp || count < 1 || count > kRoutedSgmvTile || first < 0 || first > a.npairs - count) return;  // (a foreign bucket)
  const int* pairs = bucket_list(a.bucket, a.max_tiles) + first;
  bool valid;
  const int pr = routed_sgmv_pair(a, pairs, count, valid);
  if (!valid) return;
  const int pw = pairs[std::min((lane >> 4) * 4 + wave, count - 1)];  // the row this thread owns after the LDS sum
  const int myid = routed_sgmv_id(a, pr, e, count);
  const u32x4* xrow = reinterpret_cast<const u32x4*>(a.x + (long)(a.x_per_pair ? pr : pr / a.top_k) * a.xs);
  float* trow = a.t + ((long)pw * a.nseg + s) * a.splits * a.max_rank;
  lora_sgmv_shrink_body<T>(a.table + (long)e * a.nseg + s, (long)a.nexp * a.nseg, myid, xrow, trow, blockIdx.x, blockIdx.y * 16,
                           a.max_rank, a.K8, a.steps_per_wave);
}

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_routed_expand_kernel(const RoutedSgmvArgs a) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.y, s = blockIdx.z;
  if (slot >= a.bucket[0]) return;
  const int4 tile = bucket_tile(a.bucket, slot);
  const int e = tile.x, first = tile.y, count = tile.z;
  if (e < 0 || e >= a.nexp || count < 1 || count > kRoutedSgmvTile || first < 0 || first > a.npairs - count) return;  // (a foreign bucket)
  const int* pairs = bucket_list(a.bucket, a.max_tiles) + first;
  bool valid;
  const int pr = routed_sgmv_pair(a, pairs, count, valid);
  if (!valid) return;
  const int myid = routed_sgmv_id(a, pr, e, count);
  const long row = (long)pr * a.nseg + s;
  lora_sgmv_expand_body<T>(a.table + (long)e * a.nseg + s, (long)a.nexp * a.nseg, myid, a.t + row * a.splits * a.max_rank,
                           a.y + row * a.M, blockIdx.x * kSgmvSpan, a.max_rank, a.M, a.splits);
}

template <class T>
static int launch_sgmv_routed(const RoutedSgmvArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(lora_sgmv_routed_shrink_kernel<T>, dim3(a.splits, (a.max_rank + 15) / 16, a.max_tiles * a.nseg),
                     dim3(kSgmvWaves * 64), 0, stream, a);
  if (int e = check_hip(hipGetLastError(), "lora_sgmv_routed_shrink launch")) return e;
  hipLaunchKernelGGL(lora_sgmv_routed_expand_kernel<T>, dim3((a.M + 16 * kSgmvSpan - 1) / (16 * kSgmvSpan), a.max_tiles, a.nseg),
                     dim3(kSgmvWaves * 64), 0, stream, a);
  return check_hip(hipGetLastError(), "lora_sgmv_routed_expand launch");
}

static bool sgmv_routed_shape_ok(int out_features, int in_features, int max_rank, int num_pairs, int num_experts, int num_segments) {
  return lora_shape_ok(out_features, in_features, max_rank, num_pairs, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS) &&
         out_features % 4 == 0 && num_experts >= 1 && num_experts <= AQLM_HIP_MAX_ROUTED_EXPERTS && num_segments >= 1 &&
         num_segments <= 2;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_sgmv_routed_workspace_bytes(int num_pairs, int num_segments, int max_rank, int in_features) {
  if (!sgmv_routed_shape_ok(4, in_features, max_rank, num_pairs, 1, num_segments)) return 0;
  return (size_t)num_pairs * (size_t)num_segments * (size_t)sgmv_splits(in_features) * (size_t)max_rank * 4;
}

extern "C" int aqlm_hip_lora_sgmv_routed_supported(int out_features, int in_features, int max_rank, int num_pairs, int num_experts,
                                                   int num_segments) {
  return sgmv_routed_shape_ok(out_features, in_features, max_rank, num_pairs, num_experts, num_segments) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_sgmv_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments,
                                         int max_rank, const void* adapter_ids, int adapter_ids_int64, const void* expert_ids,
                                         int expert_ids_int64, const void* bucket, int num_pairs, int top_k, const void* x,
                                         long x_row_stride, int x_per_pair, void* y, int out_features, int in_features, int dtype,
                                         void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_sgmv_routed";
  if (int e = check_not_null(who, table && expert_ids && x && y && workspace)) return e;
  if (int e = check_aligned(who, "expert_ids", ids_aligned(expert_ids, expert_ids_int64))) return e;
  if (num_experts < 1 || num_segments < 1 || top_k < 1 || num_pairs < 1 || num_pairs % top_k != 0) {
    set_last_error("%s: bad sizes (experts=%d segments=%d pairs=%d top_k=%d: all positive, pairs a multiple of top_k)", who,
                   num_experts, num_segments, num_pairs, top_k);
    return AQLM_HIP_E_INVALID;
  }
  // y is contiguous: a row per (pair, segment), row stride out_features; x holds token rows or pair rows.  (Counts past what the
  // launch takes only feed the aliasing check here: the shape checks below refuse the call.)
  const int pairs_c = std::min(num_pairs, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS);
  const int x_rows = x_per_pair ? pairs_c : std::max(1, pairs_c / top_k);
  if (int e = lora_check_args(who, table, num_adapters, max_rank, adapter_ids, adapter_ids_int64, num_pairs, x, x_row_stride, y,
                              out_features, out_features, in_features, dtype, workspace, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS, x_rows,
                              pairs_c * std::min(num_segments, 2)))
    return e;
  if (int e = check_not_null(who, bucket != nullptr)) return e;
  if (int e = check_aligned(who, "bucket", aligned16(bucket))) return e;
  if (num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS || num_segments > 2) {
    set_last_error("%s: shape outside the kernels (%d experts x %d segments; 1..%d x 1..2 supported)", who, num_experts,
                   num_segments, AQLM_HIP_MAX_ROUTED_EXPERTS);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (out_features % 4 != 0 || (reinterpret_cast<uintptr_t>(y) & 7u)) {
    set_last_error("%s: y rows not 8-byte aligned (y %p, out_features %d): the expand writes groups of 4 outputs at a row stride "
                   "of out_features", who, y, out_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = lora_check_workspace(who, workspace_bytes,
                                   aqlm_hip_lora_sgmv_routed_workspace_bytes(num_pairs, num_segments, max_rank, in_features)))
    return e;

  RoutedSgmvArgs a{};
  a.table = table;
  a.adapter_ids = adapter_ids;
  a.expert_ids = expert_ids;
  a.bucket = (const int*)bucket;
  a.x = (const uint16_t*)x;
  a.t = (float*)workspace;
  a.y = (uint16_t*)y;
  a.xs = x_row_stride;
  a.adapter_ids_int64 = adapter_ids_int64 ? 1 : 0;
  a.expert_ids_int64 = expert_ids_int64 ? 1 : 0;
  a.nadapters = num_adapters;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.npairs = num_pairs;
  a.top_k = top_k;
  a.x_per_pair = x_per_pair ? 1 : 0;
  a.max_tiles = bucket_max_tiles(num_pairs, num_experts, kRoutedSgmvTile);
  a.max_rank = max_rank;
  a.K8 = in_features / 8;
  a.splits = sgmv_splits(in_features);
  a.steps_per_wave = sgmv_steps_per_wave(in_features);
  a.M = out_features;
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == AQLM_HIP_F16 ? launch_sgmv_routed<F16>(a, stream) : launch_sgmv_routed<BF16>(a, stream);
}

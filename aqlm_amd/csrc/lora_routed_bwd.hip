// The backward of the LoRA adapters on the routed experts of a mixture-of-experts block, gfx950, wave64: what
// aqlm_hip_lora_sgmv_routed (lora_sgmv_routed.hip) cannot do by being called on other operands.
//
// grad_x needs no kernel of its own: it is aqlm_hip_lora_sgmv_routed on a TRANSPOSED table -- per entry {a: B^T [r, M],
// b: A^T [K, r]}, laid out [s][a][e] so that a segment is a one-segment table -- with x := grad_y[:, s, :].
// aqlm_hip_lora_transpose_routed (lora_routed_transpose_kernel) fills the buffer those entries point into from the weights as they
// are now: one launch over all entries of the forward table, 16-byte loads and 2-byte stores, the rank of an entry and the place
// of its copies inside the buffer checked before an address is formed.
//
// grad_A and grad_B are one reduction over pairs (aqlm_hip_lora_grad_routed, lora_routed_grad_kernel): for ONE adapter index and
// every (expert e, segment s) of the call
//     G[e][s][r][i] = scaling * sum over the pairs p of expert e with that adapter, ascending, of  w[p, s][r] * V[p, s][i]     (fp32)
// with V storage-type rows (x for grad_A, grad_y for grad_B^T) and w fp32 rank-sized rows (u = B^T grad_y for grad_A, the
// forward's t = A x for grad_B^T), given as `splits` slices that are added in slice order, as lora_sgmv_expand_body adds them.
// Both operands are laid out along the OUTPUT index i, so the kernel runs on the VALU: a lane owns 8 contiguous i (one 16-byte
// load of a V row per pair), a workgroup (one wave) 512 of them and 8 ranks, the 64 accumulators stay in VGPRs, and the w values
// are uniform over the wave (lane j fetches those of the tile's pair j, the multiply reads them lane by lane).  At rank 16 that is 16 FMA per 2 bytes loaded, about the machine's fp32-to-HBM balance; the matrix
// unit would need a transposed read of V.  A workgroup walks the tile records of the bucket, takes the tiles of its expert --
// each record and each list entry checked as lora_sgmv_routed_shrink_kernel checks them (lora_routed_tile.h) --, skips a tile none
// of whose pairs carries the adapter, issues the tile's V loads together and then multiplies.  The order of the sum is the
// bucket's, ascending pair order inside an expert: no atomics, no inter-workgroup communication, the result a function of the
// inputs alone.  Every element of a live entry is written (zeros when it has no pairs, and for r in rank .. max_rank); an entry
// that is not live (rank 0, or no multiple of 8 in 8..max_rank) is not touched.
#include "lora_routed_tile.h"
#include "lora_sgmv_body.h"

namespace aqlm {

// ---------------------------------------------------------------------------------------------------------------------------
// transpose
// ---------------------------------------------------------------------------------------------------------------------------
struct RoutedTransposeArgs {
  const aqlm_hip_lora_entry* table;       // [nadapters][nexp][nseg]: {A [r, K], B [M, r]}
  const aqlm_hip_lora_entry* transposed;  // [nseg][nadapters][nexp]: {B^T [r, M], A^T [K, r]}
  uintptr_t buf0, buf1;                   // the buffer the transposed entries point into
  int nadapters, nexp, nseg, max_rank, K, M;
};

constexpr int kTransposeThreads = 256;
constexpr int kTransposeBlocks = 64;  // per entry; each strides over the entry's 16-byte pieces

__device__ __forceinline__ uint16_t half_of(const u32x4& v, int j) {
  const uint32_t w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
  return (uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu));
}

__global__ __launch_bounds__(kTransposeThreads) void lora_routed_transpose_kernel(const RoutedTransposeArgs a) {
  const int idx = blockIdx.y;  // (ad * nexp + e) * nseg + s
  const int s = idx % a.nseg, e = (idx / a.nseg) % a.nexp, ad = idx / (a.nseg * a.nexp);
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(a.table + idx);
  const lora_entry_ptr tr = (lora_entry_ptr)(uintptr_t)(a.transposed + ((long)s * a.nadapters + ad) * a.nexp + e);
  const int rank = lora_rank(ent->rank, a.max_rank);
  if (rank == 0 || tr->rank != rank) return;  // not live, or a transposed table of other weights
  const uintptr_t bt = (uintptr_t)tr->a, at = (uintptr_t)tr->b;
  const uintptr_t bytes_a = (uintptr_t)rank * a.K * 2, bytes_b = (uintptr_t)rank * a.M * 2;
  if ((at & 1u) || at < a.buf0 || at > a.buf1 || a.buf1 - at < bytes_a) return;  // the copies lie inside the buffer
  if ((bt & 1u) || bt < a.buf0 || bt > a.buf1 || a.buf1 - bt < bytes_b) return;
  const lora_gbl_u32x4_ptr A = (lora_gbl_u32x4_ptr)(uintptr_t)ent->a;
  const lora_gbl_u32x4_ptr B = (lora_gbl_u32x4_ptr)(uintptr_t)ent->b;
  uint16_t* At = reinterpret_cast<uint16_t*>(at);
  uint16_t* Bt = reinterpret_cast<uint16_t*>(bt);
  const int K8 = a.K >> 3, r8 = rank >> 3;
  const int stride = gridDim.x * kTransposeThreads;
  // A [rank][K] -> A^T [K][rank]: neighbouring threads take neighbouring ranks, so each of the 8 stores of a wave is contiguous
  for (int it = blockIdx.x * kTransposeThreads + threadIdx.x; it < rank * K8; it += stride) {
    const int rr = it % rank, k8 = it / rank;
    const u32x4 v = A[(long)rr * K8 + k8];
#pragma unroll
    for (int j = 0; j < 8; ++j) At[(long)(k8 * 8 + j) * rank + rr] = half_of(v, j);
  }
  // B [M][rank] -> B^T [rank][M]: neighbouring threads take neighbouring outputs
  for (int it = blockIdx.x * kTransposeThreads + threadIdx.x; it < a.M * r8; it += stride) {
    const int m = it % a.M, q = it / a.M;
    const u32x4 v = B[(long)m * r8 + q];
#pragma unroll
    for (int j = 0; j < 8; ++j) Bt[(long)(q * 8 + j) * a.M + m] = half_of(v, j);
  }
}

static bool transpose_shape_ok(int out_features, int in_features, int max_rank, int num_experts, int num_segments) {
  return out_features >= 8 && out_features % 8 == 0 && in_features >= 8 && in_features % 8 == 0 && max_rank >= 8 &&
         max_rank <= kLoraMaxRank && max_rank % 8 == 0 && num_experts >= 1 && num_experts <= AQLM_HIP_MAX_ROUTED_EXPERTS &&
         num_segments >= 1 && num_segments <= 2;
}

// ---------------------------------------------------------------------------------------------------------------------------
// grad_A / grad_B
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kGradRanks = 8;   // ranks per workgroup: 8 x 8 accumulators per lane, so that rank 128 is 16 workgroups and no spill
constexpr int kGradSpan = 64 * 8;  // outputs per workgroup: 8 per lane
constexpr int kGradMaxSplits = kSgmvMaxSplits;  // w comes from a shrink launch

struct RoutedGradArgs {
  RoutedSgmvArgs r;  // table, ids, bucket and sizes as the forward's; x / xs / x_per_pair: the V rows; t / splits: w and its slices
  long v_seg_stride, w_pair_stride, w_seg_stride, w_split_stride;
  float* g;  // [nexp][nseg][max_rank][dim]
  int adapter, dim;
};

template <class T>
__global__ __launch_bounds__(64) void lora_routed_grad_kernel(const RoutedGradArgs g) {
  const RoutedSgmvArgs& a = g.r;
  const int lane = threadIdx.x;
  const int e = blockIdx.z / a.nseg, s = blockIdx.z % a.nseg;
  const int r0 = blockIdx.y * kGradRanks;
  const int i0 = (blockIdx.x * 64 + lane) * 8;
  const bool mine = i0 < g.dim;  // dim % 8 == 0: a lane's 8 outputs exist together
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(a.table + ((long)g.adapter * a.nexp + e) * a.nseg + s);
  const int rank = lora_rank(ent->rank, a.max_rank);
  if (rank == 0) return;  // not live: its region stays as it is
  const float scaling = ent->scaling;

  float acc[kGradRanks][8];
#pragma unroll
  for (int rr = 0; rr < kGradRanks; ++rr)
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) acc[rr][ii] = 0.f;

  if (r0 < rank) {  // rank % 8 == 0: the 8 ranks exist together
    const int ntiles = std::min(a.bucket[0], a.max_tiles);
    const int* list = bucket_list(a.bucket, a.max_tiles);
    const uint16_t* vbase = a.x + (long)s * g.v_seg_stride + (mine ? i0 : 0);
    const float* wbase = a.t + (long)s * g.w_seg_stride + r0;
    for (int slot = 0; slot < ntiles; ++slot) {
      const int4 tile = bucket_tile(a.bucket, slot);
      const int first = tile.y, count = tile.z;
      if (tile.x != e) continue;  // (e lies in [0, nexp): the grid)
      if (count < 1 || count > kRoutedSgmvTile || first < 0 || first > a.npairs - count) continue;  // (a foreign bucket)
      bool valid;
      const int pr = routed_sgmv_pair(a, list + first, count, valid);
      if (!valid) continue;
      const int myid = routed_sgmv_id(a, pr, e, count);
      const uint32_t match = (uint32_t)__builtin_amdgcn_ballot_w64(myid == g.adapter);  // lanes 0..15 only
      if (!match) continue;
      // lane j < 16 fetches the 8 w values of the tile's pair j (slices in slice order); the multiply reads them lane by lane.
      // All loads of a tile -- these and the V rows -- are in flight before the first product.
      float wl[kGradRanks];
#pragma unroll
      for (int rr = 0; rr < kGradRanks; ++rr) wl[rr] = 0.f;
      if (lane < kRoutedSgmvTile && ((match >> lane) & 1)) {  // (the lane's own pair: a matching lane lies below count)
        const float* wrow = wbase + (long)pr * g.w_pair_stride;
#pragma unroll
        for (int rr = 0; rr < kGradRanks; ++rr) wl[rr] = wrow[rr];
        for (int sp = 1; sp < a.splits; ++sp)
#pragma unroll
          for (int rr = 0; rr < kGradRanks; ++rr) wl[rr] += wrow[(long)sp * g.w_split_stride + rr];
      }
      u32x4 v[kRoutedSgmvTile];
#pragma unroll
      for (int j = 0; j < kRoutedSgmvTile; ++j) {  // the tile's V loads, together
        if ((match >> j) & 1) {
          const int pj = __builtin_amdgcn_readlane(pr, j);
          v[j] = *reinterpret_cast<const u32x4*>(vbase + (long)(a.x_per_pair ? pj : pj / a.top_k) * a.xs);
        }
      }
#pragma unroll
      for (int j = 0; j < kRoutedSgmvTile; ++j) {
        if ((match >> j) & 1) {
          float w[kGradRanks];
#pragma unroll
          for (int rr = 0; rr < kGradRanks; ++rr)
            w[rr] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl[rr]), j));
          const float f[8] = {T::lo(v[j].x), T::hi(v[j].x), T::lo(v[j].y), T::hi(v[j].y),
                              T::lo(v[j].z), T::hi(v[j].z), T::lo(v[j].w), T::hi(v[j].w)};
#pragma unroll
          for (int rr = 0; rr < kGradRanks; ++rr)
#pragma unroll
            for (int ii = 0; ii < 8; ++ii) acc[rr][ii] = fmaf(w[rr], f[ii], acc[rr][ii]);
        }
      }
    }
  }

  if (!mine) return;
  float* out = g.g + (((long)e * a.nseg + s) * a.max_rank + r0) * g.dim + i0;
#pragma unroll
  for (int rr = 0; rr < kGradRanks; ++rr) {
    float4* o = reinterpret_cast<float4*>(out + (long)rr * g.dim);
    o[0] = make_float4(scaling * acc[rr][0], scaling * acc[rr][1], scaling * acc[rr][2], scaling * acc[rr][3]);
    o[1] = make_float4(scaling * acc[rr][4], scaling * acc[rr][5], scaling * acc[rr][6], scaling * acc[rr][7]);
  }
}

static bool grad_shape_ok(int dim, int max_rank, int num_pairs, int num_experts, int num_segments) {
  return dim >= 8 && dim % 8 == 0 && max_rank >= 8 && max_rank <= kLoraMaxRank && max_rank % 8 == 0 && num_pairs >= 1 &&
         num_pairs <= AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS && num_experts >= 1 && num_experts <= AQLM_HIP_MAX_ROUTED_EXPERTS &&
         num_segments >= 1 && num_segments <= 2;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_transpose_routed_bytes(int num_adapters, int num_experts, int num_segments, int max_rank,
                                                       int out_features, int in_features) {
  if (num_adapters < 1 || !transpose_shape_ok(out_features, in_features, max_rank, num_experts, num_segments)) return 0;
  return (size_t)num_adapters * (size_t)num_experts * (size_t)num_segments * (size_t)max_rank *
         ((size_t)out_features + (size_t)in_features) * 2;
}

extern "C" int aqlm_hip_lora_transpose_routed_supported(int out_features, int in_features, int max_rank, int num_experts,
                                                        int num_segments) {
  return transpose_shape_ok(out_features, in_features, max_rank, num_experts, num_segments) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_transpose_routed(const aqlm_hip_lora_entry* table, const aqlm_hip_lora_entry* transposed,
                                              int num_adapters, int num_experts, int num_segments, int max_rank, int out_features,
                                              int in_features, void* buffer, size_t buffer_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_transpose_routed";
  if (int e = check_not_null(who, table && transposed && buffer)) return e;
  if (int e = check_aligned(who, "table / transposed / buffer", aligned8(table) && aligned8(transposed) && aligned16(buffer))) return e;
  if (num_adapters < 1 || num_experts < 1 || num_segments < 1 || max_rank < 1 || out_features < 1 || in_features < 1 ||
      buffer_bytes < 1) {
    set_last_error("%s: bad sizes (adapters=%d experts=%d segments=%d max_rank=%d out=%d in=%d buffer=%zu bytes: all positive)", who,
                   num_adapters, num_experts, num_segments, max_rank, out_features, in_features, buffer_bytes);
    return AQLM_HIP_E_INVALID;
  }
  if (!transpose_shape_ok(out_features, in_features, max_rank, num_experts, num_segments)) {
    set_last_error("%s: shape outside the kernel (rank a multiple of 8 in 8..%d, in_features %% 8 == 0, out_features %% 8 == 0, "
                   "1..%d experts x 1..2 segments; got max_rank=%d in=%d out=%d, %d x %d)", who, kLoraMaxRank,
                   AQLM_HIP_MAX_ROUTED_EXPERTS, max_rank, in_features, out_features, num_experts, num_segments);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const long entries = (long)num_adapters * num_experts * num_segments;
  if (entries > 65535) {
    set_last_error("%s: %ld table entries (at most 65535 per call)", who, entries);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  RoutedTransposeArgs a{};
  a.table = table;
  a.transposed = transposed;
  a.buf0 = reinterpret_cast<uintptr_t>(buffer);
  a.buf1 = a.buf0 + buffer_bytes;
  a.nadapters = num_adapters;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.max_rank = max_rank;
  a.K = in_features;
  a.M = out_features;
  const long pieces = (long)max_rank * std::max(in_features, out_features) / 8;
  const int blocks = (int)std::min<long>((pieces + kTransposeThreads - 1) / kTransposeThreads, kTransposeBlocks);
  hipLaunchKernelGGL(lora_routed_transpose_kernel, dim3(blocks, (unsigned)entries), dim3(kTransposeThreads), 0, (hipStream_t)stream_, a);
  return check_hip(hipGetLastError(), "lora_routed_transpose launch");
}

extern "C" int aqlm_hip_lora_grad_routed_supported(int dim, int max_rank, int num_pairs, int num_experts, int num_segments) {
  return grad_shape_ok(dim, max_rank, num_pairs, num_experts, num_segments) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_grad_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments,
                                         int max_rank, int adapter, const void* adapter_ids, int adapter_ids_int64,
                                         const void* expert_ids, int expert_ids_int64, const void* bucket, int num_pairs, int top_k,
                                         const void* v, long v_row_stride, long v_seg_stride, int v_per_pair, int dim, const float* w,
                                         long w_pair_stride, long w_seg_stride, int w_splits, long w_split_stride, float* g,
                                         size_t g_bytes, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_lora_grad_routed";
  if (int e = check_not_null(who, table && expert_ids && bucket && v && w && g)) return e;
  if (int e = check_aligned(who, "table / ids / bucket / w / g",
                            aligned8(table) && (!adapter_ids || ids_aligned(adapter_ids, adapter_ids_int64)) &&
                                ids_aligned(expert_ids, expert_ids_int64) && aligned16(bucket) &&
                                (reinterpret_cast<uintptr_t>(w) & 3u) == 0 && aligned16(g)))
    return e;
  if (num_adapters < 1 || num_experts < 1 || num_segments < 1 || max_rank < 1 || top_k < 1 || num_pairs < 1 ||
      num_pairs % top_k != 0 || dim < 1 || w_splits < 1 || adapter < 0 || adapter >= num_adapters) {
    set_last_error("%s: bad sizes (adapters=%d experts=%d segments=%d max_rank=%d pairs=%d top_k=%d dim=%d splits=%d: all positive, "
                   "pairs a multiple of top_k; adapter=%d in [0, adapters))", who, num_adapters, num_experts, num_segments, max_rank,
                   num_pairs, top_k, dim, w_splits, adapter);
    return AQLM_HIP_E_INVALID;
  }
  if (v_row_stride < dim || v_seg_stride < 0 || w_pair_stride < max_rank || w_seg_stride < 0 ||
      (w_splits > 1 && w_split_stride < max_rank)) {
    set_last_error("%s: strides (V row %ld, V segment %ld, w pair %ld, w segment %ld, w split %ld) shorter than the rows (dim=%d, "
                   "max_rank=%d) or negative", who, v_row_stride, v_seg_stride, w_pair_stride, w_seg_stride, w_split_stride, dim,
                   max_rank);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!grad_shape_ok(dim, max_rank, num_pairs, num_experts, num_segments) || w_splits > kGradMaxSplits || !aligned16(v) ||
      v_row_stride % 8 != 0 || v_seg_stride % 8 != 0) {
    set_last_error("%s: shape outside the kernel (rank a multiple of 8 in 8..%d, dim %% 8 == 0, 1..%d pairs, 1..%d experts x 1..2 "
                   "segments, at most %d slices of w, V rows 16-byte aligned; got max_rank=%d dim=%d pairs=%d %d x %d splits=%d V "
                   "strides %ld / %ld)", who, kLoraMaxRank, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS, AQLM_HIP_MAX_ROUTED_EXPERTS,
                   kGradMaxSplits, max_rank, dim, num_pairs, num_experts, num_segments, w_splits, v_row_stride, v_seg_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t need = (size_t)num_experts * (size_t)num_segments * (size_t)max_rank * (size_t)dim * 4;
  if (g_bytes < need) {
    set_last_error("%s: output of %zu bytes, %zu bytes needed", who, g_bytes, need);
    return AQLM_HIP_E_INVALID;
  }

  RoutedGradArgs ga{};
  RoutedSgmvArgs& a = ga.r;
  a.table = table;
  a.adapter_ids = adapter_ids;
  a.expert_ids = expert_ids;
  a.bucket = (const int*)bucket;
  a.x = (const uint16_t*)v;
  a.t = const_cast<float*>(w);  // read only here
  a.xs = v_row_stride;
  a.adapter_ids_int64 = adapter_ids_int64 ? 1 : 0;
  a.expert_ids_int64 = expert_ids_int64 ? 1 : 0;
  a.nadapters = num_adapters;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.npairs = num_pairs;
  a.top_k = top_k;
  a.x_per_pair = v_per_pair ? 1 : 0;
  a.max_tiles = bucket_max_tiles(num_pairs, num_experts, kRoutedSgmvTile);
  a.max_rank = max_rank;
  a.splits = w_splits;
  ga.v_seg_stride = v_seg_stride;
  ga.w_pair_stride = w_pair_stride;
  ga.w_seg_stride = w_seg_stride;
  ga.w_split_stride = w_split_stride;
  ga.g = g;
  ga.adapter = adapter;
  ga.dim = dim;
  const dim3 grid((dim + kGradSpan - 1) / kGradSpan, max_rank / kGradRanks, num_experts * num_segments);
  hipStream_t stream = (hipStream_t)stream_;
  if (dtype == AQLM_HIP_F16)
    hipLaunchKernelGGL(lora_routed_grad_kernel<F16>, grid, dim3(64), 0, stream, ga);
  else
    hipLaunchKernelGGL(lora_routed_grad_kernel<BF16>, grid, dim3(64), 0, stream, ga);
  return check_hip(hipGetLastError(), "lora_routed_grad launch");
}

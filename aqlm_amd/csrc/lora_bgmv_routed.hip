// LoRA adapters on the routed experts of a mixture-of-experts block (aqlm_hip_lora_bgmv_routed), gfx950, wave64: the batched
// adapter matvec of lora_bgmv.hip with a row per (token, expert) pair and projection.
//
// For every pair p < num_pairs with adapter a = adapter_ids[p / top_k] and expert e = expert_ids[p], and every projection
// s < S of the launch (include/aqlm_hip.h states the definition), with the entry [(a * E + e) * S + s] of the table:
//     t[r]    = sum_k A[r, k] * x_row(p)[k]                                  r < rank, fp32, never rounded
//     yrow[i] = round(float(yrow[i]) + scaling * sum_r B[i, r] * t[r])       yrow = y + (p * S + s) * out_features
// Two launches whose grids depend on the shapes only (shrink: rank groups x pairs x S, expand + add: output blocks x pairs x S);
// both ids stay on the device, nothing is synchronised, a captured launch stays valid when either id tensor is rewritten.  BOTH
// ids are range-checked before either forms an address (lora_common.h holds the rule): a pair whose adapter or expert id lies
// outside its range touches no table slot and its y rows are never written; an entry of rank 0 (a combination the adapter does
// not cover) or of any rank that is no multiple of 8 in 8..max_rank counts as "no adapter" the same way.
// The arithmetic is lora_bgmv_body.h's, which lora_bgmv.hip runs too: a pair's y row has the bits aqlm_hip_lora_bgmv gives for
// that one row with that entry as a one-slot table -- whatever the other pairs are, their number or their order.  No atomics, no
// inter-workgroup communication.
#include <algorithm>

#include "lora_bgmv_body.h"

namespace aqlm {

struct RoutedLoraArgs {
  const aqlm_hip_lora_entry* table;  // [nadapters][nexp][nseg]
  const void* adapter_ids;           // one per TOKEN, or NULL: adapter 0
  const void* expert_ids;            // one per pair
  const uint16_t* x;
  float* t;                          // [npairs][nseg][max_rank]
  uint16_t* y;                       // [npairs][nseg][M]
  long xs;
  int adapter_ids_int64, expert_ids_int64, nadapters, nexp, nseg, top_k, x_per_pair, max_rank, K8, steps_per_wave, M;
};

// the table entry of (pair p, segment s), or a null pointer when the pair names no adapter or no expert
__device__ __forceinline__ lora_entry_ptr routed_lora_entry(const RoutedLoraArgs& a, int p, int s) {
  const long ad = lora_row_id(a.adapter_ids, a.adapter_ids_int64, p / a.top_k, a.nadapters);
  const long ex = lora_row_id(a.expert_ids, a.expert_ids_int64, p, a.nexp);
  if (ad < 0 || ex < 0) return (lora_entry_ptr)0;
  return (lora_entry_ptr)(uintptr_t)(a.table + (ad * a.nexp + ex) * a.nseg + s);
}

template <class T>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_routed_shrink_kernel(const RoutedLoraArgs a) {
  const int p = blockIdx.y, s = blockIdx.z;
  const lora_entry_ptr ent = routed_lora_entry(a, p, s);
  if (!ent) return;  // uniform over the workgroup
  const int xr = a.x_per_pair ? p : p / a.top_k;
  lora_shrink_body<T>(ent, reinterpret_cast<const u32x4*>(a.x + (long)xr * a.xs), a.t + ((long)p * a.nseg + s) * a.max_rank,
                      blockIdx.x * kShrinkRanks, a.max_rank, a.K8, a.steps_per_wave);
}

template <class T>
__global__ __launch_bounds__(kExpandThreads) void lora_routed_expand_kernel(const RoutedLoraArgs a) {
  const int p = blockIdx.y, s = blockIdx.z;
  const lora_entry_ptr ent = routed_lora_entry(a, p, s);
  if (!ent) return;
  const long row = (long)p * a.nseg + s;
  lora_expand_body<T>(ent, a.t + row * a.max_rank, a.y + row * a.M, blockIdx.x * kExpandThreads, a.max_rank, a.M);
}

template <class T>
static int launch_lora_routed(const RoutedLoraArgs& a, int num_pairs, hipStream_t stream) {
  hipLaunchKernelGGL(lora_routed_shrink_kernel<T>, dim3(a.max_rank / kShrinkRanks, num_pairs, a.nseg), dim3(kShrinkWaves * 64), 0,
                     stream, a);
  if (int e = check_hip(hipGetLastError(), "lora_routed_shrink launch")) return e;
  hipLaunchKernelGGL(lora_routed_expand_kernel<T>, dim3((a.M + kExpandThreads - 1) / kExpandThreads, num_pairs, a.nseg),
                     dim3(kExpandThreads), 0, stream, a);
  return check_hip(hipGetLastError(), "lora_routed_expand launch");
}

static bool lora_routed_shape_ok(int out_features, int in_features, int max_rank, int num_pairs, int num_experts, int num_segments) {
  return lora_shape_ok(out_features, in_features, max_rank, num_pairs, AQLM_HIP_MAX_LORA_ROWS) && num_experts >= 1 &&
         num_experts <= AQLM_HIP_MAX_ROUTED_EXPERTS && num_segments >= 1 && num_segments <= 2;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_bgmv_routed_workspace_bytes(int num_pairs, int num_segments, int max_rank) {
  if (!lora_routed_shape_ok(1, 8, max_rank, num_pairs, 1, num_segments)) return 0;
  return (size_t)num_pairs * (size_t)num_segments * (size_t)max_rank * 4;
}

extern "C" int aqlm_hip_lora_bgmv_routed_supported(int out_features, int in_features, int max_rank, int num_pairs, int num_experts,
                                                   int num_segments) {
  return lora_routed_shape_ok(out_features, in_features, max_rank, num_pairs, num_experts, num_segments) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_bgmv_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments,
                                         int max_rank, const void* adapter_ids, int adapter_ids_int64, const void* expert_ids,
                                         int expert_ids_int64, int num_pairs, int top_k, const void* x, long x_row_stride,
                                         int x_per_pair, void* y, int out_features, int in_features, int dtype, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_bgmv_routed";
  if (int e = check_not_null(who, table && expert_ids && x && y && workspace)) return e;
  if (int e = check_aligned(who, "expert_ids", ids_aligned(expert_ids, expert_ids_int64))) return e;
  if (num_experts < 1 || num_segments < 1 || top_k < 1 || num_pairs < 1 || num_pairs % top_k != 0) {
    set_last_error("%s: bad sizes (experts=%d segments=%d pairs=%d top_k=%d: all positive, pairs a multiple of top_k)", who,
                   num_experts, num_segments, num_pairs, top_k);
    return AQLM_HIP_E_INVALID;
  }
  // y is contiguous: a row per (pair, segment), row stride out_features; x holds token rows or pair rows.  (Counts past what the
  // launch takes only feed the aliasing check here: the shape checks below refuse the call.)
  const int pairs_c = std::min(num_pairs, AQLM_HIP_MAX_LORA_ROWS);
  const int x_rows = x_per_pair ? pairs_c : std::max(1, pairs_c / top_k);
  if (int e = lora_check_args(who, table, num_adapters, max_rank, adapter_ids, adapter_ids_int64, num_pairs, x, x_row_stride, y,
                              out_features, out_features, in_features, dtype, workspace, AQLM_HIP_MAX_LORA_ROWS, x_rows,
                              pairs_c * std::min(num_segments, 2)))
    return e;
  if (num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS || num_segments > 2) {
    set_last_error("%s: shape outside the kernels (%d experts x %d segments; 1..%d x 1..2 supported)", who, num_experts,
                   num_segments, AQLM_HIP_MAX_ROUTED_EXPERTS);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = lora_check_workspace(who, workspace_bytes, aqlm_hip_lora_bgmv_routed_workspace_bytes(num_pairs, num_segments, max_rank)))
    return e;

  RoutedLoraArgs a{};
  a.table = table;
  a.adapter_ids = adapter_ids;
  a.expert_ids = expert_ids;
  a.x = (const uint16_t*)x;
  a.t = (float*)workspace;
  a.y = (uint16_t*)y;
  a.xs = x_row_stride;
  a.adapter_ids_int64 = adapter_ids_int64 ? 1 : 0;
  a.expert_ids_int64 = expert_ids_int64 ? 1 : 0;
  a.nadapters = num_adapters;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.top_k = top_k;
  a.x_per_pair = x_per_pair ? 1 : 0;
  a.max_rank = max_rank;
  a.K8 = in_features / 8;
  a.steps_per_wave = lora_shrink_steps_per_wave(in_features);
  a.M = out_features;
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == AQLM_HIP_F16 ? launch_lora_routed<F16>(a, num_pairs, stream) : launch_lora_routed<BF16>(a, num_pairs, stream);
}

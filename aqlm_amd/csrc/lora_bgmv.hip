// Per-row batched LoRA adapter matvec on top of a quantized layer's output (aqlm_hip_lora_bgmv), gfx950, wave64.
//
// For every row b < rows with adapter a = ids[b] (include/aqlm_hip.h states the definition):
//     t[b, r] = sum_k A_a[r, k] * x[b, k]                                    r < rank_a, fp32, never rounded
//     y[b, i] = round(float(y[b, i]) + scaling_a * sum_r B_a[i, r] * t[b, r])
// in two launches whose grids depend on the shapes only, in the style of the routed launches (gemv_routed.hip): the ids stay on
// the device, nothing is synchronised, a captured launch stays valid when the ids change.  Unlike there an id selects a table
// entry: lora_common.h states the rules (range check before the address, ranks that count as "no adapter") and holds them for
// this file and lora_sgmv.hip; a row without an adapter exits both kernels before its table slot is touched, and its y row is
// never written.
// The arithmetic of both kernels lives in lora_bgmv_body.h (shrink: one workgroup per (row, kShrinkRanks ranks); expand + add: a
// thread owns output i of row b), shared with the routed launch of lora_bgmv_routed.hip: here a workgroup finds its entry by
// ids[b], and its x, t and y rows by b.
// No atomics, no inter-workgroup communication; every sum has a fixed order that depends on the shapes only, so a row's bits
// depend on its own x row, its own y row and its adapter -- not on the other rows, their number or their order.
#include <algorithm>

#include "lora_bgmv_body.h"

namespace aqlm {

template <class T>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_shrink_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                        const uint16_t* x, float* t, long xs, int ids_int64,
                                                                        int nadapters, int max_rank, int K8, int steps_per_wave) {
  const int b = blockIdx.y;
  const long id = lora_row_id(ids, ids_int64, b, nadapters);
  if (id < 0) return;  // uniform over the workgroup
  lora_shrink_body<T>((lora_entry_ptr)(uintptr_t)(table + id), reinterpret_cast<const u32x4*>(x + (long)b * xs),
                      t + (long)b * max_rank, blockIdx.x * kShrinkRanks, max_rank, K8, steps_per_wave);
}

template <class T>
__global__ __launch_bounds__(kExpandThreads) void lora_expand_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                     const float* t, uint16_t* y, long ys, int ids_int64,
                                                                     int nadapters, int max_rank, int M) {
  const int b = blockIdx.y;
  const long id = lora_row_id(ids, ids_int64, b, nadapters);
  if (id < 0) return;
  lora_expand_body<T>((lora_entry_ptr)(uintptr_t)(table + id), t + (long)b * max_rank, y + (long)b * ys,
                      blockIdx.x * kExpandThreads, max_rank, M);
}

template <class T>
static int launch_lora(const aqlm_hip_lora_entry* table, int nadapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const uint16_t* x, long xs, uint16_t* y, long ys, int M, int K, float* t, hipStream_t stream) {
  const int K8 = K / 8;
  const int steps_per_wave = lora_shrink_steps_per_wave(K);
  hipLaunchKernelGGL(lora_shrink_kernel<T>, dim3(max_rank / kShrinkRanks, rows), dim3(kShrinkWaves * 64), 0, stream, table, ids, x,
                     t, xs, ids_int64, nadapters, max_rank, K8, steps_per_wave);
  if (int e = check_hip(hipGetLastError(), "lora_shrink launch")) return e;
  hipLaunchKernelGGL(lora_expand_kernel<T>, dim3((M + kExpandThreads - 1) / kExpandThreads, rows), dim3(kExpandThreads), 0, stream,
                     table, ids, (const float*)t, y, ys, ids_int64, nadapters, max_rank, M);
  return check_hip(hipGetLastError(), "lora_expand launch");
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_workspace_bytes(int rows, int max_rank) {
  if (!lora_shape_ok(1, 8, max_rank, rows, AQLM_HIP_MAX_LORA_ROWS)) return 0;
  return (size_t)rows * (size_t)max_rank * 4;
}

extern "C" int aqlm_hip_lora_bgmv_supported(int out_features, int in_features, int max_rank, int rows) {
  return lora_shape_ok(out_features, in_features, max_rank, rows, AQLM_HIP_MAX_LORA_ROWS) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_bgmv(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids, int ids_int64,
                                  int rows, const void* x, long x_row_stride, void* y, long y_row_stride, int out_features,
                                  int in_features, int dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_bgmv";
  if (int e = lora_check_args(who, table, num_adapters, max_rank, ids, ids_int64, rows, x, x_row_stride, y, y_row_stride, out_features,
                              in_features, dtype, workspace, AQLM_HIP_MAX_LORA_ROWS))
    return e;
  if (int e = lora_check_workspace(who, workspace_bytes, aqlm_hip_lora_workspace_bytes(rows, max_rank))) return e;
  auto go = [&](auto t) {
    return launch_lora<decltype(t)>(table, num_adapters, max_rank, ids, ids_int64 ? 1 : 0, rows, (const uint16_t*)x, x_row_stride,
                                    (uint16_t*)y, y_row_stride, out_features, in_features, (float*)workspace, (hipStream_t)stream_);
  };
  return dtype == AQLM_HIP_F16 ? go(F16{}) : go(BF16{});
}

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
//   * shrink: one workgroup per (row, kShrinkRanks ranks); its waves own fixed contiguous shares of K (steps of 64 lanes x 16
//     bytes), every lane keeps one x piece and kShrinkRanks A pieces in flight per step; the wave sums meet in LDS and are added
//     in wave order.  A wave per rank would leave 16 waves streaming a whole row of 14336 elements each at rank 16 and one row.
//   * expand + add: a thread owns output i of row b: its rank x 2 contiguous bytes of B_a in 16-byte loads, t[b, :] from LDS
//     (every lane reads the same address: a broadcast), one read-modify-write of y[b, i].
// No atomics, no inter-workgroup communication; every sum has a fixed order that depends on the shapes only, so a row's bits
// depend on its own x row, its own y row and its adapter -- not on the other rows, their number or their order.
#include <algorithm>

#include "lora_common.h"

namespace aqlm {

constexpr int kShrinkWaves = 8;
constexpr int kShrinkRanks = 2;   // ranks per workgroup; divides every supported rank (multiples of 8)
constexpr int kShrinkStep = 512;  // elements of K per wave step: 64 lanes x 16 bytes
constexpr int kExpandThreads = 256;

template <class T>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_shrink_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                        const uint16_t* x, float* t, long xs, int ids_int64,
                                                                        int nadapters, int max_rank, int K8, int steps_per_wave) {
  const int b = blockIdx.y, r0 = blockIdx.x * kShrinkRanks;
  const long id = lora_row_id(ids, ids_int64, b, nadapters);
  if (id < 0) return;  // uniform over the workgroup
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + id);
  if (r0 >= lora_rank(ent->rank, max_rank)) return;  // a rank group past the row's own rank
  const lora_gbl_u32x4_ptr A = (lora_gbl_u32x4_ptr)(uintptr_t)ent->a + (long)r0 * K8;
  const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (long)b * xs);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float acc[kShrinkRanks] = {};
  const int s0 = wave * steps_per_wave;
#pragma unroll 4
  for (int s = 0; s < steps_per_wave; ++s) {
    const int k8 = (s0 + s) * 64 + lane;
    const bool live = k8 < K8;
    const int kc = live ? k8 : K8 - 1;  // loads are unconditional from a clamped address; the tail is masked at the use
    const u32x4 xv = xrow[kc];
    u32x4 av[kShrinkRanks];
#pragma unroll
    for (int r = 0; r < kShrinkRanks; ++r) av[r] = A[(long)r * K8 + kc];
#pragma unroll
    for (int r = 0; r < kShrinkRanks; ++r) {
      const float d = dot8<T>(av[r], xv, acc[r]);
      acc[r] = live ? d : acc[r];
    }
  }

  __shared__ float part[kShrinkWaves][kShrinkRanks];
#pragma unroll
  for (int r = 0; r < kShrinkRanks; ++r) {
    const float v = wave_sum(acc[r]);
    if (lane == 0) part[wave][r] = v;
  }
  __syncthreads();
  if (threadIdx.x < kShrinkRanks) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kShrinkWaves; ++w) v += part[w][threadIdx.x];  // the shares meet in wave order
    t[(long)b * max_rank + r0 + threadIdx.x] = v;
  }
}

template <class T>
__global__ __launch_bounds__(kExpandThreads) void lora_expand_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                     const float* t, uint16_t* y, long ys, int ids_int64,
                                                                     int nadapters, int max_rank, int M) {
  const int b = blockIdx.y;
  const long id = lora_row_id(ids, ids_int64, b, nadapters);
  if (id < 0) return;
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + id);
  const int rank = lora_rank(ent->rank, max_rank);
  if (rank == 0) return;
  const float scaling = ent->scaling;

  __shared__ __attribute__((aligned(16))) float ts[kLoraMaxRank];
  if ((int)threadIdx.x < rank) ts[threadIdx.x] = t[(long)b * max_rank + threadIdx.x];
  __syncthreads();

  const int i = blockIdx.x * kExpandThreads + threadIdx.x;
  if (i >= M) return;
  uint16_t* yp = y + (long)b * ys + i;
  const uint16_t y0 = *yp;
  const int pieces = rank >> 3;
  const lora_gbl_u32x4_ptr B = (lora_gbl_u32x4_ptr)(uintptr_t)ent->b + (long)i * pieces;
  float acc = 0.f;
#pragma unroll 2
  for (int c = 0; c < pieces; ++c) {
    const u32x4 bv = B[c];
    const float4 t0 = reinterpret_cast<const float4*>(ts)[2 * c], t1 = reinterpret_cast<const float4*>(ts)[2 * c + 1];
    acc = fmaf(T::lo(bv.x), t0.x, acc);
    acc = fmaf(T::hi(bv.x), t0.y, acc);
    acc = fmaf(T::lo(bv.y), t0.z, acc);
    acc = fmaf(T::hi(bv.y), t0.w, acc);
    acc = fmaf(T::lo(bv.z), t1.x, acc);
    acc = fmaf(T::hi(bv.z), t1.y, acc);
    acc = fmaf(T::lo(bv.w), t1.z, acc);
    acc = fmaf(T::hi(bv.w), t1.w, acc);
  }
  *yp = T::from_float(fmaf(scaling, acc, T::to_float(y0)));
}

template <class T>
static int launch_lora(const aqlm_hip_lora_entry* table, int nadapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const uint16_t* x, long xs, uint16_t* y, long ys, int M, int K, float* t, hipStream_t stream) {
  const int K8 = K / 8;
  const int steps = (K + kShrinkStep - 1) / kShrinkStep;
  const int steps_per_wave = (steps + kShrinkWaves - 1) / kShrinkWaves;
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

// The per-row arithmetic of the batched LoRA adapter matvec, shared by aqlm_hip_lora_bgmv (lora_bgmv.hip: a row is a row of the
// batch, its adapter comes from one id) and aqlm_hip_lora_bgmv_routed (lora_bgmv_routed.hip: a row is a (token, expert) pair and
// a projection, its adapter comes from an adapter id and an expert id).  A kernel finds its table entry, its x row, its t row and
// its y row -- and returns before it gets here when the row has no adapter -- and hands them to these bodies, so both launches
// run the same operations in the same order: a row's bits are the same whichever of the two computed it.
//   * shrink: one workgroup per (row, kShrinkRanks ranks); its waves own fixed contiguous shares of K (steps of 64 lanes x 16
//     bytes), every lane keeps one x piece and kShrinkRanks A pieces in flight per step; the wave sums meet in LDS and are added
//     in wave order.  A wave per rank would leave 16 waves streaming a whole row of 14336 elements each at rank 16 and one row.
//   * expand + add: a thread owns output i of the row: its rank x 2 contiguous bytes of B in 16-byte loads, t from LDS (every
//     lane reads the same address: a broadcast), one read-modify-write of y[i].
// Every call of a workgroup is uniform (both bodies hold a barrier).
#pragma once
#include "lora_common.h"

namespace aqlm {

constexpr int kShrinkWaves = 8;
constexpr int kShrinkRanks = 2;   // ranks per workgroup; divides every supported rank (multiples of 8)
constexpr int kShrinkStep = 512;  // elements of K per wave step: 64 lanes x 16 bytes
constexpr int kExpandThreads = 256;

inline int lora_shrink_steps_per_wave(int K) {
  const int steps = (K + kShrinkStep - 1) / kShrinkStep;
  return (steps + kShrinkWaves - 1) / kShrinkWaves;
}

// t[r0 .. r0 + kShrinkRanks) of one row: `trow` its fp32 row of the workspace, `xrow` its input row
template <class T>
__device__ __forceinline__ void lora_shrink_body(lora_entry_ptr ent, const u32x4* xrow, float* trow, int r0, int max_rank, int K8,
                                                 int steps_per_wave) {
  if (r0 >= lora_rank(ent->rank, max_rank)) return;  // a rank group past the row's own rank
  const lora_gbl_u32x4_ptr A = (lora_gbl_u32x4_ptr)(uintptr_t)ent->a + (long)r0 * K8;

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
    trow[r0 + threadIdx.x] = v;
  }
}

// outputs i0 .. i0 + kExpandThreads of one row: y[i] = round(float(y[i]) + scaling * sum_r B[i, r] * t[r])
template <class T>
__device__ __forceinline__ void lora_expand_body(lora_entry_ptr ent, const float* trow, uint16_t* yrow, int i0, int max_rank, int M) {
  const int rank = lora_rank(ent->rank, max_rank);
  if (rank == 0) return;
  const float scaling = ent->scaling;

  __shared__ __attribute__((aligned(16))) float ts[kLoraMaxRank];
  if ((int)threadIdx.x < rank) ts[threadIdx.x] = trow[threadIdx.x];
  __syncthreads();

  const int i = i0 + threadIdx.x;
  if (i >= M) return;
  uint16_t* yp = yrow + i;
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

}  // namespace aqlm

// Types, LDS map and plan of the 16-row fused 1x16 MFMA GEMM (a block owns 16 output rows over all of K; gemm_1x16_rows16.h, a part
// of gemm_mfma.hip, describes the design), shared by gemm_1x16_rows16_kernel (there) and the expert-grouped kernel of
// moe_grouped.hip.  The kernel body itself is gemm_rows16_body.h.
#pragma once
#include <algorithm>

#include "aqlm_common.h"

namespace aqlm {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 64;  // k depth of one LDS chunk of X

// LDS image of one X chunk: row b (batch) holds 64 k = 8 pieces of 16 B; piece c is stored at slot c ^ ((b>>1)&7) so
// that the 16 lanes of a ds_read_b128 service group (16 distinct b mod 16) hit 16 distinct 16-B slots.
__device__ __forceinline__ int xswz(int b, int c) { return b * 8 + (c ^ ((b >> 1) & 7)); }

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <class T>
__device__ __forceinline__ f32x4 mfma16(const u32x4& a, const u32x4& b, const f32x4& c);
template <>
__device__ __forceinline__ f32x4 mfma16<F16>(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<BF16>(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

typedef __attribute__((address_space(3))) const u32x4* glds_u32x4_ptr;
typedef __attribute__((address_space(3))) const uint16_t* glds_u16_ptr;
typedef __attribute__((address_space(3))) void* glds_void_ptr;
typedef __attribute__((address_space(1))) const void* ggbl_void_ptr;

constexpr int gl_vmcnt(int n) { return (n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14); }  // vmcnt(n) only

constexpr int R16_NC = 4;     // consumer waves

template <int NBT, int CPB>
struct R16Lds {
  static constexpr int NXP = 2 * NBT >= 4 ? 4 : 2 * NBT;            // X producer waves
  static constexpr int PXW = CPB * 2 * NBT / NXP;                   // 1-KiB pieces (8 batch rows x 64 k) per X wave and step
  static constexpr uint32_t X_CHUNK = (uint32_t)NBT * 2048u;        // 16 NBT batch rows x 128 B
  static constexpr uint32_t X_STAGE = CPB * X_CHUNK;
  static constexpr uint32_t W_STAGE = CPB * 2048u;                  // 2 fragments of 1 KiB per chunk
  // Ring depths.  Steps of several chunks carry 256-512 lane-gathers each, so 3 steps in flight cover the gather latency; short
  // rings also mean a short prologue and, at <= 16 rows, 72 KiB of LDS: two blocks per CU, whose prologues and tails overlap
  // (measured against 8-stage rings: 4096 -> 11008 at 16 rows 33.1 -> 30.5 us, 4096^2 13.7 -> 13.2).
#ifndef AQLM_R16_DEEP
#define AQLM_R16_DEEP 0  // 1: the first cut's 8-stage rings (A/B builds)
#endif
  static constexpr int NSW = CPB == 1 ? 16 : (AQLM_R16_DEEP ? 8 : 4);  // stages of the fragment ring
  static constexpr int NSX = CPB == 1 ? (NBT <= 2 ? 16 : (NBT <= 4 ? 12 : 7))   // stages of the X ring: as deep in TIME as a load takes,
                             : AQLM_R16_DEEP ? (CPB == 4 ? (NBT <= 1 ? 8 : 4) : (NBT <= 4 ? 6 : 3))
                                             : (CPB == 4 ? (NBT <= 1 ? 4 : 3) : (NBT <= 4 ? 4 : 3));  // within 160 KiB
  static constexpr int NSLOT = 2 * NSW;                             // slots of the code ring (power of two)
  static constexpr uint32_t CODE_SLOT = 256u * CPB;                 // 16 rows x CPB x 16 B (g = 8) or x 8 B (g = 16, half used)
  static constexpr uint32_t W = 0;
  static constexpr uint32_t X = NSW * W_STAGE;
  static constexpr uint32_t CODES = X + NSX * X_STAGE;
  static constexpr uint32_t TOTAL = CODES + NSLOT * CODE_SLOT;
  static constexpr int WAVES = 1 + NXP + R16_NC;
  static_assert(TOTAL <= 160u * 1024u, "LDS");
  static_assert((NSLOT & (NSLOT - 1)) == 0, "code ring");
};

template <int R, int P>  // the last R + 1 steps land: one counted wait + barrier each (the wait count must be an immediate)
__device__ __forceinline__ void r16_drain() {
  __builtin_amdgcn_s_waitcnt(gl_vmcnt(R * P));
  __builtin_amdgcn_s_barrier();
  if constexpr (R > 0) r16_drain<R - 1, P>();
}

struct R16Params {
  const uint8_t* codes;     // [M][in_groups] u16
  const uint8_t* codebook;  // [65536][G] halfs
  const uint16_t* X;        // [B][xs]
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  long xs, ys;
  int M, B, in_groups, nsteps;  // nsteps = K / (64 CPB)
};

struct R16Plan {
  int nbt, cpb, nsteps;
};

// chunks per step: 4 for <= 32 rows, 2 above, where K is a multiple of the step and long enough for the rings; else 1
static bool plan_rows16(int B, int K, int G, R16Plan& r) {
  if (K % BK != 0 || B < 1 || B > 128) return false;
  const int t = (B + 15) / 16;
  r.nbt = t <= 1 ? 1 : (t <= 2 ? 2 : (t <= 4 ? 4 : 8));
  const int want = r.nbt <= 2 ? 4 : 2;
  const int chunks = K / BK;
  // (steps of several chunks move the codes in 16-B pieces: the rows of the code matrix must then be 16-B aligned)
  if (chunks % want == 0 && chunks / want >= 7 && ((K / G) * 2) % 16 == 0) r.cpb = want;  // (7 steps: any ring depth of the several-chunk configurations)
  else if (chunks >= 15) r.cpb = 1;                            // rings of 16 / <= 16 stages
  else return false;
  r.nsteps = chunks / r.cpb;
  return true;
}

}  // namespace aqlm

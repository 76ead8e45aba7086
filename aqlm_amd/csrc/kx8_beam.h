// What the two K x 8 code searches share (code_search_kx8.hip, code_search_kx8_xtx.hip): the product that stays a product, the
// widening of a lane's candidates, their dot products against one LDS row, the order-preserving score keys, the wave minima, and
// on the host side the scheme check, the dim_order parse and the launch ladder.  The selection of the best `keep` keys, built on
// these, is kx8_select_body.h.  Both kernels are held to their own arithmetic bit for bit, so every product and sum here is one
// IEEE fp32 operation: contraction is off from here to the end of the translation unit.
#pragma once
#include "aqlm_common.h"

#pragma clang fp contract(off)

namespace aqlm {

constexpr int kKxbEntries = 256;
constexpr int kKxbMaxBooks = 8;
constexpr int kKxbPerLane = kKxbEntries / WAVE;  // candidates per lane: 4
constexpr unsigned kKxbMaxBlocks = 256 * 32;     // grid-stride above this

// A product that the sum after it cannot absorb.  The pragma above stops the front end from forming fused multiply-adds, but the
// library is built with an explicit -ffp-contract=fast, under which the code generator fuses any product with the sum that uses it
// whatever the pragma says; a product that has passed through an (empty) asm operand is no longer a product to it.  No instruction
// is emitted for the barrier.
static __device__ __forceinline__ float kxb_mul(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));
  return p;
}

// lane's candidates s = 4 lane .. 4 lane + 3 of codebook c, widened: one contiguous 8 G bytes per lane
template <class T, int G>
static __device__ __forceinline__ void kxb_load_candidates(const uint16_t* codebooks, int c, int lane, float (&cw)[kKxbPerLane][G]) {
  const u32x4* src = reinterpret_cast<const u32x4*>(codebooks + ((size_t)c * kKxbEntries + (size_t)kKxbPerLane * lane) * G);
#pragma unroll
  for (int q = 0; q < kKxbPerLane; ++q)
#pragma unroll
    for (int p = 0; p < G / 8; ++p) {
      const u32x4 w = src[q * (G / 8) + p];
      cw[q][8 * p + 0] = T::lo(w.x); cw[q][8 * p + 1] = T::hi(w.x);
      cw[q][8 * p + 2] = T::lo(w.y); cw[q][8 * p + 3] = T::hi(w.y);
      cw[q][8 * p + 4] = T::lo(w.z); cw[q][8 * p + 5] = T::hi(w.z);
      cw[q][8 * p + 6] = T::lo(w.w); cw[q][8 * p + 7] = T::hi(w.w);
    }
}

// acc[q] = <row, cw[q]> for the lane's four candidates: `row` is a 16-byte-aligned LDS row (a wave-uniform broadcast), the sum runs
// over the elements ascending and starts from the first product
template <int G>
static __device__ __forceinline__ void kxb_dot4(const float (&row)[G], const float (&cw)[kKxbPerLane][G], float (&acc)[kKxbPerLane]) {
  const float4* rp = reinterpret_cast<const float4*>(row);
#pragma unroll
  for (int p = 0; p < G / 4; ++p) {
    const float4 rv = rp[p];
    const float re[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < kKxbPerLane; ++q) {
        const float prod = kxb_mul(re[t], cw[q][4 * p + t]);
        acc[q] = (p == 0 && t == 0) ? prod : acc[q] + prod;
      }
  }
}

// fp32 bits <-> unsigned integers in the order of the floats (-0 sorts below +0: a caller whose score can be -0 maps it to +0 first)
static __device__ __forceinline__ uint32_t kxb_ordered(float s) {
  const uint32_t b = __float_as_uint(s);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
static __device__ __forceinline__ float kxb_unordered(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// minimum over the wave of a 64-bit key (DPP within the rows, scalar across them); wave-uniform result
template <int CTRL>
static __device__ __forceinline__ uint64_t kxb_dpp_min(uint64_t v) {
  const uint64_t o = ((uint64_t)dpp_u32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)v);
  return o < v ? o : v;
}
static __device__ __forceinline__ uint64_t kxb_wave_min(uint64_t v) {
  v = kxb_dpp_min<0xB1>(v);
  v = kxb_dpp_min<0x4E>(v);
  v = kxb_dpp_min<0x141>(v);
  v = kxb_dpp_min<0x140>(v);
  uint64_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 16 * i) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 16 * i);
  const uint64_t x = r[0] < r[1] ? r[0] : r[1], y = r[2] < r[3] ? r[2] : r[3];
  return x < y ? x : y;
}
static __device__ __forceinline__ uint32_t kxb_wave_min_u32(uint32_t v) {
  uint32_t o;
  o = dpp_u32<0xB1>(v);  v = o < v ? o : v;
  o = dpp_u32<0x4E>(v);  v = o < v ? o : v;
  o = dpp_u32<0x141>(v); v = o < v ? o : v;
  o = dpp_u32<0x140>(v); v = o < v ? o : v;
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  const uint32_t a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
  return a < b ? a : b;
}

// The selection of the best `keep` keys is kx8_select_body.h: text that both kernels include where they select.

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline bool kxb_search_scheme_ok(int num_codebooks, int g, int beam_size) {
  return num_codebooks >= 1 && num_codebooks <= kKxbMaxBooks && (g == 8 || g == 16 || g == 32) && beam_size >= 1 &&
         beam_size <= AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM;
}

// order[i] = dim_order[i] (null: i); 0, or the message and AQLM_HIP_E_INVALID when it is no permutation of 0 .. K - 1
inline int kxb_parse_dim_order(const char* who, const int* dim_order, int num_codebooks, signed char (&order)[kKxbMaxBooks]) {
  unsigned seen = 0;
  for (int i = 0; i < num_codebooks; ++i) {
    const int c = dim_order ? dim_order[i] : i;
    if (c < 0 || c >= num_codebooks || (seen >> c & 1u)) {
      set_last_error("%s: dim_order must be a permutation of 0 .. %d (entry %d is %d)", who, num_codebooks - 1, i, c);
      return AQLM_HIP_E_INVALID;
    }
    seen |= 1u << c;
    order[i] = (signed char)c;
  }
  return 0;
}

// the launch ladder of both entries: f(F16{} or BF16{}, GroupSize<g>{}, GroupSize<PMAX>{}) with PMAX = 1 / 4 / 8 / 16, the smallest
// that holds `width` positions (each entry has its own rule for the width)
template <class F>
inline int kxb_dispatch(int dtype, int g, int width, F&& f) {
  auto by_width = [&](auto t, auto gs) {
    if (width == 1) return f(t, gs, GroupSize<1>{});
    if (width <= 4) return f(t, gs, GroupSize<4>{});
    if (width <= 8) return f(t, gs, GroupSize<8>{});
    return f(t, gs, GroupSize<16>{});
  };
  auto by_group = [&](auto t) {
    if (g == 8) return by_width(t, GroupSize<8>{});
    if (g == 16) return by_width(t, GroupSize<16>{});
    return by_width(t, GroupSize<32>{});
  };
  return dtype == AQLM_HIP_F16 ? by_group(F16{}) : by_group(BF16{});
}

}  // namespace aqlm

// The direct dequant-fused matvec body shared by gemv.hip (single-matrix and shared-input launches) and gemv_routed.hip
// (expert-routed launches of a mixture-of-experts block).  Design notes: gemv.hip's header comment.
#pragma once
#include "aqlm_common.h"

namespace aqlm {

struct GemvParams {
  const uint8_t* codes;
  const uint8_t* codebooks;
  const uint16_t* scales;
  const uint16_t* bias;  // nullable
  const uint16_t* x;
  uint16_t* y;
  int M;              // out_features
  int in_groups;      // in_features / G
  int nunits;         // in_groups / U
  int iters;          // ceil(nunits / 64)
  int pitch;          // LDS pitch (in 16-B pieces) of one (b,i,piece) row of the x tile
  int rpw;            // rows per wave
  int prefetch;       // 1x16 only: warm the XCD's L2 with a slice of the codebook first
  int cb_bytes;       // total codebook bytes
  long xs, ys;        // row strides of x / y in elements
  long code_row_bytes;
};

// Gathered rows (GATHER = true; gemv_routed.hip): batch slot b reads x row (xrows >> 6b) & 63 and writes y row (yrows >> 6b) & 63
// (strides xs / ys as usual); slots b >= nvalid run on a valid row but write nothing.  The row lists are wave-uniform registers, so
// the per-slot lookup is a shift, never an indexed private array.
struct GemvGather {
  uint64_t xrows = 0, yrows = 0;
  int nvalid = 0;
};

template <int N>
__device__ __forceinline__ void load_code_word(const uint8_t* p, uint32_t (&cw)[N]) {
  if constexpr (N == 4) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    cw[0] = v.x; cw[1] = v.y; cw[2] = v.z; cw[3] = v.w;
  } else {
    static_assert(N == 2, "code word is 8 or 16 bytes");
    const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    cw[0] = v.x; cw[1] = v.y;
  }
}

// T: F16/BF16; CODE_BYTES: 1|2; KC: codebooks; G: in_group_size; U: groups per lane-unit; NB: batch rows;
// CB_LDS: codebooks in LDS (Kx8) or L2 gathers (1x16); NWAVES: waves per block; AUX: gather cache policy.
// `block` is the workgroup's index within its own code matrix (== blockIdx.x for a single-matrix launch).
// GATHER: the batch rows come from / go to the row lists of `gather` instead of rows 0..NB-1.
template <class T, int CODE_BYTES, int KC, int G, int U, int NB, bool CB_LDS, int NWAVES, int AUX, bool GATHER = false>
__device__ __forceinline__ void gemv_body(const GemvParams& p, const int block, const GemvGather& gather = GemvGather{}) {
  constexpr int P = G / 8;                  // 16-B pieces per codebook vector
  constexpr int UB = U * KC * CODE_BYTES;   // code bytes per unit
  constexpr int CW = UB / 4;
  static_assert(UB == 8 || UB == 16, "unit must be 8 or 16 code bytes");
  constexpr int NT = NWAVES * 64;
  constexpr int CB_SIZE = CB_LDS ? 256 : 65536;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* const xl = reinterpret_cast<u32x4*>(smem_raw);
  u32x4* const cbl = xl + NB * U * P * p.pitch;  // only touched when CB_LDS

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = (block * NWAVES + wave) * p.rpw;
  int nrows = p.M - row0;
  nrows = nrows < p.rpw ? nrows : p.rpw;

  // ---- prologue: every global load is issued before the first wait (no load-wait-store loops: hipcc puts a
  // vmcnt(0) in front of each ds_write of such a loop, i.e. one L2 round trip per iteration, ~1 us per kernel).
  // (a) x pieces, 8 per thread, staged in registers (clamped, always-valid addresses)
  const int pieces_per_row = p.in_groups * P;
  const int total_x = NB * pieces_per_row;
  auto x_piece = [&](int q) -> u32x4 {
    q = q < total_x ? q : total_x - 1;
    int b = 0, qq = q;
    if constexpr (NB > 1) { b = q / pieces_per_row; qq = q - b * pieces_per_row; }
    if constexpr (GATHER) b = (int)((gather.xrows >> (6 * b)) & 63u);
    return *reinterpret_cast<const u32x4*>(p.x + (long)b * p.xs + (long)qq * 8);
  };
  auto x_store = [&](int q, const u32x4& v) {
    if (q < total_x) {
      int b = 0, qq = q;
      if constexpr (NB > 1) { b = q / pieces_per_row; qq = q - b * pieces_per_row; }
      const int j = qq / P, pp = qq % P;
      const int u = j / U, i = j % U;
      xl[((b * U + i) * P + pp) * p.pitch + u] = v;
    }
  };
  u32x4 xstage[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) xstage[k] = x_piece(tid + k * NT);

  // (b) scale / bias of the first row: unconditional loads (clamped row; bias pointer aliased to scales when absent)
  const uint16_t* const bias_src = p.bias ? p.bias : p.scales;
  const float bias_on = p.bias ? 1.f : 0.f;
  const int row_c0 = row0 < p.M ? row0 : p.M - 1;
  uint16_t scale_h = p.scales[row_c0], bias_h = bias_src[row_c0];

  // (c) first code word (HBM latency overlaps the LDS fill)
  uint32_t cw_next[CW];
#pragma unroll
  for (int k = 0; k < CW; ++k) cw_next[k] = 0;
  if (nrows > 0 && lane < p.nunits) load_code_word<CW>(p.codes + (long)row0 * p.code_row_bytes + (long)lane * UB, cw_next);

  // (d) codebooks (Kx8): staged the same way, compile-time trip count
  if constexpr (CB_LDS) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.codebooks);
    constexpr int TOTAL = KC * 256 * P;
    constexpr int PER = (TOTAL + NT - 1) / NT;
    u32x4 cstage[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) cstage[k] = src[tid + k * NT < TOTAL ? tid + k * NT : TOTAL - 1];
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (tid + k * NT < TOTAL) cbl[tid + k * NT] = cstage[k];
  }
  // (e) x -> LDS: element (b, group j = u*U+i, piece pp) -> xl[((b*U+i)*P+pp)*pitch + u]
#pragma unroll
  for (int k = 0; k < 8; ++k) x_store(tid + k * NT, xstage[k]);
  for (int q0 = tid + 8 * NT; q0 < total_x; q0 += NT * 4) {  // rare: more than 8 pieces per thread (large batch x K)
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x_piece(q0 + k * NT);
#pragma unroll
    for (int k = 0; k < 4; ++k) x_store(q0 + k * NT, v[k]);
  }

  // optional: touch a 16 KiB slice of the codebook so that this XCD's L2 is warm before the random gathers
  u32x4 pf[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pf[k] = u32x4{0u, 0u, 0u, 0u};
  if constexpr (!CB_LDS) {
    if (p.prefetch) {
      const int nchunks = p.cb_bytes >> 14;  // 16 KiB chunks
      const int chunk = (block >> 3) % (nchunks > 0 ? nchunks : 1);
      const u32x4* src = reinterpret_cast<const u32x4*>(p.codebooks + ((long)chunk << 14));
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (NT == 256 || tid < 256) pf[k] = src[k * 256 + (tid & 255)];
    }
  }
  __syncthreads();

  __amdgpu_buffer_rsrc_t rsrc;
  if constexpr (!CB_LDS) rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.codebooks, 0, p.cb_bytes, 0x00020000);

  for (int r = 0; r < nrows; ++r) {
    const int row = row0 + r;
    const float scale = T::to_float(scale_h);
    const float bias = T::to_float(bias_h) * bias_on;
    {
      const int rn = row + 1 < p.M ? row + 1 : p.M - 1;  // next row's epilogue operands (unused after the last row)
      scale_h = p.scales[rn];
      bias_h = bias_src[rn];
    }
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;

    for (int it = 0; it < p.iters; ++it) {
      const int u = it * 64 + lane;
      uint32_t cw[CW];
#pragma unroll
      for (int k = 0; k < CW; ++k) cw[k] = cw_next[k];
      // software prefetch of the next (row, iteration) code word
      {
        int nit = it + 1, nr = r;
        if (nit == p.iters) { nit = 0; nr = r + 1; }
        const int nu = nit * 64 + lane;
        if (nr < nrows && nu < p.nunits)
          load_code_word<CW>(p.codes + (long)(row0 + nr) * p.code_row_bytes + (long)nu * UB, cw_next);
      }
      if (u < p.nunits) {
        if constexpr (!CB_LDS) {
          // issue every gather of this unit before consuming any (8-16 x 16 B in flight per lane)
          u32x4 ent[U * KC * P];
#pragma unroll
          for (int i = 0; i < U; ++i)
#pragma unroll
            for (int c = 0; c < KC; ++c) {
              const uint32_t code = code_at<CODE_BYTES>(cw, i * KC + c);
              const uint32_t off = (uint32_t)(c * CB_SIZE + code) * (uint32_t)(G * 2);
#pragma unroll
              for (int pp = 0; pp < P; ++pp)
                ent[(i * KC + c) * P + pp] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + pp * 16, 0, AUX);
            }
#pragma unroll
          for (int i = 0; i < U; ++i)
#pragma unroll
            for (int pp = 0; pp < P; ++pp)
#pragma unroll
              for (int b = 0; b < NB; ++b) {
                const u32x4 xv = xl[((b * U + i) * P + pp) * p.pitch + u];
#pragma unroll
                for (int c = 0; c < KC; ++c) acc[b] = dot8<T>(ent[(i * KC + c) * P + pp], xv, acc[b]);
              }
        } else {
#pragma unroll
          for (int i = 0; i < U; ++i)
#pragma unroll
            for (int pp = 0; pp < P; ++pp) {
              u32x4 xv[NB];
#pragma unroll
              for (int b = 0; b < NB; ++b) xv[b] = xl[((b * U + i) * P + pp) * p.pitch + u];
#pragma unroll
              for (int c = 0; c < KC; ++c) {
                const uint32_t code = code_at<CODE_BYTES>(cw, i * KC + c);
                const u32x4 e = cbl[(c * 256 + code) * P + pp];
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = dot8<T>(e, xv[b], acc[b]);
              }
            }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = wave_sum(acc[b]);
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if constexpr (GATHER) {
          if (b < gather.nvalid)
            p.y[(long)((gather.yrows >> (6 * b)) & 63u) * p.ys + row] = T::from_float(__builtin_fmaf(acc[b], scale, bias));
        } else {
          p.y[(long)b * p.ys + row] = T::from_float(__builtin_fmaf(acc[b], scale, bias));
        }
      }
    }
  }
  // keep the prefetch loads alive without ever waiting on them early
#pragma unroll
  for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(pf[k]));
}

}  // namespace aqlm

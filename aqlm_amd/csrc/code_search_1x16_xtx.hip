// The calibrated code search of the 1x16 schemes (one codebook of 65536 entries, out_group_size 1, g = 8 / 16): one input group of the
// reference's src/beam_search_xtx.py for every output row of one layer (aqlm_hip_code_search_1x16_xtx; include/aqlm_hip.h has the
// definition, DESIGN.md 4.8q the bound, the mapping and the numbers).  It is aqlm_hip_code_search_kx8_xtx with K = 1 and 65536
// candidates per position, held to the same arithmetic bit for bit (tests/x16_xtx_model.py restates it in numpy): every product and
// every sum of the definition is one IEEE fp32 operation, so contraction is off and every such product passes through kxb_mul.
//
// positions x 65536 exact scores per row are too many for the VALU, so the matrix unit FILTERS and the VALU REFINES:
//   columns    a column is a (row, position) pair, n = o * positions + b.  A wave (a workgroup of 64 threads) owns 128 columns (4 tiles
//              of 32) and one split of the codebook, grid = column blocks x splits.  Its prologue forms u[b], base[b] of the
//              definition exactly, per column, and keeps them in LDS.
//   scan       code_search.hip's: codewords along M of v_mfma_f32_32x32x16, columns along N; B is u scaled by an exact power of two
//              to max|u| in [2^10, 2^11) and split into hi + lo of the codebook dtype (g = 8: one instruction, lanes 0-31 carry
//              hi, lanes 32-63 lo; g = 16: two).  A~ = fma(acc, -2s * 2^(e - 10), fma(q[s'], ss, base)): two VALU operations per score.
//   filter     per column the wave keeps the beam_size smallest EXACT keys (ordered bits of S, b * 65536 + s') it has met, unsorted,
//              and the largest score among them (+Inf while fewer are held).  A candidate is re-scored exactly -- the definition,
//              operation for operation -- unless A~ > worst + E, E >= |A~ - S| for every candidate of the column (x16_bound below).
//              The worst score only falls, so no member of the answer is ever skipped, whatever the order of the scan; the scan
//              never decides anything.  NaN scores enter no list.
//   merge      a second launch: one wave per row takes the beam_size smallest keys of the row's splits x positions lists in order
//              (keys are unique, so the merge does not depend on any order) and writes codes, sources, losses, delta and t.  A row
//              with fewer non-NaN scores than beam_size is filled with position 0 and the smallest codes not yet present, loss NaN.
// A first launch finds max|C| and max|q| (E needs them).  No address, LDS slot or loop bound is formed from a score: a list slot is
// a count or the rank of a comparison, both clamped below beam_size.  No global atomics, no scratch, no allocation; the output is a
// function of the arguments alone.
#include "kx8_beam.h"

#pragma clang fp contract(off)

namespace aqlm {

constexpr int kX16Entries = 65536;
constexpr int kX16Tiles = 4;                     // column tiles of 32 per wave
constexpr int kX16Cols = kX16Tiles * 32;         // 128
constexpr int kX16CodeTiles = kX16Entries / 32;  // codeword tiles of 32: 2048
constexpr int kX16MaxBeam = AQLM_HIP_CODE_SEARCH_1X16_XTX_MAX_BEAM;
constexpr int kX16MaxSplits = 64;
constexpr int kX16WantWaves = 2048;  // the splits double until the grid holds this many waves
constexpr int kX16MaxBlocks = 256;   // workgroups of the first launch: 256 codewords each
constexpr unsigned kX16MergeBlocks = 256 * 32;
constexpr uint64_t kX16Empty = ~0ull;  // the ordered bits of a NaN: no key that was taken

typedef float x16_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 x16_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 x16_bf16x8 __attribute__((ext_vector_type(8)));

template <class T>
static __device__ __forceinline__ x16_f32x16 x16_mfma(const u32x4& a, const u32x4& b, const x16_f32x16& c) {
  if constexpr (T::id == AQLM_HIP_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x16_f16x8, a), __builtin_bit_cast(x16_f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x16_bf16x8, a), __builtin_bit_cast(x16_bf16x8, b), c, 0, 0, 0);
}

struct X16XtxArgs {
  const float* t;            // [positions_in][out][g], strided
  const float* loss;         // [positions_in][out]
  const int16_t* codes_in;   // [positions_in][out]
  const float* h;            // [g][g]
  const float* q;            // [65536]
  const uint16_t* codebook;  // [65536][g]
  const uint16_t* scales;    // [out] or null
  float* loss_out;           // [beam][out]
  int16_t* codes_out;        // [beam][out]
  uint8_t* source;           // [beam][out]
  float* delta;              // [beam][out][g]
  float* t_out;              // [beam][out][g] or null
  float* maxima;             // workspace: [2][kX16MaxBlocks]
  uint64_t* keys;            // workspace: [splits][columns][beam]
  long t_pos_stride, t_row_stride;  // elements
  long columns;                     // out * positions_in
  int out;
  int beam;
  int positions_in;
  int splits;
};

static __device__ __forceinline__ float x16_plus_zero(float s) {
  const uint32_t b = __float_as_uint(s);
  return __uint_as_float(b == 0x80000000u ? 0u : b);
}
// |x|, with NaN counted as Inf (a maximum must not lose it)
static __device__ __forceinline__ float x16_mag(float x) {
  const float ax = __builtin_fabsf(x);
  return ax < __builtin_inff() ? ax : __builtin_inff();
}
static __device__ __forceinline__ float x16_wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, d));
  return v;
}
// codeword `code` widened to fp32
template <class T, int G>
static __device__ __forceinline__ void x16_entry(const uint16_t* codebook, uint32_t code, float (&cw)[G]) {
  const u32x4* src = reinterpret_cast<const u32x4*>(codebook + (size_t)code * G);
#pragma unroll
  for (int p = 0; p < G / 8; ++p) {
    const u32x4 w = src[p];
    cw[8 * p + 0] = T::lo(w.x); cw[8 * p + 1] = T::hi(w.x);
    cw[8 * p + 2] = T::lo(w.y); cw[8 * p + 3] = T::hi(w.y);
    cw[8 * p + 4] = T::lo(w.z); cw[8 * p + 5] = T::hi(w.z);
    cw[8 * p + 6] = T::lo(w.w); cw[8 * p + 7] = T::hi(w.w);
  }
}

// ---- launch 1: max|C| and max|q| per 256 codewords ----
template <class T, int G>
__global__ __launch_bounds__(256) void code_search_1x16_xtx_maxima_kernel(const uint16_t* __restrict__ codebook, const float* __restrict__ q,
                                                                          float* __restrict__ maxima) {
  __shared__ float red[2][4];
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  float cw[G];
  x16_entry<T, G>(codebook, c, cw);
  float cm = 0.f;
#pragma unroll
  for (int f = 0; f < G; ++f) cm = __builtin_fmaxf(cm, x16_mag(cw[f]));
  cm = x16_wave_max(cm);
  const float qm = x16_wave_max(x16_mag(q[c]));
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[0][threadIdx.x / WAVE] = cm;
    red[1][threadIdx.x / WAVE] = qm;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* r = red[threadIdx.x];
    maxima[threadIdx.x * kX16MaxBlocks + blockIdx.x] = __builtin_fmaxf(__builtin_fmaxf(r[0], r[1]), __builtin_fmaxf(r[2], r[3]));
  }
}

// E of one column (DESIGN.md 4.8q derives it): |A~ - S| <= E for every candidate, and E covers the rounding of `worst + E` too.
//   A = |2s| g U cmax bounds |2s <C, u>| (U = 2^(e + 1) > max|u|, 0 for u = 0), B = |base|, Q = |ss| max|q|.
//   in units of 2^-24 A: the split of u (fp16 2^-21 with a matrix unit that flushes subnormal operands, bf16 2^-18), the 2g fp32
//   additions of the matrix unit at 2^-23 each (4g), the g + 4 roundings of the definition and of A~ on this term, one for the
//   threshold; on B + Q five roundings (2^-21 covers them); subnormal codebook entries that a matrix unit may flush (F); a margin
//   of 2^-6 for the second-order terms and the roundings of this expression; absolute terms for products that underflow.
// Outside a range in which every intermediate is finite the bound is +Inf: every candidate of the column is refined.
template <class T, int G>
static __device__ __forceinline__ float x16_bound(float two_s, float ub, float cmax, float base, float ss, float qmax, float k, bool bad) {
  constexpr float kUnits = (T::id == AQLM_HIP_F16 ? 8.f : 64.f) + 5.f * G + 5.f;
  constexpr float kFlush = T::id == AQLM_HIP_F16 ? 0x1p-14f : 0x1p-126f;
  const float a2 = __builtin_fabsf(two_s);
  const float A = a2 * ((float)G * ub) * cmax;
  const float F = a2 * ((float)G * ub) * kFlush;
  const float B = __builtin_fabsf(base);
  const float Q = __builtin_fabsf(ss) * qmax;
  float E = ((kUnits * 0x1p-24f) * A + F + 0x1p-21f * (B + Q)) * (1.f + 0x1p-6f) + (0x1p-130f * cmax + 0x1p-140f * __builtin_fmaxf(1.f, a2));
  if (bad || !(A + B + Q + __builtin_fabsf(k) < 0x1p120f) || !(cmax < 0x1p100f)) E = __builtin_inff();
  return E;
}

// ---- launch 2: the scan ----
template <class T, int G>
__global__ __launch_bounds__(WAVE) void code_search_1x16_xtx_scan_kernel(X16XtxArgs a) {
  __shared__ float hm[G][G];
  __shared__ float us[kX16Cols][G + 1];  // u of the column (odd stride: a lane reads its own row)
  __shared__ float c_base[kX16Cols], c_two_s[kX16Cols], c_ss[kX16Cols];
  __shared__ float c_thr[kX16Cols];      // the largest score of a full list, +Inf before
  __shared__ uint32_t c_flat[kX16Cols];  // b * 65536
  __shared__ uint64_t lst[kX16MaxBeam][kX16Cols];
  __shared__ uint8_t cnt[kX16Cols], wp[kX16Cols];  // keys held; the slot of the largest key of a full list
  const int l = threadIdx.x, col = l & 31, h = l >> 5;
  const int P = a.positions_in, beam = a.beam;
  const long col0 = (long)blockIdx.x * kX16Cols;
  if (beam > kX16MaxBeam || beam < 1) return;  // (the launcher checked; a guard for the LDS arrays, wave-uniform)

  float cmax = 0.f, qmax = 0.f;
#pragma unroll
  for (int i = 0; i < kX16MaxBlocks / WAVE; ++i) {
    cmax = __builtin_fmaxf(cmax, x16_mag(a.maxima[l + WAVE * i]));
    qmax = __builtin_fmaxf(qmax, x16_mag(a.maxima[kX16MaxBlocks + l + WAVE * i]));
  }
  cmax = x16_wave_max(cmax);
  qmax = x16_wave_max(qmax);
  for (int idx = l; idx < G * G; idx += WAVE) hm[idx / G][idx % G] = a.h[idx];
  __syncthreads();

  // ---- the columns: u and base of the definition, exactly ----
#pragma unroll 1
  for (int c = l; c < kX16Cols; c += WAVE) {
    const long n = col0 + c;
    float u[G], base = 0.f, two_s = 0.f, ss = 0.f;
    uint32_t flat = 0;
#pragma unroll
    for (int f = 0; f < G; ++f) u[f] = 0.f;
    if (n < a.columns) {
      const long o = n / P;
      const int b = (int)(n - o * P);
      const float s = a.scales ? T::to_float(a.scales[o]) : 1.0f;
      two_s = kxb_mul(2.0f, s);
      ss = kxb_mul(s, s);
      const uint32_t p = (uint16_t)a.codes_in[(size_t)b * a.out + o];
      float cp[G];
      x16_entry<T, G>(a.codebook, p, cp);
      const float* tp = a.t + (size_t)b * (size_t)a.t_pos_stride + (size_t)o * (size_t)a.t_row_stride;
      float w[G];
#pragma unroll
      for (int f = 0; f < G; ++f) w[f] = kxb_mul(s, cp[f]);
#pragma unroll
      for (int e = 0; e < G; ++e) {
        float acc = kxb_mul(w[0], hm[0][e]);
#pragma unroll
        for (int f = 1; f < G; ++f) acc = acc + kxb_mul(w[f], hm[f][e]);
        u[e] = tp[e] + acc;
      }
      float d = kxb_mul(cp[0], u[0]);
#pragma unroll
      for (int f = 1; f < G; ++f) d = d + kxb_mul(cp[f], u[f]);
      base = (a.loss[(size_t)b * a.out + o] + kxb_mul(two_s, d)) - kxb_mul(ss, a.q[p]);
      flat = (uint32_t)b << 16;
    }
#pragma unroll
    for (int f = 0; f < G; ++f) us[c][f] = u[f];
    c_base[c] = base;
    c_two_s[c] = two_s;
    c_ss[c] = ss;
    c_flat[c] = flat;
    c_thr[c] = __builtin_inff();
    cnt[c] = 0;
    wp[c] = 0;
  }
  __syncthreads();

  // ---- B fragments (the split of the scaled u), the factors of A~ and the bound, per tile ----
  u32x4 bhi[kX16Tiles], blo[kX16Tiles];  // g = 8: bhi is the lane's ONE fragment (hi in lanes 0-31, lo in lanes 32-63); blo unused
  float kk[kX16Tiles], ssr[kX16Tiles], baser[kX16Tiles], bound[kX16Tiles], thr_e[kX16Tiles];
  bool valid[kX16Tiles];
#pragma unroll
  for (int t = 0; t < kX16Tiles; ++t) {
    const int c = t * 32 + col;
    valid[t] = col0 + c < a.columns;
    float r[G];
    bool bad = false;
    float mx = 0.f;
#pragma unroll
    for (int e = 0; e < G; ++e) {
      r[e] = us[c][e];
      const float ax = __builtin_fabsf(r[e]);
      bad = bad || !(ax < __builtin_inff());  // Inf or NaN
      mx = __builtin_fmaxf(mx, ax);
    }
    // max|u| = m * 2^e, m in [1, 2); the exponent is clamped from below only (code_search.hip has the same scaling)
    int e2 = (int)((__float_as_uint(mx) >> 23) & 0xffu) - 127;
    if (bad || mx == 0.f) e2 = 0;
    e2 = e2 < -100 ? -100 : e2;
    const float up = __uint_as_float((uint32_t)(127 + 10 - e2) << 23);  // u' = u * 2^(10 - e)
    const float two_s = c_two_s[c];
    kk[t] = two_s * -__uint_as_float((uint32_t)(127 + e2 - 10) << 23);   // A~ = x - 2s * 2^(e - 10) * <u', C>
    ssr[t] = c_ss[c];
    baser[t] = c_base[c];
    const float ub = mx == 0.f ? 0.f : __uint_as_float((uint32_t)(128 + e2) << 23);  // 2^(e + 1); e = 127 gives +Inf
    bound[t] = x16_bound<T, G>(two_s, ub, cmax, baser[t], ssr[t], qmax, kk[t], bad);
    thr_e[t] = __builtin_inff();
    uint32_t hi[G / 2], lo[G / 2];
#pragma unroll
    for (int p = 0; p < G / 2; ++p) {
      uint32_t hw[2], lw[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float x = bad ? 0.f : r[2 * p + q] * up;
        const uint16_t hb = T::from_float(x);
        const uint16_t lb = T::from_float(x - T::to_float(hb));
        hw[q] = hb;
        lw[q] = lb;
      }
      hi[p] = hw[0] | (hw[1] << 16);
      lo[p] = lw[0] | (lw[1] << 16);
    }
    if constexpr (G == 8) {
      bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{lo[0], lo[1], lo[2], lo[3]};
      blo[t] = bhi[t];
    } else {
      bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{hi[4], hi[5], hi[6], hi[7]};
      blo[t] = h == 0 ? u32x4{lo[0], lo[1], lo[2], lo[3]} : u32x4{lo[4], lo[5], lo[6], lo[7]};
    }
  }

  // ---- the scan of this wave's split of the codebook ----
  const int tiles = kX16CodeTiles / a.splits;
  const int tile0 = (int)blockIdx.y * tiles;
  // lane's A piece of codeword tile ct: row col; g = 8: its 16 bytes, g = 16: half h of its 32 bytes
  const u32x4* cb = reinterpret_cast<const u32x4*>(a.codebook) + (G == 8 ? col : 2 * col + h);
  // the lane's 16 rows of a tile: (reg & 3) + 8 * (reg >> 2) + 4 * h  ->  four float4 of q at 8 * j + 4 * h
  const float4* qr = reinterpret_cast<const float4*>(a.q) + h;
  auto load_a = [&](int ct) { return cb[(size_t)ct * (32 * G / 8)]; };
  u32x4 a_next = load_a(tile0);
  float4 q_next[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q_next[j] = qr[(size_t)tile0 * 8 + 2 * j];
  for (int i = 0; i < tiles; ++i) {
    const int ct = tile0 + i;
    const u32x4 a_cur = a_next;
    float qv[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qv[4 * j] = q_next[j].x;
      qv[4 * j + 1] = q_next[j].y;
      qv[4 * j + 2] = q_next[j].z;
      qv[4 * j + 3] = q_next[j].w;
    }
    const int nx = i + 1 < tiles ? ct + 1 : ct;  // (the last iteration repeats its own addresses)
    a_next = load_a(nx);
#pragma unroll
    for (int j = 0; j < 4; ++j) q_next[j] = qr[(size_t)nx * 8 + 2 * j];
    uint64_t masks = 0;  // 16 bits per tile: the lane's candidates to refine
#pragma unroll
    for (int t = 0; t < kX16Tiles; ++t) {
      x16_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      acc = x16_mfma<T>(a_cur, bhi[t], acc);
      if constexpr (G == 16) acc = x16_mfma<T>(a_cur, blo[t], acc);
      float sc[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) sc[v] = __builtin_fmaf(acc[v], kk[t], __builtin_fmaf(qv[v], ssr[t], baser[t]));
      // fminf drops a NaN operand; a column whose A~ can be NaN has an infinite bound, and nothing is above +Inf or NaN
      float tm = __builtin_fminf(sc[0], sc[1]);
#pragma unroll
      for (int v = 2; v < 16; v += 2) tm = __builtin_fminf(__builtin_fminf(tm, sc[v]), sc[v + 1]);
      const bool pass = valid[t] && !(tm > thr_e[t]);
      if (__builtin_amdgcn_ballot_w64(pass) != 0) {  // wave-uniform branch
        uint32_t m = 0;
#pragma unroll
        for (int v = 0; v < 16; ++v) m |= !(sc[v] > thr_e[t]) ? (1u << v) : 0u;
        masks |= (uint64_t)(pass ? m : 0u) << (16 * t);
      }
    }
    if (__builtin_amdgcn_ballot_w64(masks != 0) == 0) continue;

    // ---- refine: the definition, operation for operation, and the column's list ----
#pragma unroll 1
    for (int t = 0; t < kX16Tiles; ++t) {
      uint32_t m = (uint32_t)(masks >> (16 * t)) & 0xffffu;
      const int c = t * 32 + col;
      while (__builtin_amdgcn_ballot_w64(m != 0) != 0) {  // at most 16 rounds: a bit leaves every round
        const bool act = m != 0;
        const int v = act ? __builtin_ctz(m) : 0;
        m &= m - 1;
        uint64_t key = kX16Empty;
        if (act) {
          const uint32_t code = (uint32_t)ct * 32 + (uint32_t)((v & 3) + 8 * (v >> 2) + 4 * h);
          float cw[G];
          x16_entry<T, G>(a.codebook, code, cw);
          float d = kxb_mul(us[c][0], cw[0]);
#pragma unroll
          for (int f = 1; f < G; ++f) d = d + kxb_mul(us[c][f], cw[f]);
          const float S = x16_plus_zero((c_base[c] - kxb_mul(c_two_s[c], d)) + kxb_mul(c_ss[c], a.q[code]));
          if (S == S) key = ((uint64_t)kxb_ordered(S) << 32) | (c_flat[c] | code);
        }
        // lanes l and l + 32 share a column: one half at a time
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          if (h == hh && key != kX16Empty) {
            int n = cnt[c];
            n = n < beam ? n : beam;
            bool changed = false;
            if (n < beam) {
              lst[n][c] = key;
              cnt[c] = (uint8_t)(n + 1);
              changed = n + 1 == beam;
            } else {
              const int w = wp[c] & (kX16MaxBeam - 1);
              if (key < lst[w][c]) {
                lst[w][c] = key;
                changed = true;
              }
            }
            if (changed) {  // the list is full: its largest key and that key's score
              uint64_t mk = lst[0][c];
              int mi = 0;
              for (int j = 1; j < beam; ++j) {
                const uint64_t kj = lst[j][c];
                if (kj > mk) {
                  mk = kj;
                  mi = j;
                }
              }
              wp[c] = (uint8_t)mi;
              c_thr[c] = kxb_unordered((uint32_t)(mk >> 32));
            }
          }
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kX16Tiles; ++t) thr_e[t] = c_thr[t * 32 + col] + bound[t];
  }

  // ---- the lists of this split: held keys, then empty ones ----
  __syncthreads();
  for (int c = l; c < kX16Cols; c += WAVE) {
    const long n = col0 + c;
    if (n >= a.columns) continue;
    uint64_t* dst = a.keys + ((size_t)blockIdx.y * (size_t)a.columns + (size_t)n) * (size_t)beam;
    const int held = cnt[c] < beam ? cnt[c] : beam;
    for (int j = 0; j < beam; ++j) dst[j] = j < held ? lst[j][c] : kX16Empty;
  }
}

// ---- launch 3: the merge of a row's lists, and the outputs ----
template <class T, int G>
__global__ __launch_bounds__(WAVE) void code_search_1x16_xtx_merge_kernel(X16XtxArgs a) {
  __shared__ float hm[G][G];
  __shared__ float dwb[kX16MaxBeam][G];
  __shared__ uint32_t win[kX16MaxBeam];   // the flat index b * 65536 + s' of rank i
  __shared__ float wins[kX16MaxBeam];     // its score
  const int lane = threadIdx.x;
  const int P = a.positions_in, beam = a.beam;
  const int e_own = lane & (G - 1), r_own = lane / G;
  if (beam > kX16MaxBeam || beam < 1) return;
  for (int idx = lane; idx < G * G; idx += WAVE) hm[idx / G][idx % G] = a.h[idx];
  const int per_split = P * beam;  // a row's keys of one split are contiguous
  const int total = a.splits * per_split;

  for (long o = blockIdx.x; o < a.out; o += gridDim.x) {
    const float s = a.scales ? T::to_float(a.scales[o]) : 1.0f;
    // ---- the beam smallest keys in order: keys are unique, so rank i is the smallest key above rank i - 1 ----
    uint64_t last = 0;
    uint32_t taken[kX16MaxBeam];
#pragma unroll
    for (int i = 0; i < kX16MaxBeam; ++i) {
      taken[i] = 0xffffffffu;
      if (i < beam) {  // wave-uniform
        uint64_t best = kX16Empty;
        for (int j = lane; j < total; j += WAVE) {
          const int sp = j / per_split, r = j - sp * per_split;
          const uint64_t k = a.keys[((size_t)sp * (size_t)a.columns + (size_t)o * P) * (size_t)beam + r];
          if ((i == 0 || k > last) && k < best) best = k;
        }
        best = kxb_wave_min(best);
        uint32_t flat;
        float score;
        if (best != kX16Empty) {
          flat = (uint32_t)best;
          score = kxb_unordered((uint32_t)(best >> 32));
          last = best;
        } else {  // fewer non-NaN scores than beam_size: position 0, the smallest code not yet present
          flat = 0;
          for (int round = 0; round < kX16MaxBeam; ++round) {
            bool present = false;
#pragma unroll
            for (int j = 0; j < kX16MaxBeam; ++j) present = present || (j < i && taken[j] == flat);
            if (!present) break;
            ++flat;
          }
          score = __uint_as_float(0x7fc00000u);
          last = kX16Empty;  // nothing is above it: the ranks after this one are filled too
        }
        uint32_t from = flat >> 16;
        from = from < (uint32_t)P ? from : 0u;  // (always in range for keys that were taken; a guard, not a rule)
        flat = (from << 16) | (flat & 0xffffu);
        taken[i] = flat;
        if (lane == 0) {
          win[i] = flat;
          wins[i] = score;
        }
      }
    }
    __syncthreads();
    // ---- rank i from (b, s'): dw = s C[s'] - s C[p], t = t[b] - dw H ----
    for (int i = r_own; i < beam; i += WAVE / G) {
      const uint32_t flat = win[i];
      const uint32_t from = flat >> 16, code = flat & 0xffffu;
      const uint32_t p = (uint16_t)a.codes_in[(size_t)from * a.out + o];
      const float dw = kxb_mul(s, T::to_float(a.codebook[(size_t)code * G + e_own])) - kxb_mul(s, T::to_float(a.codebook[(size_t)p * G + e_own]));
      dwb[i][e_own] = dw;
      a.delta[((size_t)i * a.out + o) * G + e_own] = dw;
    }
    __syncthreads();
    if (a.t_out) {
      for (int i = r_own; i < beam; i += WAVE / G) {
        const uint32_t from = win[i] >> 16;
        float acc = kxb_mul(dwb[i][0], hm[0][e_own]);
        for (int f = 1; f < G; ++f) acc = acc + kxb_mul(dwb[i][f], hm[f][e_own]);
        const float tv = a.t[(size_t)from * (size_t)a.t_pos_stride + (size_t)o * (size_t)a.t_row_stride + e_own];
        a.t_out[((size_t)i * a.out + o) * G + e_own] = tv - acc;
      }
    }
    if (lane < beam) {
      const uint32_t flat = win[lane];
      a.codes_out[(size_t)lane * a.out + o] = (int16_t)(uint16_t)(flat & 0xffffu);  // the 16 bits as the checkpoint stores them
      a.source[(size_t)lane * a.out + o] = (uint8_t)(flat >> 16);
      a.loss_out[(size_t)lane * a.out + o] = wins[lane];
    }
    __syncthreads();
  }
}

static bool x16_scheme_ok(int g, int beam_size, int positions_in) {
  return (g == 8 || g == 16) && beam_size >= 1 && beam_size <= kX16MaxBeam && positions_in >= 1 && positions_in <= kX16MaxBeam;
}

// the splits of the codebook: a power of two, doubled until column blocks x splits waves fill the device
static int x16_splits(long columns) {
  const long blocks = (columns + kX16Cols - 1) / kX16Cols;
  int splits = 1;
  while (splits < kX16MaxSplits && blocks * splits < kX16WantWaves) splits *= 2;
  return splits;
}

static size_t x16_maxima_bytes() { return 2 * kX16MaxBlocks * sizeof(float); }

static size_t x16_workspace(int out_features, int beam_size, int positions_in) {
  const long columns = (long)out_features * positions_in;
  return x16_maxima_bytes() + (size_t)x16_splits(columns) * (size_t)columns * (size_t)beam_size * sizeof(uint64_t);
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_code_search_1x16_xtx_supported(int out_features, int in_group_size, int beam_size, int positions_in) {
  return out_features >= 1 && x16_scheme_ok(in_group_size, beam_size, positions_in) ? 1 : 0;
}

extern "C" size_t aqlm_hip_code_search_1x16_xtx_workspace_bytes(int out_features, int in_group_size, int beam_size, int positions_in) {
  if (out_features < 1 || !x16_scheme_ok(in_group_size, beam_size, positions_in)) return 0;
  return x16_workspace(out_features, beam_size, positions_in);
}

extern "C" int aqlm_hip_code_search_1x16_xtx(const void* t, long t_position_stride, long t_row_stride, const void* loss, const void* codes_in,
                                             const void* h, const void* q, const void* codebook, int dtype, const void* scales,
                                             int out_features, int in_group_size, int beam_size, int positions_in, void* loss_out,
                                             void* codes_out, void* source_out, void* delta_out, void* t_out, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_code_search_1x16_xtx";
  if (int e = check_not_null(who, t && loss && codes_in && h && q && codebook && loss_out && codes_out && source_out && delta_out && workspace))
    return e;
  if (int e = check_aligned(who, "t / loss / codes_in / H / q / scales / codebook / loss_out / codes_out / delta / t_out / workspace",
                            aligned4(t) && aligned4(loss) && aligned2(codes_in) && aligned4(h) && aligned16(q) && aligned2(scales) &&
                                aligned16(codebook) && aligned4(loss_out) && aligned2(codes_out) && aligned4(delta_out) && aligned4(t_out) &&
                                aligned16(workspace)))
    return e;
  if (out_features < 1 || in_group_size < 1) {
    set_last_error("%s: bad sizes (out=%d g=%d)", who, out_features, in_group_size);
    return AQLM_HIP_E_INVALID;
  }
  if (t_row_stride < in_group_size || (positions_in > 1 && t_position_stride < in_group_size)) {
    set_last_error("%s: bad sizes (t row stride %ld or position stride %ld below the group size %d)", who, t_row_stride, t_position_stride,
                   in_group_size);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!x16_scheme_ok(in_group_size, beam_size, positions_in)) {
    set_last_error("%s: shape outside the kernel (groups of 8 or 16, beam_size and positions_in 1 to %d; got g=%d beam_size=%d positions_in=%d)",
                   who, kX16MaxBeam, in_group_size, beam_size, positions_in);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t need = x16_workspace(out_features, beam_size, positions_in);
  if (workspace_bytes < need) {
    set_last_error("%s: a workspace of %zu bytes where %zu bytes are needed", who, workspace_bytes, need);
    return AQLM_HIP_E_INVALID;
  }
  X16XtxArgs a{};
  a.t = (const float*)t;
  a.loss = (const float*)loss;
  a.codes_in = (const int16_t*)codes_in;
  a.h = (const float*)h;
  a.q = (const float*)q;
  a.codebook = (const uint16_t*)codebook;
  a.scales = (const uint16_t*)scales;
  a.loss_out = (float*)loss_out;
  a.codes_out = (int16_t*)codes_out;
  a.source = (uint8_t*)source_out;
  a.delta = (float*)delta_out;
  a.t_out = (float*)t_out;
  a.maxima = (float*)workspace;
  a.keys = (uint64_t*)((char*)workspace + x16_maxima_bytes());
  a.t_pos_stride = positions_in > 1 ? t_position_stride : 0;
  a.t_row_stride = t_row_stride;
  a.columns = (long)out_features * positions_in;
  a.out = out_features;
  a.beam = beam_size;
  a.positions_in = positions_in;
  a.splits = x16_splits(a.columns);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned col_blocks = (unsigned)((a.columns + kX16Cols - 1) / kX16Cols);
  const unsigned rows = (unsigned)out_features < kX16MergeBlocks ? (unsigned)out_features : kX16MergeBlocks;
  return dispatch_dtype_group(dtype, in_group_size, [&](auto ty, auto gs) {
    using T = decltype(ty);
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((code_search_1x16_xtx_maxima_kernel<T, G>), dim3(kX16MaxBlocks), dim3(256), 0, stream, a.codebook, a.q, a.maxima);
    if (int e = check_hip(hipGetLastError(), "code_search_1x16_xtx maxima launch")) return e;
    hipLaunchKernelGGL((code_search_1x16_xtx_scan_kernel<T, G>), dim3(col_blocks, (unsigned)a.splits), dim3(WAVE), 0, stream, a);
    if (int e = check_hip(hipGetLastError(), "code_search_1x16_xtx scan launch")) return e;
    hipLaunchKernelGGL((code_search_1x16_xtx_merge_kernel<T, G>), dim3(rows), dim3(WAVE), 0, stream, a);
    return check_hip(hipGetLastError(), "code_search_1x16_xtx merge launch");
  });
}

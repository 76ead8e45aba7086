// Input gradient of the dense K x 8 layers (1x8 g8, 2x8 g8, 4x8 g16, 8x8 g32, ...): the TRANSPOSED product on the MFMA pipe, gfx950.
// gemm_transposed.h has the tile, the layout of the W and gy images with its bank argument, the slices and the numerics, and says why
// the shares, the consumer and the epilogue below are written out here as in gemm_1x16_transposed.hip; this file builds the W image
// of a step from codebooks in LDS.
//
// Wq is the scaled storage weight of DESIGN.md section 4.7 -- per weight an fp32 zero plus the selected entry of every codebook in
// codebook order, times the row's scale, one round-to-nearest-even -- i.e. the bits aqlm_hip_dequant_kx8 writes.  Here W never
// reaches global memory:
//   * all K codebooks (K x 256 x g x 2 bytes) are copied to LDS once per block;
//   * for a cell of the image a thread reads the cell's K code bytes (contiguous in the checkpoint layout [out][in / g][K]), gathers
//     the K pieces from the LDS codebooks, adds them in fp32 in codebook order, multiplies by scales[o], rounds once and stores 16
//     bytes;
//   * gy is masked where it is loaded: the piece that holds row `out` is read element by element, so out % 8 may be anything;
//   * two image buffers, one barrier per step: the code bytes, scales and gy of step s + 1 are requested from global memory before
//     the MFMAs of step s are issued and become the image of s + 1 after them.
//
// Row tiles.  The cost of an image (2 cells per thread: K gathers and 8 K additions each) is paid once per tile, the MFMAs once
// per 16 batch rows, so the tile is as tall as the call allows: TP = 16 for up to 16 rows, 64 up to 64 and where 128-row tiles
// would leave CUs idle, else 128.  LDS per block = codebooks + 2 x 8 KiB of W image + 2 x TP x 64 bytes of gy image:
//                 codebooks    TP 16     TP 64     TP 128
//   1x8 g8          4 KiB      22 KiB    28 KiB    36 KiB
//   2x8 g8          8 KiB      26 KiB    32 KiB    40 KiB
//   4x8 g16        32 KiB      50 KiB    56 KiB    64 KiB
//   8x8 g32       128 KiB     146 KiB   152 KiB   160 KiB   (dynamic-LDS attribute above 64 KiB; the launch declines above 160 KiB)
#include "gemm_transposed.h"

namespace aqlm {
namespace {

constexpr size_t kTMaxLds = 160u * 1024u;

struct KtArgs {
  const uint8_t* codes;      // [M][in_groups][K]
  const uint8_t* codebooks;  // [K][256][G] storage type
  const uint16_t* scales;    // [M]
  // TArgs, spelled out: K keeps the place it had among the arguments, and with it every kernel the argument loads it had
  const uint16_t* gy;
  uint16_t* gx;
  float* partial;
  long gys, gxs;
  int rows, M, N, K, in_groups, nsteps, steps_per_slice, splits;
};

// KC > 0: that many codebooks, the codes of a cell fetched as one aligned word; KC == 0: a.K (1..8) codebooks, byte loads
template <class T, int KC, int G, int NPT>
__global__ __launch_bounds__(kTThreads) void gemm_kx8_transposed_kernel(const KtArgs a) {
  constexpr int TP = 16 * NPT;                                  // batch rows of a tile
  constexpr int P = G / 8;                                      // 16-byte pieces per codebook entry
  constexpr int ACH = (TP * 4 + kTThreads - 1) / kTThreads;     // 16-byte pieces of the gy image per thread
  constexpr uint32_t A_BYTES = TP * 64u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = KC > 0 ? KC : a.K;
  const uint32_t W_BASE = (uint32_t)K * 256u * G * 2u, A_BASE = W_BASE + 2u * kTWBytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col0 = blockIdx.x * kTCols, row0 = blockIdx.y * TP, slice = blockIdx.z;
  const int s0 = slice * a.steps_per_slice, s1 = min(s0 + a.steps_per_slice, a.nsteps);  // (uniform; s0 >= s1: an empty slice)

  {  // the codebooks, once
    const u32x4* src = reinterpret_cast<const u32x4*>(a.codebooks);
    u32x4* dst = reinterpret_cast<u32x4*>(smem);
    for (int q = tid; q < K * 256 * P; q += kTThreads) dst[q] = src[q];
  }

  // ---- this thread's share of the W image: piece ch of rows wr and wr + 16 -------------------------------------------------------
  const int ch = tid & 15, wr = tid >> 4;
  const bool col_ok = col0 + ch * 8 < a.N;
  int jg = col0 / G + (ch * 8) / G;  // the group that covers the piece
  jg = jg < a.in_groups ? jg : a.in_groups - 1;
  const uint32_t pp = (uint32_t)(ch & (P - 1));  // ... and the piece's place in its entries
  const uint32_t wdst[2] = {timg(wr, ch), timg(wr + 16, ch)};
  const bool swap_halves = (wr & 8) != 0;  // (rows wr and wr + 16 share bit 3)
  // ---- ... and of the gy image: piece ac (8 output rows) of batch row ab ---------------------------------------------------------
  int ab[ACH], ac[ACH];
  bool aok[ACH];  // false: a row past `rows`, or a thread without a piece
  const uint16_t* gsrc[ACH];
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int j = tid + i * kTThreads;
    ab[i] = j >> 2;
    ac[i] = j & 3;
    aok[i] = j < TP * 4 && row0 + ab[i] < a.rows;
    gsrc[i] = a.gy + (size_t)(aok[i] ? row0 + ab[i] : 0) * a.gys;
  }

  struct Cell {
    u32x2 code;  // the K code bytes, codebook 0 lowest
    uint32_t scale;
  };
  auto load_cells = [&](int q, Cell (&c)[2]) {  // (a step past the slice: clamped copies, never used)
    q = q < a.nsteps ? q : a.nsteps - 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int r = q * kTRows + wr + 16 * h;
      r = r < a.M ? r : a.M - 1;
      const uint8_t* p = a.codes + ((size_t)r * a.in_groups + jg) * K;
      u32x2 v{0u, 0u};
      if constexpr (KC == 1) v.x = *p;
      else if constexpr (KC == 2) v.x = *reinterpret_cast<const uint16_t*>(p);
      else if constexpr (KC == 4) v.x = *reinterpret_cast<const uint32_t*>(p);
      else if constexpr (KC == 8) v = *reinterpret_cast<const u32x2*>(p);
      else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < K) v[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
      }
      c[h].code = v;
      c[h].scale = a.scales[r];
    }
  };
  auto load_gy = [&](int q, u32x4 (&g)[ACH]) {
    q = q < a.nsteps ? q : a.nsteps - 1;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int o = q * kTRows + ac[i] * 8;
      u32x4 v{0u, 0u, 0u, 0u};
      if (aok[i]) {
        if (o + 8 <= a.M) {
          v = *reinterpret_cast<const u32x4*>(gsrc[i] + o);
        } else {  // the piece that holds row `out`: element by element, nothing is read past the row
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (o + e < a.M) v[e >> 1] |= (uint32_t)gsrc[i][o + e] << ((e & 1) * 16);
        }
      }
      g[i] = v;
    }
  };
  // step q -> LDS: the image holds the bits aqlm_hip_dequant_kx8 would have written
  auto put = [&](int q, int buf, const Cell (&c)[2], const u32x4 (&g)[ACH]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < K) {
          const uint32_t code = (c[h].code[k >> 2] >> ((k & 3) * 8)) & 0xffu;
          const u32x4 e = *reinterpret_cast<const u32x4*>(smem + (((uint32_t)k * 256u + code) * P + pp) * 16u);
          f[0] += T::lo(e.x); f[1] += T::hi(e.x);
          f[2] += T::lo(e.y); f[3] += T::hi(e.y);
          f[4] += T::lo(e.z); f[5] += T::hi(e.z);
          f[6] += T::lo(e.w); f[7] += T::hi(e.w);
        }
      }
      const float scale = T::to_float((uint16_t)c[h].scale);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] *= scale;
        asm volatile("" : "+v"(f[e]));  // the product exists in fp32 before the one rounding, as in dequant_kernel (no fused mixed-precision form)
      }
      const bool ok = col_ok && q * kTRows + wr + 16 * h < a.M;  // past the matrix: zeros, whatever the codes held
      const uint32_t w0 = ok ? pack2<T>(f[0], f[1]) : 0u, w1 = ok ? pack2<T>(f[2], f[3]) : 0u;
      const uint32_t w2 = ok ? pack2<T>(f[4], f[5]) : 0u, w3 = ok ? pack2<T>(f[6], f[7]) : 0u;
      *reinterpret_cast<u32x4*>(smem + W_BASE + buf * kTWBytes + wdst[h]) = swap_halves ? u32x4{w2, w3, w0, w1} : u32x4{w0, w1, w2, w3};
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i)
      if (tid + i * kTThreads < TP * 4) *reinterpret_cast<u32x4*>(smem + A_BASE + buf * A_BYTES + tgy(ab[i], ac[i])) = g[i];
  };

  // ---- consumer addresses: wave w owns columns 32 w .. 32 w + 31; row i of its MFMA block nn is column 8 (i >> 2) + 4 nn + (i & 3) --
  const int kg = lane >> 4, li = lane & 15;
  uint32_t wsrc[2][2];  // [block][rows 8 kg + 4 h ..]: lane 4 q + p of a 16-lane group gives row q, half nn of piece 4 w + p
#pragma unroll
  for (int nn = 0; nn < 2; ++nn)
#pragma unroll
    for (int h = 0; h < 2; ++h) wsrc[nn][h] = W_BASE + timg(8 * kg + 4 * h + (li >> 2), 4 * wave + (li & 3)) + 8u * (uint32_t)(nn ^ (kg & 1));
  uint32_t asrc[NPT];
#pragma unroll
  for (int t = 0; t < NPT; ++t) asrc[t] = A_BASE + tgy(16 * t + li, kg);

  f32x4 acc[NPT][2];
#pragma unroll
  for (int t = 0; t < NPT; ++t)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) acc[t][nn] = f32x4{0.f, 0.f, 0.f, 0.f};

  Cell c[2];
  u32x4 g[ACH];
  load_cells(s0, c);
  load_gy(s0, g);
  __syncthreads();  // the codebooks are in place
  if (s0 < s1) put(s0, 0, c, g);
  __syncthreads();
  for (int q = s0; q < s1; ++q) {  // (uniform)
    const int buf = (q - s0) & 1;
    load_cells(q + 1, c);  // in flight while the MFMAs run
    load_gy(q + 1, g);
    u32x4 wf[2];
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kTWBytes + wsrc[nn][0]));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kTWBytes + wsrc[nn][1]));
      const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
      wf[nn] = u32x4{l2.x, l2.y, h2.x, h2.y};
    }
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
      const u32x4 gf = *reinterpret_cast<const u32x4*>(smem + buf * A_BYTES + asrc[t]);
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) acc[t][nn] = mfma16<T>(wf[nn], gf, acc[t][nn]);
    }
    if (q + 1 < s1) put(q + 1, buf ^ 1, c, g);
    __syncthreads();
  }

  // ---- epilogue: lane (li, kg) holds columns 8 kg .. 8 kg + 7 of its wave's 32 for batch row 16 t + li --------------------------
  const int cc = col0 + 32 * wave + 8 * kg;
#pragma unroll
  for (int t = 0; t < NPT; ++t) {
    const int b = row0 + 16 * t + li;
    if (b < a.rows && cc < a.N) {  // (N % 8 == 0: the 8 columns are inside or outside as a whole)
      const f32x4 x = acc[t][0], y = acc[t][1];
      if (a.splits == 1) {
        *reinterpret_cast<u32x4*>(a.gx + (size_t)b * a.gxs + cc) = u32x4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
      } else {
        float* dst = a.partial + ((size_t)slice * a.rows + b) * a.N + cc;
        *reinterpret_cast<f32x4*>(dst) = x;
        *reinterpret_cast<f32x4*>(dst + 4) = y;
      }
    }
  }
}

size_t lds_bytes(int K, int G, int tp) { return (size_t)K * 256 * G * 2 + 2 * kTWBytes + 2 * (size_t)tp * 64; }

bool kt_supported(int M, int N, int K, int G) {
  return M >= 1 && N >= 8 && K >= 1 && K <= 8 && (G == 8 || G == 16 || G == 32) && N % G == 0 && N % 8 == 0 && lds_bytes(K, G, 16) <= kTMaxLds;
}

// batch rows of a tile: as tall as the rows allow and the LDS holds; 64 where tiles of 128 would leave CUs without a block
int tile_rows(int rows, int N, int K, int G) {
  const long col_blocks = (N + kTCols - 1) / kTCols;
  int tp = rows <= 16 ? 16 : (rows <= 64 || (long)((rows + 127) / 128) * col_blocks < kTFullGrid ? 64 : 128);
  while (tp > 16 && lds_bytes(K, G, tp) > kTMaxLds) tp = tp == 128 ? 64 : 16;
  return tp;
}

template <class T, int KC, int G, int NPT>
int launch_kt_tile(const KtArgs& a, hipStream_t stream) {
  auto kern = gemm_kx8_transposed_kernel<T, KC, G, NPT>;
  const size_t lds = lds_bytes(a.K, G, 16 * NPT);
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
  const dim3 grid((unsigned)((a.N + kTCols - 1) / kTCols), (unsigned)((a.rows + 16 * NPT - 1) / (16 * NPT)), (unsigned)a.splits);
  hipLaunchKernelGGL(kern, grid, dim3(kTThreads), lds, stream, a);
  return check_hip(hipGetLastError(), "gemm_kx8_transposed launch");
}

template <class T, int KC, int G>
int launch_kt(const KtArgs& a, int tp, hipStream_t stream) {
  if (tp == 16) return launch_kt_tile<T, KC, G, 1>(a, stream);
  if (tp == 64) return launch_kt_tile<T, KC, G, 4>(a, stream);
  return launch_kt_tile<T, KC, G, 8>(a, stream);
}

// the checkpoint schemes get instances with their K fixed (codes aligned to the word a cell reads); everything else the K-runtime one
template <class T>
int launch_kt_scheme(const KtArgs& a, int G, int tp, hipStream_t stream) {
  const bool word = aligned8(a.codes);
  if (G == 8) {
    if (a.K == 1) return launch_kt<T, 1, 8>(a, tp, stream);
    if (a.K == 2 && word) return launch_kt<T, 2, 8>(a, tp, stream);
    return launch_kt<T, 0, 8>(a, tp, stream);
  }
  if (G == 16) return a.K == 4 && word ? launch_kt<T, 4, 16>(a, tp, stream) : launch_kt<T, 0, 16>(a, tp, stream);
  return a.K == 8 && word ? launch_kt<T, 8, 32>(a, tp, stream) : launch_kt<T, 0, 32>(a, tp, stream);
}

}  // namespace
}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_gemm_kx8_transposed_supported(int out_features, int in_features, int num_codebooks, int in_group_size) {
  return kt_supported(out_features, in_features, num_codebooks, in_group_size) ? 1 : 0;
}

// (any number of rows; splits == 0 is sized without the scheme: the most slices any tile of the call gets)
extern "C" size_t aqlm_hip_gemm_kx8_transposed_workspace_bytes(int rows, int out_features, int in_features, int splits) {
  if (rows < 1 || out_features < 1 || in_features < 1 || splits < 0 || splits > kTMaxSplits) return 0;
  if (splits == 0) splits = choose_splits(rows, out_features, in_features, rows <= 16 ? 16 : 64);
  return transposed_workspace_bytes(rows, in_features, splits);
}

extern "C" int aqlm_hip_gemm_kx8_transposed(const void* codes, const void* codebooks, const void* scales, const void* gy, void* gx, int rows,
                                            int out_features, int in_features, int num_codebooks, int in_group_size, long gy_row_stride,
                                            long gx_row_stride, int dtype, int splits, void* workspace, size_t workspace_bytes,
                                            void* stream_) {
  static const char* who = "aqlm_hip_gemm_kx8_transposed";
  if (int e = check_not_null(who, codes && codebooks && scales && gy && gx)) return e;
  if (int e = check_positive(who, rows, out_features, in_features)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (!kt_supported(out_features, in_features, num_codebooks, in_group_size) || !aligned16(codebooks) || !aligned2(scales) ||
      !transposed_call_ok(rows, out_features, in_features, splits, gy, gx, gy_row_stride, gx_row_stride)) {
    set_last_error("%s: outside the transposed kernel (%d rows, out=%d in=%d, %d codebooks, g=%d, splits %d, row strides %ld / %ld; 1..8 "
                   "codebooks of 256, g 8 / 16 / 32, in %% g == 0, in %% 8 == 0, 16-B aligned codebooks and rows)",
                   who, rows, out_features, in_features, num_codebooks, in_group_size, splits, gy_row_stride, gx_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int tp = tile_rows(rows, in_features, num_codebooks, in_group_size);
  if (splits == 0) splits = choose_splits(rows, out_features, in_features, tp);
  if (int e = check_transposed_workspace(who, rows, in_features, splits, workspace, workspace_bytes)) return e;
  const TArgs t = transposed_args(gy, gx, workspace, gy_row_stride, gx_row_stride, rows, out_features, in_features, in_group_size, splits);
  const KtArgs a{(const uint8_t*)codes, (const uint8_t*)codebooks, (const uint16_t*)scales, t.gy, t.gx, t.partial, t.gys, t.gxs,
                 t.rows, t.M, t.N, num_codebooks, t.in_groups, t.nsteps, t.steps_per_slice, t.splits};
  hipStream_t stream = (hipStream_t)stream_;
  const int e = dtype == AQLM_HIP_F16 ? launch_kt_scheme<F16>(a, in_group_size, tp, stream) : launch_kt_scheme<BF16>(a, in_group_size, tp, stream);
  if (e || splits == 1) return e;
  return launch_finalize(dtype, t, stream, "gemm_kx8_transposed finalize launch");
}

// Input gradient of the dense 1x16 layers (one codebook of 65536 entries, g 8 / 16): the TRANSPOSED product on the MFMA pipe, gfx950.
// gemm_transposed.h has the tile, the layout of the W and gy images with its bank argument, the slices and the numerics, and says why
// the shares, the consumer and the epilogue below are written out here as in gemm_kx8_transposed.hip; this file builds the W image
// of a step from codebook vectors gathered from L2.
//
// Wq is the scaled storage weight aqlm_hip_dequant_1x16 writes -- per weight fp32(codebook value) x fp32(scales[o]), held as an fp32
// product and rounded once (dequant.hip explains why the product must not fold into a mixed-precision fma).  The scale is folded
// into W, not into gy, so against code1x16_matmat_dequant_transposed only the order of the fp32 sums over o differs.  W never reaches
// global memory, and the codebook (1 - 2 MiB) never reaches LDS: its vectors are gathered from L2, once per row tile.
//   * Row tiles.  TP is 16, 64 or 256: the gathers of a step (512 per block) are paid once per tile, the MFMAs (TP / 16 x 2 per
//     wave) once per 16 rows, so the tall tile is what amortises the gather pass; it takes TP / 2 accumulator registers per lane.
//   * For a cell of the image a thread fetches the cell's code as the aligned dword that holds it (cut out where it is used: a
//     16-bit load would be extended right behind the load and wait there), gathers the 16-byte piece of the codebook vector (g 16: the
//     half the column selects) and the row's scale (again as its aligned dword), multiplies in fp32, rounds once and stores 16 bytes.
//   * Register pipeline, D steps deep (8 for the tiles of 16 and 64 rows, 4 for 256): the code words of step s are requested in
//     iteration s - 2 D, its gathers, scales and gy in iteration s - D, and all of it goes to LDS at the end of iteration s - 1 (two
//     image buffers, one barrier per step).  The loads are unconditional, from clamped addresses, and nothing touches their values
//     before `put`, where gy is masked too: a select or a conversion next to a load makes the compiler wait for it there, with every
//     younger load (moe_grouped_bwd.hip's header).  The loop is unrolled D times so that every register set has a fixed name.
// LDS per block = 2 x 8 KiB of W image + 2 x TP x 64 bytes of gy image: 18 / 24 / 48 KiB.
#include "gemm_transposed.h"

namespace aqlm {
namespace {

struct XtArgs {
  const uint32_t* codes;     // [M][in_groups] u16, read as the dwords that hold them (M * in_groups is even)
  const uint8_t* codebook;   // [65536][G] storage type
  const uint32_t* scales;    // [M] of the storage type, read as the dwords that hold them (M is even)
  TArgs t;
};

// the bits aqlm_hip_dequant_1x16 writes for two neighbours: the product exists in fp32 before the one rounding
template <class T>
__device__ __forceinline__ uint32_t scaled2(uint32_t e, float scale) {
  float lo = T::lo(e) * scale, hi = T::hi(e) * scale;
  asm volatile("" : "+v"(lo), "+v"(hi));
  return pack2<T>(lo, hi);
}

template <class T, int G, int NPT>
__global__ __launch_bounds__(kTThreads) void gemm_1x16_transposed_kernel(const XtArgs a) {
  constexpr int TP = 16 * NPT;                                  // batch rows of a tile
  constexpr int ACH = (TP * 4 + kTThreads - 1) / kTThreads;     // 16-byte pieces of the gy image per thread
  constexpr uint32_t A_BYTES = TP * 64u, A_BASE = 2u * kTWBytes;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kTWBytes + 2 * A_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col0 = blockIdx.x * kTCols, row0 = blockIdx.y * TP, slice = blockIdx.z;
  const int s0 = slice * a.t.steps_per_slice, s1 = min(s0 + a.t.steps_per_slice, a.t.nsteps);  // (uniform; s0 >= s1: an empty slice)

  // ---- this thread's share of the W image: piece ch of rows wr and wr + 16 -------------------------------------------------------
  const int ch = tid & 15, wr = tid >> 4;
  const bool col_ok = col0 + ch * 8 < a.t.N;
  int cg = G == 8 ? col0 / 8 + ch : col0 / 16 + (ch >> 1);  // the code of a row that covers the piece
  cg = cg < a.t.in_groups ? cg : a.t.in_groups - 1;
  const uint32_t half_off = G == 8 ? 0u : (uint32_t)(ch & 1) * 16u;
  const uint32_t wdst[2] = {timg(wr, ch), timg(wr + 16, ch)};
  const bool swap_halves = (wr & 8) != 0;  // (rows wr and wr + 16 share bit 3)
  const uint32_t scale_shift = (uint32_t)(wr & 1) * 16u;  // (... and bit 0: where the row's scale lies in its dword)
  // ---- ... and of the gy image: piece ac (8 output rows) of batch row ab ---------------------------------------------------------
  int ab[ACH], ac[ACH];
  bool aok[ACH];  // false: a row past `rows`, or a thread without a piece
  const uint16_t* gsrc[ACH];  // (those without a row: row 0's)
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int j = tid + i * kTThreads;
    ab[i] = j >> 2;
    ac[i] = j & 3;
    aok[i] = j < TP * 4 && row0 + ab[i] < a.t.rows;
    gsrc[i] = a.t.gy + (size_t)(aok[i] ? row0 + ab[i] : 0) * a.t.gys;
  }

  // (a step past the last: clamped copies, never used)
  auto w_row = [&](int q, int h) {
    q = q < a.t.nsteps ? q : a.t.nsteps - 1;
    const int r = q * kTRows + wr + 16 * h;
    return r < a.t.M ? r : a.t.M - 1;
  };
  auto load_codes = [&](int q, uint32_t (&c)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) c[h] = a.codes[((size_t)w_row(q, h) * a.t.in_groups + cg) >> 1];
  };
  auto gather = [&](int q, const uint32_t (&c)[2], u32x4 (&w)[2], uint32_t (&sc)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = w_row(q, h);
      const uint32_t code = (c[h] >> ((((uint32_t)r * (uint32_t)a.t.in_groups + (uint32_t)cg) & 1u) * 16u)) & 0xffffu;
      w[h] = *reinterpret_cast<const u32x4*>(a.codebook + (size_t)code * (G * 2) + half_off);
      sc[h] = a.scales[r >> 1];
    }
  };
  auto load_gy = [&](int q, u32x4 (&g)[ACH]) {
    q = q < a.t.nsteps ? q : a.t.nsteps - 1;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      int o = q * kTRows + ac[i] * 8;
      o = o < a.t.M ? o : a.t.M - 8;  // (M % 8 == 0: a piece is inside or outside as a whole)
      g[i] = *reinterpret_cast<const u32x4*>(gsrc[i] + o);
    }
  };
  // step q -> LDS: the image holds the bits aqlm_hip_dequant_1x16 would have written
  auto put = [&](int q, int buf, const u32x4 (&w)[2], const uint32_t (&sc)[2], const u32x4 (&g)[ACH]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float scale = T::to_float((uint16_t)(sc[h] >> scale_shift));  // (a row the clamp moved is masked below)
      const uint32_t ok = col_ok && q * kTRows + wr + 16 * h < a.t.M ? ~0u : 0u;  // past the matrix: zeros, whatever the code held
      const uint32_t w0 = scaled2<T>(w[h].x, scale) & ok, w1 = scaled2<T>(w[h].y, scale) & ok;
      const uint32_t w2 = scaled2<T>(w[h].z, scale) & ok, w3 = scaled2<T>(w[h].w, scale) & ok;
      *reinterpret_cast<u32x4*>(smem + buf * kTWBytes + wdst[h]) = swap_halves ? u32x4{w2, w3, w0, w1} : u32x4{w0, w1, w2, w3};
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if (tid + i * kTThreads < TP * 4) {
        const bool ok = aok[i] && q * kTRows + ac[i] * 8 < a.t.M;
        *reinterpret_cast<u32x4*>(smem + A_BASE + buf * A_BYTES + tgy(ab[i], ac[i])) = ok ? g[i] : u32x4{0u, 0u, 0u, 0u};
      }
    }
  };

  // ---- consumer addresses: wave w owns columns 32 w .. 32 w + 31; row i of its MFMA block nn is column 8 (i >> 2) + 4 nn + (i & 3) --
  const int kg = lane >> 4, li = lane & 15;
  uint32_t wsrc[2][2];  // [block][rows 8 kg + 4 h ..]: lane 4 q + p of a 16-lane group gives row q, half nn of piece 4 w + p
#pragma unroll
  for (int nn = 0; nn < 2; ++nn)
#pragma unroll
    for (int h = 0; h < 2; ++h) wsrc[nn][h] = timg(8 * kg + 4 * h + (li >> 2), 4 * wave + (li & 3)) + 8u * (uint32_t)(nn ^ (kg & 1));
  const uint32_t asrc = A_BASE + tgy(li, kg);  // (batch row 16 t + li: 1024 t bytes further, the XOR sees b mod 16 only)

  f32x4 acc[NPT][2];
#pragma unroll
  for (int t = 0; t < NPT; ++t)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) acc[t][nn] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int D = NPT <= 4 ? 8 : 4;  // (the tall tile: registers for the accumulators, and long steps that cover more latency each)
  static_assert(D % 2 == 0, "the LDS buffer of step s0 + j is j & 1 == (j % D) & 1");
  uint32_t c[D][2], sc[D][2];
  u32x4 w[D][2], g[D][ACH];
#pragma unroll
  for (int j = 0; j < D; ++j) load_codes(s0 + j, c[j]);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    gather(s0 + j, c[j], w[j], sc[j]);
    load_gy(s0 + j, g[j]);
    load_codes(s0 + j + D, c[j]);
  }
  if (s0 < s1) put(s0, 0, w[0], sc[0], g[0]);
  __syncthreads();
  for (int q0 = s0; q0 < s1; q0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int q = q0 + j;
      if (q < s1) {  // (uniform; once false, false for the rest of the round)
        const int buf = j & 1;
        gather(q + D, c[j], w[j], sc[j]);
        load_gy(q + D, g[j]);
        load_codes(q + 2 * D, c[j]);
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
          const u32x4 gf = *reinterpret_cast<const u32x4*>(smem + buf * A_BYTES + asrc + 1024u * t);
#pragma unroll
          for (int nn = 0; nn < 2; ++nn) acc[t][nn] = mfma16<T>(wf[nn], gf, acc[t][nn]);
        }
        if (q + 1 < s1) put(q + 1, buf ^ 1, w[(j + 1) % D], sc[(j + 1) % D], g[(j + 1) % D]);
        __syncthreads();
      }
    }
  }

  // ---- epilogue: lane (li, kg) holds columns 8 kg .. 8 kg + 7 of its wave's 32 for batch row 16 t + li --------------------------
  const int cc = col0 + 32 * wave + 8 * kg;
#pragma unroll
  for (int t = 0; t < NPT; ++t) {
    const int b = row0 + 16 * t + li;
    if (b < a.t.rows && cc < a.t.N) {  // (N % 8 == 0: the 8 columns are inside or outside as a whole)
      const f32x4 x = acc[t][0], y = acc[t][1];
      if (a.t.splits == 1) {
        *reinterpret_cast<u32x4*>(a.t.gx + (size_t)b * a.t.gxs + cc) = u32x4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
      } else {
        float* dst = a.t.partial + ((size_t)slice * a.t.rows + b) * a.t.N + cc;
        *reinterpret_cast<f32x4*>(dst) = x;
        *reinterpret_cast<f32x4*>(dst + 4) = y;
      }
    }
  }
}

// out % 8 == 0: a 16-byte piece of a gy row is inside the row or outside as a whole; an even number of codes: the dword that holds a
// code never leaves them
bool xt_supported(int M, int N, int G) {
  return M >= 8 && N >= 8 && (G == 8 || G == 16) && M % 8 == 0 && N % G == 0 && (((long)M * (N / G)) & 1) == 0;
}

// batch rows of a tile, from the rows and the block count alone: 16 up to 16 rows, 256 where tiles of 256 still give every CU a
// block, else 64
int xt_tile_rows(int rows, int N) {
  const long col_blocks = (N + kTCols - 1) / kTCols;
  if (rows <= 16) return 16;
  return rows > 64 && (long)((rows + 255) / 256) * col_blocks >= kTFullGrid ? 256 : 64;
}

template <class T, int G, int NPT>
int launch_xt_tile(const XtArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.t.N + kTCols - 1) / kTCols), (unsigned)((a.t.rows + 16 * NPT - 1) / (16 * NPT)), (unsigned)a.t.splits);
  hipLaunchKernelGGL((gemm_1x16_transposed_kernel<T, G, NPT>), grid, dim3(kTThreads), 0, stream, a);
  return check_hip(hipGetLastError(), "gemm_1x16_transposed launch");
}

template <class T, int G>
int launch_xt(const XtArgs& a, int tp, hipStream_t stream) {
  if (tp == 16) return launch_xt_tile<T, G, 1>(a, stream);
  if (tp == 64) return launch_xt_tile<T, G, 4>(a, stream);
  return launch_xt_tile<T, G, 16>(a, stream);
}

}  // namespace
}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_gemm_1x16_transposed_supported(int out_features, int in_features, int in_group_size) {
  return xt_supported(out_features, in_features, in_group_size) ? 1 : 0;
}

// (the rows of a call, and splits == 0 sized for the call's own tile)
extern "C" size_t aqlm_hip_gemm_1x16_transposed_workspace_bytes(int rows, int out_features, int in_features, int splits) {
  if (rows < 1 || rows > 65536 || out_features < 1 || in_features < 1 || splits < 0 || splits > kTMaxSplits) return 0;
  if (splits == 0) splits = choose_splits(rows, out_features, in_features, xt_tile_rows(rows, in_features));
  return transposed_workspace_bytes(rows, in_features, splits);
}

extern "C" int aqlm_hip_gemm_1x16_transposed(const void* codes, const void* codebook, const void* scales, const void* gy, void* gx, int rows,
                                             int out_features, int in_features, int in_group_size, long gy_row_stride, long gx_row_stride,
                                             int dtype, int splits, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_gemm_1x16_transposed";
  if (int e = check_not_null(who, codes && codebook && scales && gy && gx)) return e;
  if (int e = check_positive(who, rows, out_features, in_features)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (!xt_supported(out_features, in_features, in_group_size) || !aligned4(codes) || !aligned16(codebook) || !aligned4(scales) ||
      !transposed_call_ok(rows, out_features, in_features, splits, gy, gx, gy_row_stride, gx_row_stride)) {
    set_last_error("%s: outside the transposed kernel (%d rows, out=%d in=%d, g=%d, splits %d, row strides %ld / %ld; g 8 / 16, out %% 8 "
                   "== 0, in %% g == 0, an even number of codes, 4-B aligned codes and scales, 16-B aligned codebook and rows)",
                   who, rows, out_features, in_features, in_group_size, splits, gy_row_stride, gx_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int tp = xt_tile_rows(rows, in_features);
  if (splits == 0) splits = choose_splits(rows, out_features, in_features, tp);
  if (int e = check_transposed_workspace(who, rows, in_features, splits, workspace, workspace_bytes)) return e;
  XtArgs a{};
  a.codes = (const uint32_t*)codes;
  a.codebook = (const uint8_t*)codebook;
  a.scales = (const uint32_t*)scales;
  a.t = transposed_args(gy, gx, workspace, gy_row_stride, gx_row_stride, rows, out_features, in_features, in_group_size, splits);
  hipStream_t stream = (hipStream_t)stream_;
  const int e = dispatch_dtype_group(dtype, in_group_size, [&](auto ty, auto g) { return launch_xt<decltype(ty), decltype(g)::value>(a, tp, stream); });
  if (e || splits == 1) return e;
  return launch_finalize(dtype, a.t, stream, "gemm_1x16_transposed finalize launch");
}

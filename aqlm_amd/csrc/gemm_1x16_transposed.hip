// Input gradient of the dense 1x16 layers (one codebook of 65536 entries, g 8 / 16): the TRANSPOSED product on the MFMA pipe, gfx950.
//
//   gx[b, :] = sum_o gy[b, o] * Wq[o, :]          gy [rows][out], gx [rows][in], fp16 / bf16
//
// Wq is the scaled storage weight aqlm_hip_dequant_1x16 writes -- per weight fp32(codebook value) x fp32(scales[o]), held as an fp32
// product and rounded once (dequant.hip explains why the product must not fold into a mixed-precision fma).  The scale is folded
// into W, not into gy, so against code1x16_matmat_dequant_transposed only the order of the fp32 sums over o differs.  W never reaches
// global memory, and the codebook (1 - 2 MiB) never reaches LDS: its vectors are gathered from L2, once per row tile.
//   * Work split.  A block of 4 waves owns a tile of TP batch rows x 128 columns of gx and walks the output rows in steps of 32, the
//     k of one v_mfma_f32_16x16x32.  TP is 16, 64 or 256: the gathers of a step (512 per block) are paid once per tile, the MFMAs
//     (TP / 16 x 2 per wave) once per 16 rows, so the tall tile is what amortises the gather pass; it takes TP / 2 accumulator
//     registers per lane.
//   * The W image of a step is [32 rows][128 columns] in LDS.  A thread owns two (row, 16-byte piece) cells: piece ch = tid & 15 of
//     rows wr = tid >> 4 and wr + 16.  It fetches the cell's code as the aligned dword that holds it (cut out where it is used: a
//     16-bit load would be extended right behind the load and wait there), gathers the 16-byte piece of the codebook vector (g 16: the
//     half the column selects) and the row's scale (again as its aligned dword), multiplies in fp32, rounds once and stores 16 bytes.
//   * Register pipeline, D steps deep (8 for the tiles of 16 and 64 rows, 4 for 256): the code words of step s are requested in
//     iteration s - 2 D, its gathers, scales and gy in iteration s - D, and all of it goes to LDS at the end of iteration s - 1 (two
//     image buffers, one barrier per step).  The loads are unconditional, from clamped addresses, and nothing touches their values
//     before `put`: a select or a conversion next to a load makes the compiler wait for it there, with every younger load
//     (moe_grouped_bwd.hip's header).  The loop is unrolled D times so that every register set has a fixed name.
//   * Transposed reads.  The product sums over the image's ROWS, so the waves read it column-major with ds_read_b64_tr_b16 (two reads
//     make the 8 k values of one MFMA operand).  Rows are 256 bytes; piece ch of row r lies at 16-byte slot ch ^ ((r & 3) << 2), and
//     rows with bit 3 set hold the two 8-byte halves of every piece exchanged.  The addresses of one read: lane (kg = lane >> 4,
//     li = lane & 15) of wave w asks for row 8 kg + 4 h + (li >> 2), piece 4 w + (li & 3), logical half nn.  A 32-lane half is
//     kg in {2 k, 2 k + 1}: rows r0 .. r0 + 3 and r0 + 8 .. r0 + 11 with r0 a multiple of 4.  Within one kg the 16 lanes meet slots
//     (4 w + p) ^ (q << 2), q = li >> 2, p = li & 3 -- the XOR moves bits 2..3 of the slot, p its bits 0..1: 16 distinct 16-byte slots,
//     which are the whole 256-byte bank row.  The two kg differ in row bit 3, so they read the SAME slots but opposite physical halves
//     (8 (nn ^ (kg & 1))): 32 distinct 8-byte slots, no bank shared.  An image write of 16 lanes (one wr, 16 ch) covers one whole row.
//     (Argued from these addresses, here and for the gy image; no counter run has measured it.)
//   * gy of a step ([TP][32]) is staged beside the image: 64-byte rows, piece c of batch row b at slot c ^ ((b >> 2) & 3) -- rows
//     b, b + 4, b + 8, b + 12 share a quarter of the banks and the XOR tells them apart for the 16 lanes of a consumer's 16-byte read.
//     Rows past `rows`, output rows past `out` and columns past `in` enter as ZEROS: the transposed reads need EXEC all ones, so data
//     is masked, never lanes, and every wave runs the same control flow.
//   * The operands are swapped (A = W^T, B = gy^T) and the columns of a wave's two MFMA blocks are interleaved in fours, so a lane
//     ends with 8 consecutive columns of one batch row: fp32 accumulators, one rounding, one 16-byte store.
// LDS per block = 2 x 8 KiB of W image + 2 x TP x 64 bytes of gy image: 18 / 24 / 48 KiB.
//
// Splitting the output rows.  `splits` blocks per tile share the steps; their fp32 tiles go to a workspace [splits][rows][in] and a
// second kernel adds them in slice order before the one rounding -- deterministic, no atomics; a slice without steps writes zeros.
// splits == 1 writes gx directly.
//
// Numerics: exact products of storage-type operands, fp32 accumulation over o ascending (per slice).  An MFMA output column depends
// on its own gy row only: a row's bits depend neither on the other rows of the call nor on their number, for given splits.
#include <algorithm>

#include "gemm_rows16.h"

namespace aqlm {
namespace {

constexpr int kXCols = 128;     // columns of gx per block
constexpr int kXRows = 32;      // output rows of W per step (the k of one MFMA)
constexpr int kXThreads = 256;  // 4 waves, 32 columns each
constexpr uint32_t kXWBytes = kXRows * kXCols * 2;
constexpr int kXMaxSplits = 16;
constexpr int kXFullGrid = 256;  // blocks from which the device counts as filled (one per CU)

struct XtArgs {
  const uint32_t* codes;     // [M][in_groups] u16, read as the dwords that hold them (M * in_groups is even)
  const uint8_t* codebook;   // [65536][G] storage type
  const uint32_t* scales;    // [M] of the storage type, read as the dwords that hold them (M is even)
  const uint16_t* gy;        // [rows][gys]
  uint16_t* gx;              // [rows][gxs]
  float* partial;            // [splits][rows][N], splits > 1
  long gys, gxs;
  int rows, M, N, in_groups, nsteps, steps_per_slice, splits;
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* glds_s16x4_ptr;

// byte offset of 16-byte piece ch (8 columns) of row `row` in the W image (the header has the bank argument)
__device__ __forceinline__ uint32_t ximg(int row, int ch) { return 256u * row + 16u * (ch ^ ((row & 3) << 2)); }
// ... and of piece c (8 rows of W) of batch row b in the gy image
__device__ __forceinline__ uint32_t xgy(int b, int c) { return 64u * b + 16u * (c ^ ((b >> 2) & 3)); }

template <class T>
__device__ __forceinline__ uint32_t xpack2(float a, float b) { return (uint32_t)T::from_float(a) | ((uint32_t)T::from_float(b) << 16); }

// the bits aqlm_hip_dequant_1x16 writes for two neighbours: the product exists in fp32 before the one rounding
template <class T>
__device__ __forceinline__ uint32_t scaled2(uint32_t e, float scale) {
  float lo = T::lo(e) * scale, hi = T::hi(e) * scale;
  asm volatile("" : "+v"(lo), "+v"(hi));
  return xpack2<T>(lo, hi);
}

template <class T, int G, int NPT>
__global__ __launch_bounds__(kXThreads) void gemm_1x16_transposed_kernel(const XtArgs a) {
  constexpr int TP = 16 * NPT;                                  // batch rows of a tile
  constexpr int ACH = (TP * 4 + kXThreads - 1) / kXThreads;     // 16-byte pieces of the gy image per thread
  constexpr uint32_t A_BYTES = TP * 64u, A_BASE = 2u * kXWBytes;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kXWBytes + 2 * A_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col0 = blockIdx.x * kXCols, row0 = blockIdx.y * TP, slice = blockIdx.z;
  const int s0 = slice * a.steps_per_slice, s1 = min(s0 + a.steps_per_slice, a.nsteps);  // (uniform; s0 >= s1: an empty slice)

  // ---- this thread's share of the W image: piece ch of rows wr and wr + 16 -------------------------------------------------------
  const int ch = tid & 15, wr = tid >> 4;
  const bool col_ok = col0 + ch * 8 < a.N;
  int cg = G == 8 ? col0 / 8 + ch : col0 / 16 + (ch >> 1);  // the code of a row that covers the piece
  cg = cg < a.in_groups ? cg : a.in_groups - 1;
  const uint32_t half_off = G == 8 ? 0u : (uint32_t)(ch & 1) * 16u;
  const uint32_t wdst[2] = {ximg(wr, ch), ximg(wr + 16, ch)};
  const bool swap_halves = (wr & 8) != 0;  // (rows wr and wr + 16 share bit 3)
  const uint32_t scale_shift = (uint32_t)(wr & 1) * 16u;  // (... and bit 0: where the row's scale lies in its dword)
  // ---- ... and of the gy image: piece ac (8 output rows) of batch row ab ---------------------------------------------------------
  int ab[ACH], ac[ACH];
  bool aok[ACH];  // false: a row past `rows`, or a thread without a piece
  const uint16_t* gsrc[ACH];  // (those without a row: row 0's)
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int j = tid + i * kXThreads;
    ab[i] = j >> 2;
    ac[i] = j & 3;
    aok[i] = j < TP * 4 && row0 + ab[i] < a.rows;
    gsrc[i] = a.gy + (size_t)(aok[i] ? row0 + ab[i] : 0) * a.gys;
  }

  // (a step past the last: clamped copies, never used)
  auto w_row = [&](int q, int h) {
    q = q < a.nsteps ? q : a.nsteps - 1;
    const int r = q * kXRows + wr + 16 * h;
    return r < a.M ? r : a.M - 1;
  };
  auto load_codes = [&](int q, uint32_t (&c)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) c[h] = a.codes[((size_t)w_row(q, h) * a.in_groups + cg) >> 1];
  };
  auto gather = [&](int q, const uint32_t (&c)[2], u32x4 (&w)[2], uint32_t (&sc)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = w_row(q, h);
      const uint32_t code = (c[h] >> ((((uint32_t)r * (uint32_t)a.in_groups + (uint32_t)cg) & 1u) * 16u)) & 0xffffu;
      w[h] = *reinterpret_cast<const u32x4*>(a.codebook + (size_t)code * (G * 2) + half_off);
      sc[h] = a.scales[r >> 1];
    }
  };
  auto load_gy = [&](int q, u32x4 (&g)[ACH]) {
    q = q < a.nsteps ? q : a.nsteps - 1;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      int o = q * kXRows + ac[i] * 8;
      o = o < a.M ? o : a.M - 8;  // (M % 8 == 0: a piece is inside or outside as a whole)
      g[i] = *reinterpret_cast<const u32x4*>(gsrc[i] + o);
    }
  };
  // step q -> LDS: the image holds the bits aqlm_hip_dequant_1x16 would have written
  auto put = [&](int q, int buf, const u32x4 (&w)[2], const uint32_t (&sc)[2], const u32x4 (&g)[ACH]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float scale = T::to_float((uint16_t)(sc[h] >> scale_shift));  // (a row the clamp moved is masked below)
      const uint32_t ok = col_ok && q * kXRows + wr + 16 * h < a.M ? ~0u : 0u;  // past the matrix: zeros, whatever the code held
      const uint32_t w0 = scaled2<T>(w[h].x, scale) & ok, w1 = scaled2<T>(w[h].y, scale) & ok;
      const uint32_t w2 = scaled2<T>(w[h].z, scale) & ok, w3 = scaled2<T>(w[h].w, scale) & ok;
      *reinterpret_cast<u32x4*>(smem + buf * kXWBytes + wdst[h]) = swap_halves ? u32x4{w2, w3, w0, w1} : u32x4{w0, w1, w2, w3};
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if (tid + i * kXThreads < TP * 4) {
        const bool ok = aok[i] && q * kXRows + ac[i] * 8 < a.M;
        *reinterpret_cast<u32x4*>(smem + A_BASE + buf * A_BYTES + xgy(ab[i], ac[i])) = ok ? g[i] : u32x4{0u, 0u, 0u, 0u};
      }
    }
  };

  // ---- consumer addresses: wave w owns columns 32 w .. 32 w + 31; row i of its MFMA block nn is column 8 (i >> 2) + 4 nn + (i & 3) --
  const int kg = lane >> 4, li = lane & 15;
  uint32_t wsrc[2][2];  // [block][rows 8 kg + 4 h ..]: lane 4 q + p of a 16-lane group gives row q, half nn of piece 4 w + p
#pragma unroll
  for (int nn = 0; nn < 2; ++nn)
#pragma unroll
    for (int h = 0; h < 2; ++h) wsrc[nn][h] = ximg(8 * kg + 4 * h + (li >> 2), 4 * wave + (li & 3)) + 8u * (uint32_t)(nn ^ (kg & 1));
  const uint32_t asrc = A_BASE + xgy(li, kg);  // (batch row 16 t + li: 1024 t bytes further, the XOR sees b mod 16 only)

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
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kXWBytes + wsrc[nn][0]));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kXWBytes + wsrc[nn][1]));
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
    if (b < a.rows && cc < a.N) {  // (N % 8 == 0: the 8 columns are inside or outside as a whole)
      const f32x4 x = acc[t][0], y = acc[t][1];
      if (a.splits == 1) {
        *reinterpret_cast<u32x4*>(a.gx + (size_t)b * a.gxs + cc) = u32x4{xpack2<T>(x[0], x[1]), xpack2<T>(x[2], x[3]), xpack2<T>(y[0], y[1]), xpack2<T>(y[2], y[3])};
      } else {
        float* dst = a.partial + ((size_t)slice * a.rows + b) * a.N + cc;
        *reinterpret_cast<f32x4*>(dst) = x;
        *reinterpret_cast<f32x4*>(dst + 4) = y;
      }
    }
  }
}

// the slices meet: fp32 sums in slice order, one rounding; a thread owns 8 columns of a row
template <class T>
__global__ __launch_bounds__(256) void gemm_1x16_transposed_finalize_kernel(const float* partial, uint16_t* gx, long gxs, int rows, int N, int splits) {
  const size_t n8 = (size_t)N / 8, total = (size_t)rows * n8, plane = (size_t)rows * N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / n8, c = (i - b * n8) * 8;
    const float* src = partial + b * N + c;
    f32x4 x = *reinterpret_cast<const f32x4*>(src), y = *reinterpret_cast<const f32x4*>(src + 4);
    for (int z = 1; z < splits; ++z) {
      x += *reinterpret_cast<const f32x4*>(src + z * plane);
      y += *reinterpret_cast<const f32x4*>(src + z * plane + 4);
    }
    *reinterpret_cast<u32x4*>(gx + b * gxs + c) = u32x4{xpack2<T>(x[0], x[1]), xpack2<T>(x[2], x[3]), xpack2<T>(y[0], y[1]), xpack2<T>(y[2], y[3])};
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
  const long col_blocks = (N + kXCols - 1) / kXCols;
  if (rows <= 16) return 16;
  return rows > 64 && (long)((rows + 255) / 256) * col_blocks >= kXFullGrid ? 256 : 64;
}

// splits == 0: enough slices to give every CU a block, while the workspace stays within a quarter of the W it replaces
// (splits * rows * in * 4 <= out * in * 2 / 4) and every slice has steps
int xt_choose_splits(int rows, int M, int N) {
  const int tp = xt_tile_rows(rows, N);
  const long blocks = (long)((rows + tp - 1) / tp) * ((N + kXCols - 1) / kXCols);
  const long nsteps = (M + kXRows - 1) / kXRows;
  const long s = std::min<long>({(kXFullGrid + blocks - 1) / blocks, nsteps, (long)M / (8L * rows), (long)kXMaxSplits});
  return s < 2 ? 1 : (int)s;
}

template <class T, int G, int NPT>
int launch_xt_tile(const XtArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kXCols - 1) / kXCols), (unsigned)((a.rows + 16 * NPT - 1) / (16 * NPT)), (unsigned)a.splits);
  hipLaunchKernelGGL((gemm_1x16_transposed_kernel<T, G, NPT>), grid, dim3(kXThreads), 0, stream, a);
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

extern "C" size_t aqlm_hip_gemm_1x16_transposed_workspace_bytes(int rows, int out_features, int in_features, int splits) {
  if (rows < 1 || rows > 65536 || out_features < 1 || in_features < 1 || splits < 0 || splits > kXMaxSplits) return 0;
  if (splits == 0) splits = xt_choose_splits(rows, out_features, in_features);
  return splits <= 1 ? 0 : (size_t)splits * rows * in_features * sizeof(float);
}

extern "C" int aqlm_hip_gemm_1x16_transposed(const void* codes, const void* codebook, const void* scales, const void* gy, void* gx, int rows,
                                             int out_features, int in_features, int in_group_size, long gy_row_stride, long gx_row_stride,
                                             int dtype, int splits, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_gemm_1x16_transposed";
  if (int e = check_not_null(who, codes && codebook && scales && gy && gx)) return e;
  if (int e = check_positive(who, rows, out_features, in_features)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (!xt_supported(out_features, in_features, in_group_size) || rows > 65536 || splits < 0 || splits > kXMaxSplits || !aligned4(codes) ||
      !aligned16(codebook) || !aligned4(scales) || !aligned16(gy) || !aligned16(gx) || gy_row_stride % 8 != 0 || gx_row_stride % 8 != 0 ||
      gy_row_stride < out_features || gx_row_stride < in_features) {
    set_last_error("%s: outside the transposed kernel (%d rows, out=%d in=%d, g=%d, splits %d, row strides %ld / %ld; g 8 / 16, out %% 8 "
                   "== 0, in %% g == 0, an even number of codes, 4-B aligned codes and scales, 16-B aligned codebook and rows)",
                   who, rows, out_features, in_features, in_group_size, splits, gy_row_stride, gx_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int tp = xt_tile_rows(rows, in_features);
  if (splits == 0) splits = xt_choose_splits(rows, out_features, in_features);
  if (splits > 1 && (!workspace || !aligned16(workspace) || workspace_bytes < (size_t)splits * rows * in_features * sizeof(float))) {
    set_last_error("%s: %d slices need a 16-B aligned workspace of %zu bytes, got %zu", who, splits,
                   (size_t)splits * rows * in_features * sizeof(float), workspace ? workspace_bytes : (size_t)0);
    return AQLM_HIP_E_INVALID;
  }
  XtArgs a{};
  a.codes = (const uint32_t*)codes;
  a.codebook = (const uint8_t*)codebook;
  a.scales = (const uint32_t*)scales;
  a.gy = (const uint16_t*)gy;
  a.gx = (uint16_t*)gx;
  a.partial = (float*)workspace;
  a.gys = gy_row_stride;
  a.gxs = gx_row_stride;
  a.rows = rows;
  a.M = out_features;
  a.N = in_features;
  a.in_groups = in_features / in_group_size;
  a.nsteps = (out_features + kXRows - 1) / kXRows;
  a.splits = splits;
  a.steps_per_slice = (a.nsteps + splits - 1) / splits;
  hipStream_t stream = (hipStream_t)stream_;
  const int e = dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) { return launch_xt<decltype(t), decltype(g)::value>(a, tp, stream); });
  if (e || splits == 1) return e;
  const size_t items = (size_t)rows * (in_features / 8);
  const unsigned blocks = (unsigned)std::min<size_t>((items + 255) / 256, 256u * 16u);
  if (dtype == AQLM_HIP_F16)
    hipLaunchKernelGGL(gemm_1x16_transposed_finalize_kernel<F16>, dim3(blocks), dim3(256), 0, stream, a.partial, a.gx, a.gxs, rows, in_features, splits);
  else
    hipLaunchKernelGGL(gemm_1x16_transposed_finalize_kernel<BF16>, dim3(blocks), dim3(256), 0, stream, a.partial, a.gx, a.gxs, rows, in_features, splits);
  return check_hip(hipGetLastError(), "gemm_1x16_transposed finalize launch");
}

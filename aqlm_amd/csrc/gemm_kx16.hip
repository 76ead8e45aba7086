// K x 9..16-bit AQLM layers at 7+ rows: dequantise fused INTO the MFMA, gfx950.
//
//   y[b, o] = (sum_i sum_k codebooks[k][codes[o, i / 8, k] & mask][i % 8] * x[b, i]) * scales[o] + bias[o]
//
// K = 2 or 4 codebooks of 2^nbits entries (nbits 9 .. 16) in 16-bit containers, g 8: the 2x12 and 2x16 schemes of the AQLM paper's 3-
// and 4-bit models, and 4x16.  Codes int16 [out][in / 8][K] in the checkpoint layout, codebooks [K][2^nbits][8] of the storage type.
//
//   * W never exists, not even in a register.  The weight of a group is the SUM of K codebook vectors; v_mfma_f32_16x16x32 sums
//     products into an fp32 accumulator; so the kernel feeds each gathered vector to an MFMA of its own, K per 32-k chunk against the
//     same X fragment, and the sum over the codebooks happens in fp32 inside the accumulator.  No VALU add, and no rounding of W to 16
//     bits as in dequantise + GEMM: the products are exact, the sums fp32.
//   * Operands.  A gathered 16-byte vector is 8 consecutive k of one output row, which is exactly what lane (li = lane & 15,
//     kg = lane >> 4) of a 16x16x32 MFMA holds of its 32 x 16 operand: column li (output row row0 + li), k-octet kg.  So lane (li, kg)
//     loads the K codes of (row0 + li, group 4 c + kg) as ONE 4- or 8-byte word and gathers its own operand; nothing passes through LDS.
//     The other operand is X: lane (li, kg) holds x[b0 + 16 t + li, 32 c + 8 kg ..] for batch tile t, one 16-byte load from global
//     memory (X is small and shared by every workgroup: it stays in L2 / the vector L1).  The accumulator of lane (li, kg) is then
//     y[b0 + 16 t + 4 kg + j, row0 + li], j = 0 .. 3: one scale and one bias per lane.
//   * Work split.  A workgroup owns 16 output rows over ALL of k: no partial sums in global memory, no workspace, no second kernel.
//     Its 8 waves deal the chunks among themselves in contiguous ranges (ceil(chunks / 8) each; the last ranges may be short or
//     empty) -- a workgroup of one wave would leave a CU with 4 waves of latency hiding for what is a gather-bound kernel -- and meet
//     once at the end: every wave puts its accumulators in LDS, wave t adds those of tile t in wave order 0 .. 7 and writes y.  The
//     order is fixed, so two calls give the same bits; a row's bits depend neither on the other rows nor on their number (the MFMA
//     treats the batch columns independently and the chunk ranges depend on in_features alone).
//   * Register ring, D chunks deep (8 at one batch tile and 2 codebooks, else 4: the ring of K x D gathered vectors and NBT x D X
//     fragments has to fit beside NBT accumulators in the 256 VGPRs a 512-thread block leaves a lane): the code word of chunk c is
//     requested in iteration c - 2 D, its K gathers and the X fragments in iteration c - D.  Every load is unconditional and from a
//     clamped address -- chunk min(c, chunks - 1), row min(row, out - 1), batch row min(b, rows - 1); a code is masked to the
//     codebook -- so nothing is read outside a buffer and no branch stands around a load; the gathers go through a buffer descriptor of
//     exactly the codebooks' bytes on top of that.  Only the store is masked.
//   * Up to 4 batch tiles (64 rows) per launch; the entry loops over passes of 64 rows, each a launch that gathers again -- which is
//     why the route ends at a measured row count (hip_kernel.FUSED_KX16_MAX_ROWS) and dequantise + GEMM takes over.
//   * Why the codebooks stay in L2 even where they would fit in LDS (2x12: 2 x 4096 x 16 B = 128 KiB): DESIGN.md section 4.8v.
#include "gemm_rows16.h"

namespace aqlm {
namespace {

constexpr int kKxWaves = 8;             // waves of a workgroup: they deal the k chunks
constexpr int kKxThreads = 64 * kKxWaves;
constexpr int kKxPassRows = 64;         // batch rows of a launch: 4 tiles of 16

struct Kx16Args {
  const uint8_t* codes;      // [M][in_groups][K] u16
  const uint8_t* codebooks;  // [K][entries][8] storage type
  const uint16_t* scales;    // [M]
  const uint16_t* bias;      // [M] or null
  const uint16_t* x;         // [rows][xs]
  uint16_t* y;               // [rows][ys]
  long xs, ys;
  int rows, M, in_groups, nchunks, chunks_per_wave;
  uint32_t entries, mask, cb_bytes;
};

template <int KC>
struct CodeWord;
template <>
struct CodeWord<2> {
  typedef uint32_t type;
};
template <>
struct CodeWord<4> {
  typedef u32x2 type;
};

// code k of the word that holds the KC codes of a group
__device__ __forceinline__ uint32_t kx_code(uint32_t w, int k) { return (w >> (16 * k)) & 0xffffu; }
__device__ __forceinline__ uint32_t kx_code(const u32x2& w, int k) { return ((k < 2 ? w.x : w.y) >> (16 * (k & 1))) & 0xffffu; }

template <class T, int KC, int NBT>
__global__ __launch_bounds__(kKxThreads) void gemm_kx16_rows_kernel(const Kx16Args a) {
  typedef typename CodeWord<KC>::type cw_t;
  constexpr int D = (KC == 2 && NBT == 1) ? 8 : 4;
  __shared__ __attribute__((aligned(16))) f32x4 red[kKxWaves][NBT][64];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kg = lane >> 4;
  const int row = blockIdx.x * 16 + li;
  const int row_c = row < a.M ? row : a.M - 1;
  const int c0 = wave * a.chunks_per_wave;                                                          // (uniform)
  const int c1 = c0 + a.chunks_per_wave < a.nchunks ? c0 + a.chunks_per_wave : a.nchunks;           // (c0 >= c1: a wave without chunks)

  // the K codes of (row, group 4 c + kg): one aligned word (in_groups % 4 == 0: group 4 c + kg exists for every c < nchunks)
  const uint8_t* const code_row = a.codes + (size_t)row_c * a.in_groups * (KC * 2);
  auto load_codes = [&](int c) -> cw_t {
    c = c < a.nchunks ? c : a.nchunks - 1;
    return *reinterpret_cast<const cw_t*>(code_row + (size_t)(4 * c + kg) * (KC * 2));
  };
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.codebooks, 0, (int)a.cb_bytes, 0x00020000);
  auto gather = [&](const cw_t& cw, u32x4 (&w)[KC]) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const uint32_t off = ((uint32_t)k * a.entries + (kx_code(cw, k) & a.mask)) * 16u;
      w[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, AUX_DEFAULT);
    }
  };
  // batch row 16 t + li of the pass, k-octet kg of chunk c
  const uint16_t* xrow[NBT];
#pragma unroll
  for (int t = 0; t < NBT; ++t) {
    const int b = 16 * t + li;
    xrow[t] = a.x + (size_t)(b < a.rows ? b : a.rows - 1) * (size_t)a.xs + 8 * kg;
  }
  auto load_x = [&](int c, u32x4 (&xf)[NBT]) {
    c = c < a.nchunks ? c : a.nchunks - 1;
#pragma unroll
    for (int t = 0; t < NBT; ++t) xf[t] = *reinterpret_cast<const u32x4*>(xrow[t] + (size_t)32 * c);
  };

  // epilogue operands: unconditional loads (clamped row; the bias pointer aliased to the scales when absent)
  const uint16_t scale_h = a.scales[row_c];
  const uint16_t bias_h = (a.bias ? a.bias : a.scales)[row_c];

  f32x4 acc[NBT];
#pragma unroll
  for (int t = 0; t < NBT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  cw_t cw[D];
  u32x4 w[D][KC], xf[D][NBT];
#pragma unroll
  for (int j = 0; j < D; ++j) cw[j] = load_codes(c0 + j);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    gather(cw[j], w[j]);
    load_x(c0 + j, xf[j]);
    cw[j] = load_codes(c0 + j + D);
  }
  auto consume = [&](int j) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int t = 0; t < NBT; ++t) acc[t] = mfma16<T>(xf[j][t], w[j][k], acc[t]);
  };
  // whole rounds of D chunks without a branch inside (a branch makes the compiler wait for every load in flight where its paths
  // join); unrolled: every register set of the ring has a fixed name
  int q0 = c0;
  for (; q0 + D <= c1; q0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      consume(j);
      gather(cw[j], w[j]);  // chunk q0 + j + D
      load_x(q0 + j + D, xf[j]);
      cw[j] = load_codes(q0 + j + 2 * D);
      __builtin_amdgcn_sched_barrier(0);  // (keep the steps apart: scheduled together, all their loads are waited for at once)
    }
  }
  // the last c1 - q0 < D chunks are in the ring already
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (q0 + j < c1) consume(j);  // (uniform)

  // ---- the waves meet: tile t is added by wave t, in wave order ----------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < NBT; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave < NBT) {
    f32x4 s = red[0][wave][lane];
#pragma unroll
    for (int v = 1; v < kKxWaves; ++v) s += red[v][wave][lane];
    const float scale = T::to_float(scale_h);
    const float bias = a.bias ? T::to_float(bias_h) : 0.f;
    if (row < a.M) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = 16 * wave + 4 * kg + j;
        if (b < a.rows) a.y[(size_t)b * a.ys + row] = T::from_float(__builtin_fmaf(s[j], scale, bias));
      }
    }
  }
}

bool kx16_supported(int M, int N, int K, int nbits, int G, int rows) {
  return M >= 1 && N >= 32 && N % 32 == 0 && (K == 2 || K == 4) && nbits >= 9 && nbits <= 16 && G == 8 && rows >= 1 && rows <= 65536;
}

template <class T, int KC>
int launch_kx16(const Kx16Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.M + 15) / 16)), block(kKxThreads);
  const int tiles = (a.rows + 15) / 16;
  if (tiles <= 1) hipLaunchKernelGGL((gemm_kx16_rows_kernel<T, KC, 1>), grid, block, 0, stream, a);
  else if (tiles == 2) hipLaunchKernelGGL((gemm_kx16_rows_kernel<T, KC, 2>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((gemm_kx16_rows_kernel<T, KC, 4>), grid, block, 0, stream, a);
  return check_hip(hipGetLastError(), "gemm_kx16_rows launch");
}

}  // namespace
}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_gemm_kx16_rows_supported(int out_features, int in_features, int num_codebooks, int nbits, int in_group_size,
                                                 int rows) {
  return kx16_supported(out_features, in_features, num_codebooks, nbits, in_group_size, rows) ? 1 : 0;
}

extern "C" int aqlm_hip_gemm_kx16_rows(const void* codes, const void* codebooks, const void* scales, const void* bias, const void* x,
                                       void* y, int rows, int out_features, int in_features, int num_codebooks, int nbits,
                                       int in_group_size, long xs, long ys, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_gemm_kx16_rows";
  if (int e = check_not_null(who, codes && codebooks && scales && x && y)) return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  if (rows <= 0) {
    set_last_error("%s: sizes must be positive", who);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_x_row_stride(who, rows, in_features, xs)) return e;
  if (nbits < 9 || nbits > 16 || num_codebooks < 2 || num_codebooks > 8) {
    set_last_error("%s: nbits %d / num_codebooks %d unsupported (9..16 bits in 16-bit containers, 2..8 codebooks)", who, nbits,
                   num_codebooks);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int K = num_codebooks;
  if (!kx16_supported(out_features, in_features, K, nbits, in_group_size, rows) || tuning().force_generic ||
      (K == 2 ? !aligned4(codes) : !aligned8(codes)) || !aligned16(codebooks) || !aligned16(x) || !aligned2(scales) ||
      (bias && !aligned2(bias)) || !aligned2(y) || xs % 8 != 0) {
    set_last_error("%s: outside the fused kernel (%d rows, out=%d in=%d, %dx%d g=%d, row strides %ld / %ld; 2 or 4 codebooks, g 8, "
                   "in %% 32 == 0, codes aligned to a group's word, 16-B aligned codebooks and rows of x)",
                   who, rows, out_features, in_features, K, nbits, in_group_size, xs, ys);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  Kx16Args a{};
  a.codes = (const uint8_t*)codes;
  a.codebooks = (const uint8_t*)codebooks;
  a.scales = (const uint16_t*)scales;
  a.bias = (const uint16_t*)bias;
  a.xs = xs;
  a.ys = ys;
  a.M = out_features;
  a.in_groups = in_features / 8;
  a.nchunks = in_features / 32;
  a.chunks_per_wave = (a.nchunks + kKxWaves - 1) / kKxWaves;
  a.entries = 1u << nbits;
  a.mask = a.entries - 1u;
  a.cb_bytes = (uint32_t)K * a.entries * 16u;
  hipStream_t stream = (hipStream_t)stream_;
  for (int done = 0; done < rows; done += kKxPassRows) {
    a.rows = rows - done < kKxPassRows ? rows - done : kKxPassRows;
    a.x = (const uint16_t*)x + (size_t)done * xs;
    a.y = (uint16_t*)y + (size_t)done * ys;
    int e;
    if (dtype == AQLM_HIP_F16) e = K == 2 ? launch_kx16<F16, 2>(a, stream) : launch_kx16<F16, 4>(a, stream);
    else e = K == 2 ? launch_kx16<BF16, 2>(a, stream) : launch_kx16<BF16, 4>(a, stream);
    if (e) return e;
  }
  return 0;
}

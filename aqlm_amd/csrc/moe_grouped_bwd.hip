// Input gradient of the expert-grouped 1x16 GEMM (moe_grouped.hip): the TRANSPOSED product of a mixture-of-experts block, gfx950.
//
//   gx[p, :] = sum_s (gy[p, s, :] * scales[e_p, s]) @ Wq[e_p, s]          fp32 [num_pairs][in_features]
//
// One launch per projection group on the bucket the forward made (aqlm_hip_moe_bucket), on a grid of column blocks x tile slots
// that depends on the shapes only.  W is never written to memory: a block owns its tile's pairs x 128 columns of gx over ALL
// output rows and both segments (no partial sums, no finalize) and walks the rows in steps of 32:
//   * every thread fetches two 16-byte pieces of the step's codebook vectors (code word, then the gather) and, for the tile's
//     gy rows, 8 values and their scales; both land in registers, requested 8 steps ahead for tiles of 16 / 32 pairs and 4 for
//     larger ones (the code words twice as far), while the MFMAs of the steps before run, and go to LDS one step ahead (two
//     buffers, one barrier per step);
//   * the W image of a step is [32 rows][128 columns], as the codebook vectors lie; the product sums over its ROWS, so the waves
//     read it column-major with ds_read_b64_tr_b16 (two reads make the 8 k values of one v_mfma_f32_16x16x32 operand) through
//     the XOR swizzle of 256-byte rows under which the transposed reads of a 32-lane half share no bank;
//   * gy * scales is formed in fp32 and rounded once to the storage type: the other MFMA operand.
// The operands are swapped (A = W^T, B = (gy scales)^T), so a lane ends with 4 consecutive columns of one pair: 16-byte stores.
// Registers, not LDS-DMA rings with producer waves as in gemm_rows16_body.h: the images take 18 - 32 KiB per block, several blocks
// share a CU, every wave stays an MFMA consumer, and the waits are the compiler's counted ones (DESIGN.md section 4.8e lists the
// three ways in which hipcc turned them into full drains, and what the code does about each).
//
// Numerics: exact products of storage-type operands, fp32 accumulation in a fixed order (segment, then output row ascending).
// An MFMA output column depends on its own B column only, so a pair's bits depend on its gy row and its expert alone -- not on
// the other pairs, the tile size or the slot.
#include "gemm_rows16.h"
#include "moe_bucket.h"

namespace aqlm {
namespace {

constexpr int kBwdCols = 128;     // columns of gx per block
constexpr int kBwdRows = 32;      // output rows of W per step (the k of one MFMA)
constexpr int kBwdThreads = 256;  // 4 waves, 32 columns each
constexpr uint32_t kBwdWBytes = kBwdRows * kBwdCols * 2;

struct BwdArgs {
  const aqlm_hip_routed_entry* table;  // device, [nexp][nseg]
  const int* bucket;                   // from moe_bucket_kernel
  const uint16_t* gy;                  // [npairs][nseg][M], pair stride gys
  float* gx;                           // [npairs][K]
  long gys;
  int nexp, nseg, npairs, tile_pairs, max_tiles;
  int M, K, in_groups, msteps;         // msteps = ceil(M / 32)
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
// pointers read from the table are global memory: said so, or the loads become flat ones, which the LDS waits would then cover
typedef __attribute__((address_space(1))) const uint32_t* ggbl_u32_ptr;
typedef __attribute__((address_space(1))) const u32x4* ggbl_u32x4_ptr;
typedef __attribute__((address_space(3))) s16x4* glds_s16x4_ptr;

// byte offset of 16-byte piece ch (8 columns) of row `row` in the W image: 256-byte rows, pieces XORed so that a transposed read
// (4 rows x 16 columns per 16 lanes, a half's two blocks 8 rows apart) meets 32 distinct 8-byte bank pairs
__device__ __forceinline__ uint32_t wimg(int row, int ch) { return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
// ... and of piece c (8 rows of W) of batch row b in the gy image: 64-byte rows
__device__ __forceinline__ uint32_t aimg(int b, int c) { return 64u * b + 16u * (c ^ ((b >> 1) & 3)); }

template <class T, int G, int NPT>
__global__ __launch_bounds__(kBwdThreads) void gemm_1x16_grouped_transposed_kernel(const BwdArgs a) {
  constexpr int TP = 16 * NPT;                                  // pairs of a full tile
  constexpr int ACH = (TP * 4 + kBwdThreads - 1) / kBwdThreads;  // 16-byte pieces of the gy image per thread
  constexpr uint32_t A_BYTES = TP * 64u, A_BASE = 2u * kBwdWBytes;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kBwdWBytes + 2 * A_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = blockIdx.y, col0 = blockIdx.x * kBwdCols;
  const int* list = bucket_list(a.bucket, a.max_tiles);
  if (slot == 0) {  // the pairs of out-of-range ids get zero rows
    int nbad;
    const int* bad = bucket_bad_pairs(a.bucket, list, a.npairs, nbad);
    for (int i = tid; i < nbad * (kBwdCols / 4); i += kBwdThreads) {
      const int pr = bad[i / (kBwdCols / 4)], c = col0 + (i % (kBwdCols / 4)) * 4;
      if ((unsigned)pr < (unsigned)a.npairs && c < a.K) *reinterpret_cast<f32x4*>(a.gx + (size_t)pr * a.K + c) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  if (slot >= a.bucket[0]) return;
  const int4 tile = bucket_tile(a.bucket, slot);
  const int e = tile.x, first = tile.y, count = tile.z;
  if (e < 0 || e >= a.nexp || count < 1 || count > a.tile_pairs || count > TP || first < 0 || first > a.npairs - count) return;  // (a foreign bucket)
  // from here on every wave runs the same control flow with all lanes on: the transposed reads need EXEC all ones
  const aqlm_hip_routed_entry ent0 = a.table[e * a.nseg], ent1 = a.table[e * a.nseg + a.nseg - 1];
  const int* pairs = list + first;
  const int nsteps = a.nseg * a.msteps;

  // ---- this thread's share of the W image: piece ch of rows wr and wr + 16 ------------------------------------------------
  const int ch = tid & 15, wr = tid >> 4;
  const bool col_ok = col0 + ch * 8 < a.K;
  int cg = G == 8 ? col0 / 8 + ch : col0 / 16 + (ch >> 1);  // code of the row that covers the piece
  cg = cg < a.in_groups ? cg : a.in_groups - 1;
  const uint32_t half_off = G == 8 ? 0u : (uint32_t)(ch & 1) * 16u;
  const uint32_t wdst[2] = {wimg(wr, ch), wimg(wr + 16, ch)};
  // ---- ... and of the gy image: piece ac of batch row ab ----------------------------------------------------------------------
  // The loads below are unconditional, from clamped addresses, and their values are used nowhere before `put`: a select or a
  // conversion next to a load would make the compiler wait for it there, with every younger load (checked in the -S output).
  int ab[ACH], ac[ACH];
  bool aok[ACH];              // false: a padding row of a short tile, or a thread without a piece
  const uint16_t* gsrc[ACH];  // the pair's gy row (those without one: pair 0's)
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int j = tid + i * kBwdThreads;
    ab[i] = j >> 2;
    ac[i] = j & 3;
    int pr = -1;
    if (j < TP * 4 && ab[i] < count) pr = pairs[ab[i]];
    aok[i] = (unsigned)pr < (unsigned)a.npairs;
    gsrc[i] = a.gy + (size_t)(aok[i] ? pr : 0) * a.gys;
  }

  auto seg_of = [&](int q) { return q >= a.msteps ? 1 : 0; };
  // A code word is fetched as the aligned dword that holds it and cut out where it is used, D iterations later: a 16-bit load is
  // extended (or packed with its neighbour) right behind the load, which waits for it there.  (The codes of a layer are an even
  // number of 16-bit words from a 16-byte aligned base: the dword never leaves them.)
  auto code_index = [&](int q, int h) {
    const int s = seg_of(q), r0 = (q - s * a.msteps) * kBwdRows;
    int r = r0 + wr + 16 * h;
    r = r < a.M ? r : a.M - 1;
    return (size_t)r * a.in_groups + cg;
  };
  auto load_codes = [&](int q, uint32_t (&c)[2]) {
    q = q < nsteps ? q : nsteps - 1;
    const ggbl_u32_ptr codes = (ggbl_u32_ptr)(seg_of(q) ? ent1.codes : ent0.codes);
#pragma unroll
    for (int h = 0; h < 2; ++h) c[h] = codes[code_index(q, h) >> 1];
  };
  auto gather = [&](int q, const uint32_t (&c)[2], u32x4 (&w)[2]) {
    q = q < nsteps ? q : nsteps - 1;
    const uintptr_t cb = (uintptr_t)(seg_of(q) ? ent1.codebook : ent0.codebook);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t code = (c[h] >> (((uint32_t)code_index(q, h) & 1u) * 16u)) & 0xffffu;
      w[h] = *(ggbl_u32x4_ptr)(cb + (size_t)code * (G * 2) + half_off);
    }
  };
  auto load_a = [&](int q, u32x4 (&g)[ACH], u32x4 (&sc)[ACH]) {
    q = q < nsteps ? q : nsteps - 1;
    const int s = seg_of(q), r0 = (q - s * a.msteps) * kBwdRows;
    const uintptr_t scales = (uintptr_t)(s ? ent1.scales : ent0.scales);
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      int r = r0 + ac[i] * 8;
      r = r < a.M ? r : a.M - 8;  // (M % 8 == 0: a piece is inside or outside as a whole)
      g[i] = *reinterpret_cast<const u32x4*>(gsrc[i] + (size_t)s * a.M + r);
      sc[i] = *(ggbl_u32x4_ptr)(scales + (size_t)r * 2);
    }
  };
  auto put = [&](int q, int buf, const u32x4 (&w)[2], const u32x4 (&g)[ACH], const u32x4 (&sc)[ACH]) {  // step q -> LDS
    q = q < nsteps ? q : nsteps - 1;
    const int r0 = (q - seg_of(q) * a.msteps) * kBwdRows;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // past the matrix: zeros, whatever the code held
      const bool ok = col_ok && r0 + wr + 16 * h < a.M;
      *reinterpret_cast<u32x4*>(smem + buf * kBwdWBytes + wdst[h]) = ok ? w[h] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if (tid + i * kBwdThreads < TP * 4) {
        const bool ok = aok[i] && r0 + ac[i] * 8 < a.M;
        u32x4 o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {  // gy * scale in fp32, one rounding
          const uint32_t lo = T::from_float(T::lo(g[i][d]) * T::lo(sc[i][d])), hi = T::from_float(T::hi(g[i][d]) * T::hi(sc[i][d]));
          o[d] = ok ? lo | (hi << 16) : 0u;
        }
        *reinterpret_cast<u32x4*>(smem + A_BASE + buf * A_BYTES + aimg(ab[i], ac[i])) = o;
      }
    }
  };

  // ---- consumer addresses: wave w owns columns 32 w .. 32 w + 31, two 16-column blocks ----------------------------------------
  const int kg = lane >> 4, li = lane & 15;
  uint32_t wsrc[2][2];  // [column block][rows 8 kg + 4 h ..]: lane 4 q + p of a 16-lane group gives row q, columns 4 p .. 4 p + 3
#pragma unroll
  for (int nn = 0; nn < 2; ++nn)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      wsrc[nn][h] = wimg(8 * kg + 4 * h + (li >> 2), 2 * (2 * wave + nn) + ((li & 3) >> 1)) + 8u * (li & 1);
  uint32_t asrc[NPT];
#pragma unroll
  for (int t = 0; t < NPT; ++t) asrc[t] = A_BASE + aimg(16 * t + li, kg);

  f32x4 acc[NPT][2];
#pragma unroll
  for (int t = 0; t < NPT; ++t)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) acc[t][nn] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Register pipeline, D steps deep: step s is requested in iteration s - D (its code words D iterations before that) and goes to
  // LDS at the end of iteration s - 1, so D - 1 whole steps of other work cover the code -> codebook chain.  The loop is unrolled
  // D times: every register set and LDS buffer has a fixed name, and the counted waits the compiler places leave the younger
  // loads in flight.
  constexpr int D = NPT <= 2 ? 8 : 4;  // (small tiles: few blocks, long chains per block; large tiles: registers for the accumulators)
  static_assert(D % 2 == 0, "the LDS buffer of step s is s & 1 == (s % D) & 1");
  uint32_t c[D][2];
  u32x4 w[D][2], g[D][ACH], sc[D][ACH];
#pragma unroll
  for (int j = 0; j < D; ++j) load_codes(j, c[j]);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    gather(j, c[j], w[j]);
    load_a(j, g[j], sc[j]);
    load_codes(j + D, c[j]);
  }
  put(0, 0, w[0], g[0], sc[0]);
  __syncthreads();
  for (int q0 = 0; q0 < nsteps; q0 += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int q = q0 + j;
      if (q < nsteps) {  // (uniform; once false, false for the rest of the round)
        const int buf = j & 1;
        gather(q + D, c[j], w[j]);  // (past the last step: clamped copies, never read)
        load_a(q + D, g[j], sc[j]);
        load_codes(q + 2 * D, c[j]);
        u32x4 wf[2];
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kBwdWBytes + wsrc[nn][0]));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kBwdWBytes + wsrc[nn][1]));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          wf[nn] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
          const u32x4 gf = *reinterpret_cast<const u32x4*>(smem + buf * A_BYTES + asrc[t]);
#pragma unroll
          for (int nn = 0; nn < 2; ++nn) acc[t][nn] = mfma16<T>(wf[nn], gf, acc[t][nn]);
        }
        put(q + 1, buf ^ 1, w[(j + 1) % D], g[(j + 1) % D], sc[(j + 1) % D]);
        __syncthreads();
      }
    }
  }

  // ---- epilogue: lane (li, kg) holds columns 4 kg .. 4 kg + 3 of each of its column blocks for batch row 16 t + li ------------
#pragma unroll
  for (int t = 0; t < NPT; ++t) {
    const int b = 16 * t + li;
    if (b < count) {
      const int pr = pairs[b];
      if ((unsigned)pr < (unsigned)a.npairs) {
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
          const int c = col0 + 32 * wave + 16 * nn + 4 * kg;
          if (c < a.K) *reinterpret_cast<f32x4*>(a.gx + (size_t)pr * a.K + c) = acc[t][nn];
        }
      }
    }
  }
}

template <class T, int G>
int launch_bwd(const BwdArgs& a, dim3 grid, hipStream_t stream) {
  switch (a.tile_pairs) {
    case 16: hipLaunchKernelGGL((gemm_1x16_grouped_transposed_kernel<T, G, 1>), grid, dim3(kBwdThreads), 0, stream, a); break;
    case 32: hipLaunchKernelGGL((gemm_1x16_grouped_transposed_kernel<T, G, 2>), grid, dim3(kBwdThreads), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((gemm_1x16_grouped_transposed_kernel<T, G, 4>), grid, dim3(kBwdThreads), 0, stream, a); break;
    default: hipLaunchKernelGGL((gemm_1x16_grouped_transposed_kernel<T, G, 8>), grid, dim3(kBwdThreads), 0, stream, a); break;
  }
  return check_hip(hipGetLastError(), "gemm_1x16_grouped_transposed launch");
}

// (columns go in 16-byte pieces of 8 and stores in fours: any K of whole codebook vectors)
bool bwd_supported(int M, int K, int g) { return M > 0 && K > 0 && M % 16 == 0 && K % 16 == 0 && (g == 8 || g == 16); }

}  // namespace
}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_gemm_1x16_grouped_transposed_supported(int out_features, int in_features, int in_group_size) {
  return bwd_supported(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_gemm_1x16_grouped_transposed(const aqlm_hip_routed_entry* table, int num_experts, int num_segments,
                                                     const void* bucket, int tile_pairs, int num_pairs, const void* gy,
                                                     long gy_pair_stride, void* gx, int out_features, int in_features,
                                                     int in_group_size, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_gemm_1x16_grouped_transposed";
  if (int e = check_not_null(who, table && bucket && gy && gx)) return e;
  if (int e = check_aligned(who, "table / bucket", aligned8(table) && aligned16(bucket))) return e;
  if (int e = check_experts(who, num_experts, num_segments)) return e;
  if (num_pairs < 1 || num_pairs > AQLM_HIP_MAX_GROUPED_PAIRS || !tile_pairs_ok(tile_pairs)) {
    set_last_error("%s: %d pairs, tiles of %d (1..%d pairs; tiles of 16 / 32 / 64 / 128)", who, num_pairs, tile_pairs,
                   AQLM_HIP_MAX_GROUPED_PAIRS);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_group_size(who, in_group_size)) return e;
  if (!bwd_supported(out_features, in_features, in_group_size) || !aligned16(gy) || !aligned16(gx) || gy_pair_stride % 8 != 0 ||
      gy_pair_stride < (long)num_segments * out_features) {
    set_last_error("%s: shape outside the transposed kernel (out=%d in=%d g=%d, gy stride %ld)", who, out_features, in_features,
                   in_group_size, gy_pair_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  BwdArgs a{};
  a.table = table;
  a.bucket = (const int*)bucket;
  a.gy = (const uint16_t*)gy;
  a.gx = (float*)gx;
  a.gys = gy_pair_stride;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.npairs = num_pairs;
  a.tile_pairs = tile_pairs;
  a.max_tiles = bucket_max_tiles(num_pairs, num_experts, tile_pairs);
  a.M = out_features;
  a.K = in_features;
  a.in_groups = in_features / in_group_size;
  a.msteps = (out_features + kBwdRows - 1) / kBwdRows;
  const dim3 grid((unsigned)((in_features + kBwdCols - 1) / kBwdCols), (unsigned)a.max_tiles, 1u);
  hipStream_t stream = (hipStream_t)stream_;
  return dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) { return launch_bwd<decltype(t), decltype(g)::value>(a, grid, stream); });
}

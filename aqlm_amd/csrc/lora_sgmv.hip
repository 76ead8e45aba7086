// Segmented LoRA adapter GEMM on top of a quantized layer's output at any row count (aqlm_hip_lora_sgmv), gfx950, wave64: the
// prefill counterpart of the per-row matvec of lora_bgmv.hip, on v_mfma_f32_16x16x32_{f16,bf16}.
//
// For every row b < rows with adapter a = ids[b] (include/aqlm_hip.h states the definition):
//     t[b, r] = sum_k A_a[r, k] * x[b, k]                                    r < rank_a, fp32
//     hi = round_T(t), lo = round_T(t - float(hi))                           T = the storage type
//     y[b, i] = round_T(float(y[b, i]) + scaling_a * sum_r B_a[i, r] * (hi[b, r] + lo[b, r]))
// in two launches whose grids depend on rows, max_rank, in_features and out_features only: the ids stay on the device, nothing is
// synchronised or allocated, a captured launch stays valid when the ids change.  Which rows have an adapter is decided by the
// id and rank rules of lora_common.h, shared with lora_bgmv.hip: the others are never written and nothing is loaded through their
// table slot.
//
// Rows are cut into tiles of 16.  A workgroup reads its tile's 16 ids and serves the distinct valid adapters among them one after
// the other: the first unserved lane's id, the rows that share it by ballot, one pass, until no row is left.  In every pass ALL 16
// rows go through the MFMA (rows of other adapters produce values nobody stores; rows past `rows` load from the last row's
// address); only the rows of the pass's adapter are stored, so a row is written exactly once per launch.  Cost: one pass per
// distinct adapter of a tile -- per-sequence ids at prefill give one pass per tile and two at a seam; the worst case, 16 rows with
// 16 different adapters, is 16 passes.
//
// x [rows][in], A_a [rank][in], B_a [out][rank] and t [rows][rank] are all row-major along the summed index, and a lane's operand
// fragment of the 16x16x32 MFMA is 8 consecutive k of one row: one 16-byte global load, no LDS staging, no transposition.
//   * shrink: A operand = x rows (M = the tile's rows), B operand = A_a rows (N = 16 ranks).  K is cut into sgmv_splits(in_features)
//     slices over workgroups and each slice into fixed contiguous shares of its 4 waves; the wave sums meet in LDS and are added in
//     wave order, the slice sums go to the fp32 workspace [rows][splits][max_rank] and are added in slice order by the expand.  The
//     cut is a function of in_features alone, never of rows: a row's bits do not depend on how many rows travel with it.
//   * expand + add: A operand = B_a rows (M = 16 outputs i), B operand = hi / lo of t (N = the tile's rows), formed in registers;
//     two MFMAs per k-step, and that K is only the rank.  The C/D layout (col = lane & 15, row = (lane >> 4) * 4 + reg) then gives
//     a lane 4 consecutive i of one row b: one 8-byte read-modify-write of y; a partial last group goes element by element.
// K tails are masked at the use (both operands zeroed), loads are unconditional from clamped addresses.  No atomics; every sum has
// a fixed order that depends on the shapes only, and the rows and columns of an MFMA do not mix: a row's bits depend on its own x
// row, its own y row and its adapter.  fp16 only: |t| above 65504 has no hi / lo pair (hi is infinite) and turns the row into NaN.
#include "gemm_rows16.h"
#include "lora_common.h"

namespace aqlm {

constexpr int kSgmvWaves = 4;
constexpr int kSgmvTilesPerWave = 4;                      // neighbouring 16-output tiles of an expand wave: 128 bytes of a y row
constexpr int kSgmvSpan = kSgmvWaves * kSgmvTilesPerWave;  // 16-output tiles per expand workgroup
constexpr int kSgmvSliceK = 1024;   // elements of K a shrink workgroup aims at ...
constexpr int kSgmvMaxSplits = 8;   // ... with at most this many slices (the workspace grows with them)
constexpr int kSgmvInFlight = 8;    // k-steps a shrink wave loads before it multiplies
static_assert(kSgmvWaves == 4, "the shrink's LDS sum gives wave w the accumulator register w of every lane");

// slices of K over workgroups: a function of in_features alone
static inline int sgmv_splits(int K) { return std::min(std::max((K + kSgmvSliceK - 1) / kSgmvSliceK, 1), kSgmvMaxSplits); }

template <class T>
__device__ __forceinline__ uint32_t sgmv_hi2(float a, float b) {
  return (uint32_t)T::from_float(a) | ((uint32_t)T::from_float(b) << 16);
}
template <class T>
__device__ __forceinline__ uint32_t sgmv_lo2(float a, float b, uint32_t hi) {
  return sgmv_hi2<T>(a - T::lo(hi), b - T::hi(hi));
}

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_shrink_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                           const uint16_t* x, float* t, long xs, int ids_int64,
                                                                           int nadapters, int max_rank, int rows, int K8, int splits,
                                                                           int steps_per_wave) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int split = blockIdx.x, r0 = blockIdx.y * 16, b0 = blockIdx.z * 16;
  const int myid = lora_tile_id(ids, ids_int64, b0, rows, nadapters, lane);
  uint64_t pending = __builtin_amdgcn_ballot_w64(myid >= 0);
  if (!pending) return;  // uniform over the workgroup: every wave reads the same 16 ids

  const int q = lane >> 4, c = lane & 15;
  const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (long)std::min(b0 + c, rows - 1) * xs);
  const int s0 = (split * kSgmvWaves + wave) * steps_per_wave;
  __shared__ float part[kSgmvWaves][4][64];

  while (pending) {
    const int a = __builtin_amdgcn_readlane(myid, (int)__builtin_ctzll(pending));  // the first unserved row's adapter
    const uint64_t match = __builtin_amdgcn_ballot_w64(myid == a);
    pending &= ~match;
    const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + a);
    const int rank = lora_rank(ent->rank, max_rank);
    if (r0 >= rank) continue;  // no adapter at all (rank 0), or a rank tile past this adapter's rank
    const lora_gbl_u32x4_ptr A = (lora_gbl_u32x4_ptr)(uintptr_t)ent->a + (long)std::min(r0 + c, rank - 1) * K8;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < steps_per_wave; s += kSgmvInFlight) {  // kSgmvInFlight k-steps of both operands in flight
      u32x4 xv[kSgmvInFlight], av[kSgmvInFlight];
      bool live[kSgmvInFlight];
#pragma unroll
      for (int u = 0; u < kSgmvInFlight; ++u) {
        const int piece = (s0 + s + u) * 4 + q;
        live[u] = s + u < steps_per_wave && piece < K8;  // past the wave's share, or the tail of K
        const int pc = live[u] ? piece : K8 - 1;  // loads are unconditional from a clamped address; masked at the use
        xv[u] = xrow[pc];
        av[u] = A[pc];
      }
#pragma unroll
      for (int u = 0; u < kSgmvInFlight; ++u) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        acc = mfma16<T>(live[u] ? xv[u] : zero, live[u] ? av[u] : zero, acc);  // D[b = 4 q + reg][r = c]
      }
    }

#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[wave][reg][lane] = acc[reg];
    __syncthreads();
    {
      const int reg = wave;  // thread (reg, lane) owns one element of the 16 x 16 tile
      float v = part[0][reg][lane];
#pragma unroll
      for (int w = 1; w < kSgmvWaves; ++w) v += part[w][reg][lane];  // the shares meet in wave order
      const int row = q * 4 + reg;
      if (((match >> row) & 1) && r0 + c < rank) t[((long)(b0 + row) * splits + split) * max_rank + r0 + c] = v;
    }
    __syncthreads();
  }
}

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_expand_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                           const float* t, uint16_t* y, long ys, int ids_int64,
                                                                           int nadapters, int max_rank, int rows, int M, int splits) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile0 = blockIdx.x * kSgmvSpan, b0 = blockIdx.y * 16;
  const int myid = lora_tile_id(ids, ids_int64, b0, rows, nadapters, lane);
  uint64_t pending = __builtin_amdgcn_ballot_w64(myid >= 0);
  if (!pending) return;

  const int q = lane >> 4, c = lane & 15;
  const float* trow = t + (long)std::min(b0 + c, rows - 1) * splits * max_rank;
  const u32x4 zero = {0u, 0u, 0u, 0u};

  while (pending) {
    const int a = __builtin_amdgcn_readlane(myid, (int)__builtin_ctzll(pending));
    const uint64_t match = __builtin_amdgcn_ballot_w64(myid == a);
    pending &= ~match;
    const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + a);
    const int rank = lora_rank(ent->rank, max_rank);
    if (rank == 0) continue;
    const float scaling = ent->scaling;
    const int pieces = rank >> 3;

    // t[b = c][r = 32 ks + 8 q + j] of the tile, slices added in slice order, as the pair hi + lo of storage-type values
    u32x4 hi[kLoraMaxRank / 32], lo[kLoraMaxRank / 32];
#pragma unroll
    for (int ks = 0; ks < kLoraMaxRank / 32; ++ks) {
      hi[ks] = lo[ks] = zero;
      if (ks * 4 < pieces) {
        const int piece = ks * 4 + q;
        const bool live = piece < pieces;  // rank pieces past rank_a inside a 32-wide k-step: masked
        const float4* p = reinterpret_cast<const float4*>(trow + (live ? piece : 0) * 8);
        float4 v0 = p[0], v1 = p[1];
        for (int s = 1; s < splits; ++s) {
          p = reinterpret_cast<const float4*>(trow + (long)s * max_rank + (live ? piece : 0) * 8);
          const float4 w0 = p[0], w1 = p[1];
          v0.x += w0.x; v0.y += w0.y; v0.z += w0.z; v0.w += w0.w;
          v1.x += w1.x; v1.y += w1.y; v1.z += w1.z; v1.w += w1.w;
        }
        u32x4 h, l;
        h.x = sgmv_hi2<T>(v0.x, v0.y); h.y = sgmv_hi2<T>(v0.z, v0.w); h.z = sgmv_hi2<T>(v1.x, v1.y); h.w = sgmv_hi2<T>(v1.z, v1.w);
        l.x = sgmv_lo2<T>(v0.x, v0.y, h.x); l.y = sgmv_lo2<T>(v0.z, v0.w, h.y);
        l.z = sgmv_lo2<T>(v1.x, v1.y, h.z); l.w = sgmv_lo2<T>(v1.z, v1.w, h.w);
        hi[ks] = live ? h : zero;
        lo[ks] = live ? l : zero;
      }
    }

    const bool mine = (match >> c) & 1;  // row b0 + c belongs to this pass (and exists: rows past `rows` have no id)
    // the wave's kSgmvTilesPerWave neighbouring output tiles: per row b its four 8-byte groups of each tile, 128 bytes of y in all.
    // Tiles past out_features load B_a from its last row and store nothing.
    const int i00 = (tile0 + wave * kSgmvTilesPerWave) * 16;
    if (i00 >= M) continue;
    f32x4 acc[kSgmvTilesPerWave];
#pragma unroll
    for (int j = 0; j < kSgmvTilesPerWave; ++j) {
      const lora_gbl_u32x4_ptr B = (lora_gbl_u32x4_ptr)(uintptr_t)ent->b + (long)std::min(i00 + j * 16 + c, M - 1) * pieces;
      acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kLoraMaxRank / 32; ++ks) {
        if (ks * 4 < pieces) {
          const int piece = ks * 4 + q;
          const bool live = piece < pieces;
          u32x4 bv = B[live ? piece : 0];
          bv = live ? bv : zero;
          acc[j] = mfma16<T>(bv, hi[ks], acc[j]);  // D[i = 4 q + reg][b = c]
          acc[j] = mfma16<T>(bv, lo[ks], acc[j]);
        }
      }
    }
    uint16_t* yrow = y + (long)(b0 + c) * ys + i00 + q * 4;
    u32x2 v[kSgmvTilesPerWave];
#pragma unroll
    for (int j = 0; j < kSgmvTilesPerWave; ++j)
      if (mine && i00 + j * 16 + q * 4 + 4 <= M) v[j] = *reinterpret_cast<const u32x2*>(yrow + j * 16);
#pragma unroll
    for (int j = 0; j < kSgmvTilesPerWave; ++j) {
      const int i = i00 + j * 16 + q * 4;
      uint16_t* yp = yrow + j * 16;
      if (mine && i + 4 <= M) {
        const uint32_t y0 = T::from_float(fmaf(scaling, acc[j][0], T::lo(v[j].x)));
        const uint32_t y1 = T::from_float(fmaf(scaling, acc[j][1], T::hi(v[j].x)));
        const uint32_t y2 = T::from_float(fmaf(scaling, acc[j][2], T::lo(v[j].y)));
        const uint32_t y3 = T::from_float(fmaf(scaling, acc[j][3], T::hi(v[j].y)));
        u32x2 o;
        o.x = y0 | (y1 << 16);
        o.y = y2 | (y3 << 16);
        *reinterpret_cast<u32x2*>(yp) = o;
      } else if (mine && i < M) {  // out_features % 4 != 0: the last group, element by element
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (i + e < M) yp[e] = T::from_float(fmaf(scaling, acc[j][e], T::to_float(yp[e])));
      }
    }
  }
}

template <class T>
static int launch_sgmv(const aqlm_hip_lora_entry* table, int nadapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const uint16_t* x, long xs, uint16_t* y, long ys, int M, int K, float* t, hipStream_t stream) {
  const int K8 = K / 8;
  const int splits = sgmv_splits(K);
  const int steps = (K8 + 3) / 4;  // k-steps of 32
  const int steps_per_wave = (steps + splits * kSgmvWaves - 1) / (splits * kSgmvWaves);
  const int row_tiles = (rows + 15) / 16;
  hipLaunchKernelGGL(lora_sgmv_shrink_kernel<T>, dim3(splits, (max_rank + 15) / 16, row_tiles), dim3(kSgmvWaves * 64), 0, stream,
                     table, ids, x, t, xs, ids_int64, nadapters, max_rank, rows, K8, splits, steps_per_wave);
  if (int e = check_hip(hipGetLastError(), "lora_sgmv_shrink launch")) return e;
  hipLaunchKernelGGL(lora_sgmv_expand_kernel<T>, dim3((M + 16 * kSgmvSpan - 1) / (16 * kSgmvSpan), row_tiles), dim3(kSgmvWaves * 64),
                     0, stream, table, ids, (const float*)t, y, ys, ids_int64, nadapters, max_rank, rows, M, splits);
  return check_hip(hipGetLastError(), "lora_sgmv_expand launch");
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_sgmv_workspace_bytes(int rows, int max_rank, int in_features) {
  if (!lora_shape_ok(1, in_features, max_rank, rows, AQLM_HIP_MAX_LORA_SGMV_ROWS)) return 0;
  return (size_t)rows * (size_t)sgmv_splits(in_features) * (size_t)max_rank * 4;
}

extern "C" int aqlm_hip_lora_sgmv_supported(int out_features, int in_features, int max_rank, int rows) {
  return lora_shape_ok(out_features, in_features, max_rank, rows, AQLM_HIP_MAX_LORA_SGMV_ROWS) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_sgmv(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids, int ids_int64,
                                  int rows, const void* x, long x_row_stride, void* y, long y_row_stride, int out_features,
                                  int in_features, int dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_sgmv";
  if (int e = lora_check_args(who, table, num_adapters, max_rank, ids, ids_int64, rows, x, x_row_stride, y, y_row_stride, out_features,
                              in_features, dtype, workspace, AQLM_HIP_MAX_LORA_SGMV_ROWS))
    return e;
  if ((reinterpret_cast<uintptr_t>(y) & 7u) || (rows > 1 && y_row_stride % 4 != 0)) {
    set_last_error("%s: y rows not 8-byte aligned (y %p, stride %ld elements): the expand writes groups of 4 outputs", who, y,
                   y_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = lora_check_workspace(who, workspace_bytes, aqlm_hip_lora_sgmv_workspace_bytes(rows, max_rank, in_features))) return e;
  auto go = [&](auto t) {
    return launch_sgmv<decltype(t)>(table, num_adapters, max_rank, ids, ids_int64 ? 1 : 0, rows, (const uint16_t*)x, x_row_stride,
                                    (uint16_t*)y, y_row_stride, out_features, in_features, (float*)workspace, (hipStream_t)stream_);
  };
  return dtype == AQLM_HIP_F16 ? go(F16{}) : go(BF16{});
}

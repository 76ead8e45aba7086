// The tile arithmetic of the segmented LoRA adapter GEMM, shared by aqlm_hip_lora_sgmv (lora_sgmv.hip: a tile is 16 consecutive
// rows of the batch) and aqlm_hip_lora_sgmv_routed (lora_sgmv_routed.hip: a tile is a slot of the expert bucket, up to 16
// (token, expert) pairs of one expert gathered through the pair list).  A kernel finds, per lane, the x row, the t row and the
// y row of the tile row the lane works on and that row's adapter id, and hands them to these bodies, so both launches run the
// same operations in the same order: a row's bits are the same whichever of the two computed it.  lora_sgmv.hip describes the
// arithmetic, the passes and the operand layout.
//
// The adapter id `a` of a pass selects the entry table[a * entry_stride]: the dense launch passes its table and stride 1, the
// routed launch the entry of (adapter 0, the tile's expert, the segment) and the stride of an adapter, num_experts x num_segments.
// Every call of a workgroup is uniform: all waves get the same 16 ids (the shrink body holds barriers).
#pragma once
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

// k-steps of 32 per shrink wave: a function of in_features alone
static inline int sgmv_steps_per_wave(int K) {
  const int steps = (K / 8 + 3) / 4;
  const int splits = sgmv_splits(K);
  return (steps + splits * kSgmvWaves - 1) / (splits * kSgmvWaves);
}

template <class T>
__device__ __forceinline__ uint32_t sgmv_hi2(float a, float b) {
  return (uint32_t)T::from_float(a) | ((uint32_t)T::from_float(b) << 16);
}
template <class T>
__device__ __forceinline__ uint32_t sgmv_lo2(float a, float b, uint32_t hi) {
  return sgmv_hi2<T>(a - T::lo(hi), b - T::hi(hi));
}

// Slice `split` of t[.., r0 .. r0 + 16) of one tile.  myid: lanes 0..15 the adapter id of tile row `lane`, or -1 when the row
// does not exist or has no adapter; lanes 16..63: -1.  xrow: the x row of tile row lane & 15 (a row that does not exist: any
// readable row).  trow: the workspace row [splits][max_rank] of tile row (lane >> 4) * 4 + wave, the element this thread owns
// after the LDS sum (dereferenced only when that row belongs to the pass).
template <class T>
__device__ __forceinline__ void lora_sgmv_shrink_body(const aqlm_hip_lora_entry* table, long entry_stride, int myid,
                                                      const u32x4* xrow, float* trow, int split, int r0, int max_rank, int K8,
                                                      int steps_per_wave) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint64_t pending = __builtin_amdgcn_ballot_w64(myid >= 0);
  if (!pending) return;  // uniform over the workgroup: every wave holds the same 16 ids

  const int q = lane >> 4, c = lane & 15;
  const int s0 = (split * kSgmvWaves + wave) * steps_per_wave;
  __shared__ float part[kSgmvWaves][4][64];

  while (pending) {
    const int a = __builtin_amdgcn_readlane(myid, (int)__builtin_ctzll(pending));  // the first unserved row's adapter
    const uint64_t match = __builtin_amdgcn_ballot_w64(myid == a);
    pending &= ~match;
    const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + (long)a * entry_stride);
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
      if (((match >> row) & 1) && r0 + c < rank) trow[(long)split * max_rank + r0 + c] = v;
    }
    __syncthreads();
  }
}

// Outputs [tile0 * 16, (tile0 + kSgmvSpan) * 16) of one tile's y rows.  myid as for the shrink; trow: the workspace row of tile
// row lane & 15 (a row that does not exist: any readable row); yrow: the y row of tile row lane & 15 (dereferenced only when
// that row belongs to the pass).
template <class T>
__device__ __forceinline__ void lora_sgmv_expand_body(const aqlm_hip_lora_entry* table, long entry_stride, int myid,
                                                      const float* trow, uint16_t* yrow, int tile0, int max_rank, int M,
                                                      int splits) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint64_t pending = __builtin_amdgcn_ballot_w64(myid >= 0);
  if (!pending) return;

  const int q = lane >> 4, c = lane & 15;
  const u32x4 zero = {0u, 0u, 0u, 0u};

  while (pending) {
    const int a = __builtin_amdgcn_readlane(myid, (int)__builtin_ctzll(pending));
    const uint64_t match = __builtin_amdgcn_ballot_w64(myid == a);
    pending &= ~match;
    const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + (long)a * entry_stride);
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

    const bool mine = (match >> c) & 1;  // tile row c belongs to this pass (and exists: rows that do not exist have no id)
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
    uint16_t* yq = yrow + i00 + q * 4;
    u32x2 v[kSgmvTilesPerWave];
#pragma unroll
    for (int j = 0; j < kSgmvTilesPerWave; ++j)
      if (mine && i00 + j * 16 + q * 4 + 4 <= M) v[j] = *reinterpret_cast<const u32x2*>(yq + j * 16);
#pragma unroll
    for (int j = 0; j < kSgmvTilesPerWave; ++j) {
      const int i = i00 + j * 16 + q * 4;
      uint16_t* yp = yq + j * 16;
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

}  // namespace aqlm

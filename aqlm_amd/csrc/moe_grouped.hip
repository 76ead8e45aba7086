// Expert-grouped 1x16 GEMM of a mixture-of-experts block (Mixtral prefill, batched decode, training), gfx950.
//
// Two launches serve one projection layer of the block -- or two layers that read the same rows (w1 and w3) -- for any
// number of (token, expert) pairs, without the expert ids ever reaching the host:
//   * moe_bucket_kernel (ONE workgroup): an LDS histogram of the ids, a prefix sum and a stable scatter put each expert's
//     pairs in ascending pair order and cut them into tiles of <= tile_pairs pairs.  One workgroup: no inter-workgroup
//     communication (the XCDs do not share an L2);
//   * gemm_1x16_grouped_kernel: the 16-row fused MFMA GEMM (gemm_rows16_body.h) on a grid of row blocks x tile slots x
//     segments that depends on the shapes only, so a captured hipGraph stays valid for any routing.  A block reads its tile
//     (expert, first, count), takes W from the routed table entry of that expert and gathers the tile's X rows through the
//     pair list; a slot past the tile count exits after reading one word.
// Per pair the code walk, the MFMA order and the epilogue are the rows16 kernel's: each expert's rows are bit-identical to
// aqlm_hip_gemm_1x16_mfma on that expert's rows wherever that op runs the 16-row kernel, and no pair's bits depend on the
// other pairs (an MFMA output column depends on its own B column only; the tile size changes the number of columns, never
// their k order).
#include "gemm_rows16.h"
#include "moe_bucket.h"

namespace aqlm {

constexpr int kBucketThreads = 1024;
constexpr int kBucketWaves = kBucketThreads / 64;

__device__ __forceinline__ int bucket_of(const void* ids, int ids_int64, int p, int nexp) {
  const long id = ids_int64 ? reinterpret_cast<const long*>(ids)[p] : (long)reinterpret_cast<const int*>(ids)[p];
  return id >= 0 && id < (long)nexp ? (int)id : nexp;  // ids are compared, never used to form an address
}

__global__ __launch_bounds__(kBucketThreads) void moe_bucket_kernel(const void* ids, int ids_int64, int npairs, int nexp,
                                                                    int tile_pairs, int max_tiles, int* bucket) {
  constexpr int NB = AQLM_HIP_MAX_ROUTED_EXPERTS + 1;  // experts + the bucket of out-of-range ids
  __shared__ int hist[NB], cursor[NB], tile0[NB];
  __shared__ int wcnt[kBucketWaves][NB];  // pairs of bucket b in wave w's share of the current round
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = nexp + 1;
  int4* tiles = bucket_tiles(bucket);
  int* list = bucket_list(bucket, max_tiles);

  for (int b = tid; b < nb; b += kBucketThreads) hist[b] = 0;
  __syncthreads();
  for (int p = tid; p < npairs; p += kBucketThreads) atomicAdd(&hist[bucket_of(ids, ids_int64, p, nexp)], 1);
  __syncthreads();
  if (wave == 0) {  // exclusive scans of the pair counts and the tile counts: lane l owns buckets [l C, l C + C)
    const int C = (nb + 63) / 64;
    int sp = 0, st = 0;
    for (int j = 0; j < C; ++j) {
      const int b = lane * C + j;
      if (b < nb) {
        sp += hist[b];
        if (b < nexp) st += (hist[b] + tile_pairs - 1) / tile_pairs;
      }
    }
    int ip = sp, it = st;  // inclusive scans over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(ip, d), ut = __shfl_up(it, d);
      if (lane >= d) {
        ip += up;
        it += ut;
      }
    }
    int op = ip - sp, ot = it - st;
    for (int j = 0; j < C; ++j) {
      const int b = lane * C + j;
      if (b < nb) {
        cursor[b] = op;
        tile0[b] = ot;
        op += hist[b];
        if (b < nexp) ot += (hist[b] + tile_pairs - 1) / tile_pairs;
      }
    }
    if (lane == 63) {
      bucket[0] = it;  // tiles (the last lane's inclusive scan covers every expert)
      bucket[1] = hist[nexp];
      bucket[2] = npairs - hist[nexp];
      bucket[3] = 0;
    }
  }
  __syncthreads();
  for (int e = tid; e < nexp; e += kBucketThreads) {
    const int n = hist[e];
    for (int j = 0; j * tile_pairs < n; ++j)
      tiles[tile0[e] + j] = int4{e, cursor[e] + j * tile_pairs, std::min(tile_pairs, n - j * tile_pairs), 0};
  }
  // stable scatter, 1024 pairs per round: rank inside the wave by ballots over the buckets present in it, then the counts of
  // the lower waves of the round, then the bucket's cursor
  for (int r0 = 0; r0 < npairs; r0 += kBucketThreads) {
    __syncthreads();  // (first round: the tile table above is done with the cursors)
    for (int i = tid; i < kBucketWaves * nb; i += kBucketThreads) wcnt[i / nb][i % nb] = 0;
    __syncthreads();
    const int p = r0 + tid;
    const bool live = p < npairs;
    const int b = live ? bucket_of(ids, ids_int64, p, nexp) : -1;
    int rank = 0;
    uint64_t rest = __builtin_amdgcn_ballot_w64(live);
    while (rest) {
      const int leader = __builtin_ctzll(rest);
      const int bb = __builtin_amdgcn_readlane(b, leader);
      const uint64_t m = __builtin_amdgcn_ballot_w64(live && b == bb);
      if (live && b == bb) rank = __builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (lane == leader) wcnt[wave][bb] = __builtin_popcountll(m);
      rest &= ~m;
    }
    __syncthreads();
    if (live) {
      int pos = cursor[b] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][b];
      list[pos] = p;
    }
    __syncthreads();
    for (int bb = tid; bb < nb; bb += kBucketThreads) {
      int s = 0;
      for (int w = 0; w < kBucketWaves; ++w) s += wcnt[w][bb];
      cursor[bb] += s;
    }
  }
}

struct GroupedArgs {
  const aqlm_hip_routed_entry* table;  // device, [nexp][nseg]
  const int* bucket;                   // from moe_bucket_kernel
  const uint16_t* x;
  uint16_t* y;                         // [npairs][nseg][M]
  long xs;
  int nexp, nseg, npairs, top_k, x_per_pair, tile_pairs, max_tiles;
  int M, in_groups, nsteps;
};

template <class T, int G, int NBT, int CPB>
__global__ __launch_bounds__((R16Lds<NBT, CPB>::WAVES * 64)) void gemm_1x16_grouped_kernel(const GroupedArgs a) {
  const int slot = blockIdx.y, s = blockIdx.z;
  const long ys = (long)a.nseg * a.M;  // pair stride of y
  const int* list = bucket_list(a.bucket, a.max_tiles);
  if (slot == 0) {  // the pairs of out-of-range ids get zero rows
    int nbad;
    const int* bad = bucket_bad_pairs(a.bucket, list, a.npairs, nbad);
    for (int i = threadIdx.x; i < nbad * 16; i += blockDim.x) {
      const int pr = bad[i >> 4];
      if ((unsigned)pr < (unsigned)a.npairs) a.y[(long)pr * ys + (long)s * a.M + blockIdx.x * 16 + (i & 15)] = 0;
    }
  }
  if (slot >= a.bucket[0]) return;
  const int4 tile = bucket_tile(a.bucket, slot);
  const int e = tile.x, first = tile.y, count = tile.z;
  if (e < 0 || e >= a.nexp || count < 1 || count > a.tile_pairs || first < 0 || first > a.npairs - count) return;  // (a foreign bucket)
  const aqlm_hip_routed_entry ent = a.table[e * a.nseg + s];
  const int* pairs = list + first;
  R16Params p{};
  p.codes = reinterpret_cast<const uint8_t*>(ent.codes);
  p.codebook = reinterpret_cast<const uint8_t*>(ent.codebook);
  p.scales = reinterpret_cast<const uint16_t*>(ent.scales);
  p.bias = reinterpret_cast<const uint16_t*>(ent.bias);
  p.X = a.x;
  p.Y = a.y + (long)s * a.M;
  p.xs = a.xs;
  p.ys = ys;
  p.M = a.M;
  p.B = count;
  p.in_groups = a.in_groups;
  p.nsteps = a.nsteps;
  // pair of batch row b (rows past the tile: its last pair, computed and never stored); any value outside [0, npairs) -> 0
  auto pair_at = [&](int b) {
    const int pr = pairs[b < count ? b : count - 1];
    return (unsigned)pr < (unsigned)a.npairs ? pr : 0;
  };
#define R16_ROW0 ((int)blockIdx.x * 16)
#define R16_X_ROW(b) (a.x_per_pair ? pair_at(b) : pair_at(b) / a.top_k)
#define R16_Y_ROW(b) (pair_at(b))
#include "gemm_rows16_body.h"
}

template <class T, int G>
static int launch_grouped(const GroupedArgs& a, const R16Plan& r, dim3 grid, hipStream_t stream) {
  auto go = [&](auto kern, size_t lds, int waves) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(waves * 64), lds, stream, a);
    return check_hip(hipGetLastError(), "gemm_1x16_grouped launch");
  };
#define AQLM_GR_CASE(NBT_, CPB_) return go(gemm_1x16_grouped_kernel<T, G, NBT_, CPB_>, R16Lds<NBT_, CPB_>::TOTAL, R16Lds<NBT_, CPB_>::WAVES)
  if (r.cpb == 1) {
    switch (r.nbt) {
      case 1: AQLM_GR_CASE(1, 1);
      case 2: AQLM_GR_CASE(2, 1);
      case 4: AQLM_GR_CASE(4, 1);
      default: AQLM_GR_CASE(8, 1);
    }
  }
  switch (r.nbt) {
    case 1: AQLM_GR_CASE(1, 4);
    case 2: AQLM_GR_CASE(2, 4);
    case 4: AQLM_GR_CASE(4, 2);
    default: AQLM_GR_CASE(8, 2);
  }
#undef AQLM_GR_CASE
}

static bool grouped_supported(int M, int K, int g) {
  if (M <= 0 || K <= 0 || M % 16 != 0 || (g != 8 && g != 16) || K % g != 0) return false;
  R16Plan r;
  for (int t = kTilePairsMin; t <= kTilePairsMax; t *= 2)
    if (!plan_rows16(t, K, g, r)) return false;
  return true;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_moe_bucket_bytes(int num_pairs, int num_experts, int tile_pairs) {
  if (num_pairs < 1 || num_pairs > AQLM_HIP_MAX_GROUPED_PAIRS || num_experts < 1 || num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS ||
      !tile_pairs_ok(tile_pairs))
    return 0;
  return (bucket_words(num_pairs, num_experts, tile_pairs) * 4 + 15) / 16 * 16;
}

extern "C" int aqlm_hip_moe_bucket(const void* expert_ids, int ids_int64, int num_pairs, int num_experts, int tile_pairs,
                                   void* bucket, void* stream) {
  static const char* who = "aqlm_hip_moe_bucket";
  if (int e = check_not_null(who, expert_ids && bucket)) return e;
  if (int e = check_aligned(who, "expert_ids / bucket", ids_aligned(expert_ids, ids_int64) && aligned16(bucket))) return e;
  if (num_pairs < 1 || num_pairs > AQLM_HIP_MAX_GROUPED_PAIRS || num_experts < 1 || num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS ||
      !tile_pairs_ok(tile_pairs)) {
    set_last_error("%s: %d pairs, %d experts, tiles of %d (1..%d pairs, 1..%d experts, tiles of 16 / 32 / 64 / 128)", who, num_pairs,
                   num_experts, tile_pairs, AQLM_HIP_MAX_GROUPED_PAIRS, AQLM_HIP_MAX_ROUTED_EXPERTS);
    return AQLM_HIP_E_INVALID;
  }
  hipLaunchKernelGGL(moe_bucket_kernel, dim3(1), dim3(kBucketThreads), 0, (hipStream_t)stream, expert_ids, ids_int64 ? 1 : 0,
                     num_pairs, num_experts, tile_pairs, bucket_max_tiles(num_pairs, num_experts, tile_pairs), (int*)bucket);
  return check_hip(hipGetLastError(), "moe_bucket launch");
}

extern "C" int aqlm_hip_gemm_1x16_grouped_supported(int out_features, int in_features, int in_group_size) {
  return grouped_supported(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_gemm_1x16_grouped(const aqlm_hip_routed_entry* table, int num_experts, int num_segments, const void* bucket,
                                          int tile_pairs, int num_pairs, int top_k, const void* x, long x_row_stride, int x_per_pair,
                                          void* y, int out_features, int in_features, int in_group_size, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_gemm_1x16_grouped";
  if (int e = check_not_null(who, table && bucket && x && y)) return e;
  if (int e = check_aligned(who, "table / bucket", aligned8(table) && aligned16(bucket))) return e;
  if (int e = check_experts(who, num_experts, num_segments)) return e;
  if (num_pairs < 1 || num_pairs > AQLM_HIP_MAX_GROUPED_PAIRS || top_k < 1 || num_pairs % top_k != 0 || !tile_pairs_ok(tile_pairs)) {
    set_last_error("%s: %d pairs with top_k %d, tiles of %d (1..%d pairs, a multiple of top_k; tiles of 16 / 32 / 64 / 128)", who,
                   num_pairs, top_k, tile_pairs, AQLM_HIP_MAX_GROUPED_PAIRS);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_group_size(who, in_group_size)) return e;
  R16Plan r;
  if (!grouped_supported(out_features, in_features, in_group_size) || !plan_rows16(tile_pairs, in_features, in_group_size, r) ||
      !aligned16(x) || x_row_stride % 8 != 0) {
    set_last_error("%s: shape outside the 16-row kernel (out=%d in=%d g=%d, x stride %ld)", who, out_features, in_features,
                   in_group_size, x_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  GroupedArgs a{};
  a.table = table;
  a.bucket = (const int*)bucket;
  a.x = (const uint16_t*)x;
  a.y = (uint16_t*)y;
  a.xs = x_row_stride;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.npairs = num_pairs;
  a.top_k = top_k;
  a.x_per_pair = x_per_pair ? 1 : 0;
  a.tile_pairs = tile_pairs;
  a.max_tiles = bucket_max_tiles(num_pairs, num_experts, tile_pairs);
  a.M = out_features;
  a.in_groups = in_features / in_group_size;
  a.nsteps = r.nsteps;
  const dim3 grid((unsigned)(out_features / 16), (unsigned)a.max_tiles, (unsigned)num_segments);
  hipStream_t stream = (hipStream_t)stream_;
  return dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) {
    return launch_grouped<decltype(t), decltype(g)::value>(a, r, grid, stream);
  });
}

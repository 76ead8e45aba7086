// The bucket of the expert-grouped launches: the one statement of its layout.  moe_bucket_kernel (moe_grouped.hip) writes it; the
// grouped GEMM (moe_grouped.hip), its transposed product (moe_grouped_bwd.hip) and the routed segmented adapter GEMM
// (lora_sgmv_routed.hip, tiles of 16) read it through the accessors below.
//
// int32 words: [0] tiles, [1] pairs with an id outside [0, E), [2] pairs with a valid id, [3] 0;
// then max_tiles x {expert, first, count, 0}; then the pair list [num_pairs]: the valid pairs by expert, in ascending pair
// order inside an expert, then the pairs with an out-of-range id.  A tile is `count` <= tile_pairs entries of the list from
// `first`, all of one expert.
#pragma once
#include <algorithm>

#include "aqlm_common.h"

namespace aqlm {

constexpr int kBucketHeader = 4;

// tile slots of a bucket (and of the grids that read it): a bound that depends on the sizes only, never on the routing
inline int bucket_max_tiles(int num_pairs, int num_experts, int tile_pairs) {
  return (num_pairs + tile_pairs - 1) / tile_pairs + std::min(num_experts, num_pairs);
}

// int32 words of a bucket
inline size_t bucket_words(int num_pairs, int num_experts, int tile_pairs) {
  return kBucketHeader + 4 * (size_t)bucket_max_tiles(num_pairs, num_experts, tile_pairs) + (size_t)num_pairs;
}

// pairs per tile: 16, 32, 64 or 128 (the caller's choice; the readers instantiate one kernel per size)
constexpr int kTilePairsMin = 16, kTilePairsMax = 128;
inline bool tile_pairs_ok(int t) { return t >= kTilePairsMin && t <= kTilePairsMax && (t & (t - 1)) == 0; }

// the tile table and the pair list (writer and readers)
__device__ __forceinline__ int4* bucket_tiles(int* bucket) { return reinterpret_cast<int4*>(bucket + kBucketHeader); }
__device__ __forceinline__ const int4* bucket_tiles(const int* bucket) { return reinterpret_cast<const int4*>(bucket + kBucketHeader); }
__device__ __forceinline__ int* bucket_list(int* bucket, int max_tiles) { return bucket + kBucketHeader + 4 * max_tiles; }
__device__ __forceinline__ const int* bucket_list(const int* bucket, int max_tiles) { return bucket + kBucketHeader + 4 * max_tiles; }

// the pairs with an out-of-range id, the tail of the list: the blocks of slot 0 (which every grid has) give them zero rows.  An
// entry is a pair only if it lies in [0, num_pairs): the reader checks that before it forms an address.
__device__ __forceinline__ const int* bucket_bad_pairs(const int* bucket, const int* list, int npairs, int& nbad) {
  nbad = std::min(bucket[1], npairs);
  return list + (npairs - nbad);
}

// Tile record of a slot, for a reader that has checked slot < bucket[0] (a slot past the tile count exits after that one word).
// The reader then drops a record that no bucket of its sizes holds (a foreign bucket): e outside [0, nexp), count outside
// [1, the largest tile it takes], first outside [0, npairs - count].  That chain of early returns stays in the kernels: as a
// function that returns a flag it compiles to other branches.
__device__ __forceinline__ int4 bucket_tile(const int* bucket, int slot) { return bucket_tiles(bucket)[slot]; }

}  // namespace aqlm

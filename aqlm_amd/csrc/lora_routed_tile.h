// What the kernels that walk the 16-pair expert bucket on behalf of the routed adapters share (lora_sgmv_routed.hip: the segmented
// adapter GEMM; lora_routed_bwd.hip: the adapter gradient reduction): the arguments that describe the ids and the bucket, and how a
// wave reads the pairs of one tile and their adapter ids -- every list entry and both ids checked before they form an address.
#pragma once
#include "lora_common.h"
#include "moe_bucket.h"

namespace aqlm {

constexpr int kRoutedSgmvTile = 16;  // pairs per bucket tile: the rows of one MFMA

struct RoutedSgmvArgs {
  const aqlm_hip_lora_entry* table;  // [nadapters][nexp][nseg]
  const void* adapter_ids;           // one per TOKEN, or NULL: adapter 0
  const void* expert_ids;            // one per pair
  const int* bucket;                 // from moe_bucket_kernel, tiles of kRoutedSgmvTile pairs
  const uint16_t* x;
  float* t;                          // [npairs][nseg][splits][max_rank]
  uint16_t* y;                       // [npairs][nseg][M]
  long xs;
  int adapter_ids_int64, expert_ids_int64, nadapters, nexp, nseg, npairs, top_k, x_per_pair, max_tiles;
  int max_rank, K8, splits, steps_per_wave, M;
};

// The pair of tile row lane & 15 (rows past the tile: its last pair, computed and never stored) and, with valid = false, the
// news that some entry of the tile's list is no pair: uniform over the workgroup, every wave reads the same 16 entries.
__device__ __forceinline__ int routed_sgmv_pair(const RoutedSgmvArgs& a, const int* pairs, int count, bool& valid) {
  const int pr = pairs[std::min((int)(threadIdx.x & 15), count - 1)];
  valid = __builtin_amdgcn_ballot_w64((unsigned)pr >= (unsigned)a.npairs) == 0;
  return pr;
}

// lanes 0..15: the adapter id of the tile's pair `lane`, or -1 when the tile has no such pair, the pair was routed to another
// expert than the tile's or its token names no adapter; lanes 16..63: -1.  `pr` is the lane's pair, checked to lie in [0, npairs).
__device__ __forceinline__ int routed_sgmv_id(const RoutedSgmvArgs& a, int pr, int e, int count) {
  const int lane = threadIdx.x & 63;
  if (lane >= count) return -1;  // count <= 16
  if (lora_row_id<int>(a.expert_ids, a.expert_ids_int64, pr, a.nexp) != e) return -1;
  return lora_row_id<int>(a.adapter_ids, a.adapter_ids_int64, pr / a.top_k, a.nadapters);
}

}  // namespace aqlm

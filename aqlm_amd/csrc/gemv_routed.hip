// Expert-routed 1x16 matvec of a mixture-of-experts block (Mixtral decode), gfx950, wave64.
//
// One launch computes every (token, expert) pair of one projection layer of the block -- or of two layers that read the
// same rows (w1 and w3) -- without the expert ids ever reaching the host:
//   * grid = row blocks x segments x experts, fixed by the shapes, so a captured hipGraph stays valid for any routing;
//   * every wave reads the <= 64 ids itself and ballots `id == its workgroup's expert`: ids are compared, never used to
//     form an address, so any id array is safe (out-of-range ids match no expert; expert 0's workgroups write their rows
//     of such pairs as zeros);
//   * a workgroup whose expert has no pair exits before touching anything else;
//   * the pairs of the expert run through gemv_body (gemv_body.h) in its gathered-row form, NBMAX pairs per pass:
//     the same code walk, the same summation order and the same epilogue as aqlm_hip_gemv_1x16, hence bit-identical rows.
#include <algorithm>

#include "aqlm_common.h"
#include "gemv_body.h"

namespace aqlm {

struct RoutedArgs {
  const aqlm_hip_routed_entry* table;  // device, [nexp][nseg]
  const void* ids;                     // device, [npairs] int64 or int32
  const uint16_t* x;
  uint16_t* y;                         // [npairs][nseg][M]
  long xs;
  int ids_int64, npairs, top_k, x_per_pair, nexp, nseg;
  int M, in_groups, nunits, iters, pitch, rpw, prefetch, cb_bytes;
};

constexpr int kRoutedWaves = 4;

// NBMAX: pairs per pass (chosen on the host from the token count and the x-tile budget, never from the routing); a pass
// with fewer pairs pads its slots with the last pair's x row and writes nothing for them
template <class T, int G, int NBMAX>
__global__ __launch_bounds__(kRoutedWaves * 64) void gemv_1x16_routed_kernel(const RoutedArgs a) {
  const int e = blockIdx.z, s = blockIdx.y, block = blockIdx.x;
  const int lane = threadIdx.x & 63;
  long id = -1;
  if (lane < a.npairs) id = a.ids_int64 ? reinterpret_cast<const long*>(a.ids)[lane] : (long)reinterpret_cast<const int*>(a.ids)[lane];
  const bool live = lane < a.npairs;
  uint64_t mine = __builtin_amdgcn_ballot_w64(live && id == (long)e);
  const uint64_t orphans = e == 0 ? __builtin_amdgcn_ballot_w64(live && (id < 0 || id >= (long)a.nexp)) : 0;
  if (!mine && !orphans) return;  // wave-uniform and identical in every wave of the workgroup

  const long ys = (long)a.nseg * a.M;  // pair stride of y
  if (orphans) {
    const int row0 = (block * kRoutedWaves + (int)(threadIdx.x >> 6)) * a.rpw;
    const int nrows = std::min(a.rpw, a.M - row0);  // rpw <= 64: one store per lane
    for (uint64_t m = orphans; m; m &= m - 1) {
      const int pr = __builtin_ctzll(m);
      if (lane < nrows) a.y[(long)pr * ys + (long)s * a.M + row0 + lane] = 0;
    }
  }
  if (!mine) return;

  const aqlm_hip_routed_entry ent = a.table[e * a.nseg + s];
  GemvParams p;
  p.codes = reinterpret_cast<const uint8_t*>(ent.codes);
  p.codebooks = reinterpret_cast<const uint8_t*>(ent.codebook);
  p.scales = reinterpret_cast<const uint16_t*>(ent.scales);
  p.bias = reinterpret_cast<const uint16_t*>(ent.bias);
  p.x = a.x;
  p.y = a.y + (long)s * a.M;
  p.M = a.M;
  p.in_groups = a.in_groups;
  p.nunits = a.nunits;
  p.iters = a.iters;
  p.pitch = a.pitch;
  p.rpw = a.rpw;
  p.prefetch = a.prefetch;
  p.cb_bytes = a.cb_bytes;
  p.xs = a.xs;
  p.ys = ys;
  p.code_row_bytes = (long)a.in_groups * 2;

  bool first = true;
  while (mine) {
    GemvGather g;
    int xr = 0;
    for (int k = 0; k < NBMAX && mine; ++k) {
      const int pr = __builtin_ctzll(mine);
      mine &= mine - 1;
      xr = a.x_per_pair ? pr : pr / a.top_k;
      g.xrows |= (uint64_t)xr << (6 * k);
      g.yrows |= (uint64_t)pr << (6 * k);
      g.nvalid = k + 1;
    }
    for (int k = g.nvalid; k < NBMAX; ++k) g.xrows |= (uint64_t)xr << (6 * k);  // padding slots read the last valid row
    if (!first) __syncthreads();  // the previous pass's waves are done with the x tile
    first = false;
    // one body per kernel: a second instance in the same kernel (to run a short pass at a smaller NB) costs 30-90 VGPRs,
    // i.e. one or two waves per SIMD, more than the padding slots cost
    gemv_body<T, 2, 1, G, 8, NBMAX, false, kRoutedWaves, AUX_DEFAULT, true>(p, block, g);
  }
}

static constexpr size_t kRoutedMaxXTileBytes = 64 * 1024;

template <class T, int G, int NBMAX>
static int launch_routed(const RoutedArgs& a, dim3 grid, hipStream_t stream) {
  constexpr int P = G / 8;
  auto kern = gemv_1x16_routed_kernel<T, G, NBMAX>;
  const size_t lds = (size_t)NBMAX * 8 * P * a.pitch * 16;
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
  hipLaunchKernelGGL(kern, grid, dim3(kRoutedWaves * 64), lds, stream, a);
  return check_hip(hipGetLastError(), "gemv_1x16_routed launch");
}

template <class T, int G>
static int dispatch_routed(int nbmax, const RoutedArgs& a, dim3 grid, hipStream_t s) {
  switch (nbmax) {
    case 1: return launch_routed<T, G, 1>(a, grid, s);
    case 2: return launch_routed<T, G, 2>(a, grid, s);
    case 4: return launch_routed<T, G, 4>(a, grid, s);
    default: return launch_routed<T, G, 8>(a, grid, s);
  }
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_gemv_1x16_routed(const aqlm_hip_routed_entry* table, int num_experts, int num_segments,
                                         const void* expert_ids, int ids_int64, int num_pairs, int top_k, const void* x,
                                         long x_row_stride, int x_per_pair, void* y, int out_features, int in_features,
                                         int in_group_size, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_gemv_1x16_routed";
  if (int e = check_not_null(who, table && expert_ids && x && y)) return e;
  if (int e = check_aligned(who, "table / expert_ids", aligned8(table) && ids_aligned(expert_ids, ids_int64))) return e;
  if (int e = check_experts(who, num_experts, num_segments)) return e;
  if (int e = check_pairs(who, num_pairs, top_k, AQLM_HIP_MAX_ROUTED_PAIRS)) return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_group_size(who, in_group_size)) return e;
  const int in_groups = in_features / in_group_size;
  const size_t x_row_bytes = (size_t)in_features * 2;
  if (in_groups % 8 != 0 || !aligned16(x) || x_row_stride % 8 != 0 || x_row_bytes > kRoutedMaxXTileBytes ||
      tuning().force_generic) {
    set_last_error("%s: shape outside the direct kernel (in=%d g=%d, x stride %ld)", who, in_features, in_group_size,
                   x_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  // pairs per pass: the token count rounded up to a power of two (<= 8), halved while the x tile does not fit.  A router's
  // top-k experts of one token are distinct, so no expert sees more pairs than there are tokens; any other id array is
  // still exact, in more passes
  int nbmax = 1;
  while (nbmax < std::min(num_pairs / top_k, AQLM_HIP_MAX_GEMV_BATCH)) nbmax *= 2;
  while (nbmax > 1 && (size_t)nbmax * x_row_bytes > kRoutedMaxXTileBytes) nbmax /= 2;

  RoutedArgs a{};
  a.table = table;
  a.ids = expert_ids;
  a.x = (const uint16_t*)x;
  a.y = (uint16_t*)y;
  a.xs = x_row_stride;
  a.ids_int64 = ids_int64 ? 1 : 0;
  a.npairs = num_pairs;
  a.top_k = top_k;
  a.x_per_pair = x_per_pair ? 1 : 0;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.M = out_features;
  a.in_groups = in_groups;
  a.nunits = in_groups / 8;
  a.iters = (a.nunits + 63) / 64;
  a.pitch = a.nunits | 1;
  a.prefetch = tuning().gemv1x16_prefetch_cb;
  a.cb_bytes = 65536 * in_group_size * 2;
  // most workgroups of a decode step find no pair and exit: a few rows per wave keep their number near 512 per
  // (expert, segment) instead of one per 4 rows
  int rpw = tuning().gemv_rows_per_wave;
  if (rpw <= 0) rpw = (out_features + kRoutedWaves * 512 - 1) / (kRoutedWaves * 512);
  a.rpw = std::max(1, std::min(rpw, 64));
  const int rows_per_block = kRoutedWaves * a.rpw;
  const dim3 grid((out_features + rows_per_block - 1) / rows_per_block, num_segments, num_experts);
  hipStream_t stream = (hipStream_t)stream_;
  return dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) {
    return dispatch_routed<decltype(t), decltype(g)::value>(nbmax, a, grid, stream);
  });
}

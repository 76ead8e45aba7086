// The V step of PV-tuning for the K x 8 schemes (1 to 8 codebooks of 256 entries, out_group_size 1, g = 8 / 16 / 32): the reference's
// `_beam_search_update_codes_groupwise` for every group of one layer, without its [groups, beams, 256] score tensor
// (aqlm_hip_code_search_kx8; include/aqlm_hip.h has the definition, DESIGN.md 4.8n the mapping and the numbers).  The entry is held
// to ITS OWN ARITHMETIC bit for bit (tests/kx8_search_model.py restates it in numpy): every product and every sum of the scoring
// code is one IEEE fp32 operation, so this translation unit switches contraction off -- the library's -ffp-contract=fast must not
// fuse a product into the sum that follows it.
//
//   work       one wave (a workgroup of 64 threads) per group, grid-stride over the groups of the call; lane l owns the candidates
//              s = 4 l .. 4 l + 3 of the step's codebook: their 4 g elements are widened into registers once per step (one
//              contiguous 8 g bytes per lane) and serve every beam position; |C_s|^2 comes from the same registers.
//   residues   res[position][g] in LDS, read as wave-uniform broadcasts; lane b forms |res[b]|^2.
//   scores     S(b, s) = (rn[b] - 2 dot) + cn: 4 * positions values per lane, kept in registers as order-preserving unsigned
//              integers (a score is never -0: cn is a sum of squares, so +0 or above).
//   selection  kx8_select_body.h, which this kernel shares with the calibrated search: the best `keep` 64-bit keys (score bits,
//              b * 256 + s) in order, equal scores to the smaller flat index; its comment has the two ways and why no address is ever
//              formed from a score.  A source position is clamped to the positions that exist.
// No global atomics, no scratch, no workspace; the output is a function of the arguments alone.
#include "kx8_beam.h"

#pragma clang fp contract(off)

namespace aqlm {

struct Kx8SearchArgs {
  const void* reference;
  const uint16_t* scales;     // [out] or null
  const uint16_t* codebooks;  // [K][256][g]
  const int8_t* prev_codes;   // [out * in / g][K]
  const void* group_ids;
  int8_t* codes_out;  // [num_groups][K]
  float* scores_out;  // [num_groups] or null
  long ref_stride;    // elements
  long num_groups;
  long total_groups;  // out * in / g
  int nj;             // in / g
  int ref_dtype;
  int ids_int64;
  int num_codebooks;
  int beam;
  signed char order[kKxbMaxBooks];
};

// the flat group id of output slot `slot` (wave-uniform), or -1: the slot writes nothing and no address is formed from its id
static __device__ __forceinline__ long kxs_group_of(const Kx8SearchArgs& a, long slot) {
  long gid = slot;
  if (a.group_ids) gid = a.ids_int64 ? (long)reinterpret_cast<const long long*>(a.group_ids)[slot] : (long)reinterpret_cast<const int*>(a.group_ids)[slot];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(unsigned long)gid);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long)gid >> 32));
  gid = (long)(((unsigned long)hi << 32) | lo);
  return gid >= 0 && gid < a.total_groups ? gid : -1;
}

// T: the codebook dtype, G: the group size, PMAX: the beam positions the registers are laid out for (beam_size <= PMAX)
template <class T, int G, int PMAX>
__global__ __launch_bounds__(WAVE) void code_search_kx8_kernel(Kx8SearchArgs a) {
  __shared__ __attribute__((aligned(16))) float res[PMAX][G];
  __shared__ float rn[PMAX];
  __shared__ uint32_t win[PMAX];               // the flat index b * 256 + s of rank i
  __shared__ uint8_t beams[2][PMAX][kKxbMaxBooks];
  __shared__ uint64_t cand[WAVE];              // the keys that reach the bound of a step with several hypotheses to keep
  const int lane = threadIdx.x;
  const int K = a.num_codebooks;
  const int e_own = lane & (G - 1);  // the element this lane serves in every element-wise pass (G divides 64)

  auto entry = [&](int c, int code, int e) { return T::to_float(a.codebooks[((size_t)c * kKxbEntries + (size_t)code) * G + e]); };

  for (long slot = blockIdx.x; slot < a.num_groups; slot += gridDim.x) {
    const long gid = kxs_group_of(a, slot);
    if (gid < 0) continue;  // wave-uniform
    const long o = gid / a.nj, j = gid - o * a.nj;

    // ---- res[0] = r - kept, one position whose beam is the previous codes ----
    if (lane < G) {
      const float x = load_ref(a.reference, (size_t)o * (size_t)a.ref_stride + (size_t)j * G + lane, a.ref_dtype);
      float r = x;
      if (a.scales) r = x / T::to_float(a.scales[o]);  // IEEE division (correctly rounded: the compiler's default for HIP)
      float kept = entry(0, (uint8_t)a.prev_codes[(size_t)gid * K], lane);
      for (int c = 1; c < K; ++c) kept = kept + entry(c, (uint8_t)a.prev_codes[(size_t)gid * K + c], lane);
      res[0][lane] = r - kept;
    }
    if (lane < K) beams[0][0][lane] = (uint8_t)a.prev_codes[(size_t)gid * K + lane];
    __syncthreads();

    int P = 1, cur = 0;
    uint32_t top = 0;
    for (int step = 0; step < K; ++step) {
      const int c = a.order[step];
      const bool last = step == K - 1;
      const int keep = last ? 1 : a.beam;  // (beam_size <= 16 < 256: min(beam_size, positions * 256) is beam_size)

      // ---- free the step's codebook: res[b] = res[b] + C_c[beam[b][c]] ----
      for (int idx = lane; idx < P * G; idx += WAVE) {
        const int b = idx / G;
        res[b][e_own] = res[b][e_own] + entry(c, beams[cur][b][c], e_own);
      }
      // ---- the lane's four candidates, widened, and their squared norms ----
      float cw[kKxbPerLane][G];
      kxb_load_candidates<T, G>(a.codebooks, c, lane, cw);
      float cn[kKxbPerLane];
#pragma unroll
      for (int q = 0; q < kKxbPerLane; ++q) {
        float acc = kxb_mul(cw[q][0], cw[q][0]);
#pragma unroll
        for (int e = 1; e < G; ++e) acc = acc + kxb_mul(cw[q][e], cw[q][e]);
        cn[q] = acc;
      }
      __syncthreads();
      if (lane < P) {
        float acc = kxb_mul(res[lane][0], res[lane][0]);
        for (int e = 1; e < G; ++e) acc = acc + kxb_mul(res[lane][e], res[lane][e]);
        rn[lane] = acc;
      }
      __syncthreads();

      // ---- scores: 4 per position, as ordered integers ----
      uint32_t u[PMAX * kKxbPerLane];
#pragma unroll
      for (int k = 0; k < PMAX * kKxbPerLane; ++k) u[k] = 0xffffffffu;
#pragma unroll
      for (int b = 0; b < PMAX; ++b) {
        if (b < P) {  // wave-uniform
          float acc[kKxbPerLane];
          kxb_dot4<G>(res[b], cw, acc);
          const float rnb = rn[b];
#pragma unroll
          for (int q = 0; q < kKxbPerLane; ++q) u[b * kKxbPerLane + q] = kxb_ordered((rnb - kxb_mul(2.0f, acc[q])) + cn[q]);
        }
      }

      // ---- the best `keep` keys, in order; `top`: the score of the one the last step keeps ----
      bool rounds = PMAX == 1 || keep == 1;  // (PMAX == 1 is launched for one hypothesis only)
#define KXB_SELECT_SCORES 0
#include "kx8_select_body.h"
#undef KXB_SELECT_SCORES
      __syncthreads();

      // ---- rank i takes the codes of its source position with code c replaced; residues move POSITION BY POSITION ----
      for (int idx = lane; idx < keep * K; idx += WAVE) {
        const int i = idx / K, cc = idx - i * K;
        const uint32_t flat = win[i];
        uint32_t source = flat >> 8;
        source = source < (uint32_t)P ? source : 0u;  // (always in range for keys that were taken; a guard, not a rule)
        beams[cur ^ 1][i][cc] = cc == c ? (uint8_t)(flat & 255u) : beams[cur][source][cc];
      }
      if (!last) {
        const float first = res[0][e_own];  // after the first step every new position starts from old position 0
        __syncthreads();
        for (int idx = lane; idx < keep * G; idx += WAVE) {
          const int i = idx / G;
          const float old = P == 1 ? first : res[i][e_own];
          res[i][e_own] = old - entry(c, (int)(win[i] & 255u), e_own);
        }
      }
      __syncthreads();
      cur ^= 1;
      P = keep;
    }
    if (lane < K) a.codes_out[(size_t)slot * K + lane] = (int8_t)beams[cur][0][lane];  // the 8 bits as the checkpoint stores them
    if (lane == 0 && a.scores_out) a.scores_out[slot] = kxb_unordered(top);
    __syncthreads();
  }
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_code_search_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size, int beam_size) {
  if (out_features < 1 || in_features < 1 || !kxb_search_scheme_ok(num_codebooks, in_group_size, beam_size) || in_features % in_group_size != 0) return 0;
  return (long)out_features * (long)(in_features / in_group_size) <= AQLM_HIP_CODE_SEARCH_MAX_GROUPS ? 1 : 0;
}

extern "C" size_t aqlm_hip_code_search_kx8_workspace_bytes(long num_groups, int num_codebooks, int in_group_size, int beam_size) {
  (void)num_groups; (void)num_codebooks; (void)in_group_size; (void)beam_size;
  return 0;  // |C|^2 is formed per wave from the registers that hold the candidates
}

extern "C" int aqlm_hip_code_search_kx8(const void* reference, int reference_dtype, long reference_row_stride, const void* scales,
                                        const void* codebooks, int dtype, const void* prev_codes, int out_features, int in_features,
                                        int num_codebooks, int in_group_size, int beam_size, const int* dim_order, const void* group_ids,
                                        int group_ids_int64, long num_groups, void* codes_out, void* scores_out, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_code_search_kx8";
  (void)workspace; (void)workspace_bytes;
  if (int e = check_not_null(who, reference && codebooks && prev_codes && codes_out)) return e;
  const bool ids_ok = !group_ids || ids_aligned(group_ids, group_ids_int64);
  if (int e = check_aligned(who, "reference / scales / codebooks / group_ids / scores_out",
                            ref_aligned(reference, reference_dtype) && aligned2(scales) && aligned16(codebooks) && ids_ok && aligned4(scores_out)))
    return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  const long total = (long)out_features * (long)(in_features / in_group_size);
  if (reference_row_stride < in_features || num_groups < 1 || (!group_ids && num_groups != total)) {
    set_last_error("%s: bad sizes (reference row stride %ld < in_features %d, or %ld groups where the layer has %ld and no group_ids are given)",
                   who, reference_row_stride, in_features, num_groups, total);
    return AQLM_HIP_E_INVALID;
  }
  if (reference_dtype != AQLM_HIP_F16 && reference_dtype != AQLM_HIP_BF16 && reference_dtype != AQLM_HIP_F32) {
    set_last_error("%s: the reference is float16, bfloat16 or float32 (dtype id %d)", who, reference_dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!kxb_search_scheme_ok(num_codebooks, in_group_size, beam_size) || total > AQLM_HIP_CODE_SEARCH_MAX_GROUPS ||
      num_groups > AQLM_HIP_CODE_SEARCH_MAX_GROUPS) {
    set_last_error("%s: shape outside the kernel (1 to 8 codebooks, groups of 8, 16 or 32, beam_size 1 to %d, at most 2^31 - 1 groups; got "
                   "K=%d g=%d beam_size=%d out=%d in=%d, %ld groups)", who, AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM, num_codebooks, in_group_size,
                   beam_size, out_features, in_features, num_groups);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  Kx8SearchArgs a{};
  if (int e = kxb_parse_dim_order(who, dim_order, num_codebooks, a.order)) return e;
  a.reference = reference;
  a.scales = (const uint16_t*)scales;
  a.codebooks = (const uint16_t*)codebooks;
  a.prev_codes = (const int8_t*)prev_codes;
  a.group_ids = group_ids;
  a.codes_out = (int8_t*)codes_out;
  a.scores_out = (float*)scores_out;
  a.ref_stride = reference_row_stride;
  a.num_groups = num_groups;
  a.total_groups = total;
  a.nj = in_features / in_group_size;
  a.ref_dtype = reference_dtype;
  a.ids_int64 = group_ids_int64 ? 1 : 0;
  a.num_codebooks = num_codebooks;
  a.beam = beam_size;
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = (unsigned)(num_groups < (long)kKxbMaxBlocks ? num_groups : (long)kKxbMaxBlocks);
  // (with one codebook the only step is the last one, which keeps one hypothesis whatever beam_size says)
  const int width = num_codebooks == 1 ? 1 : beam_size;
  return kxb_dispatch(dtype, in_group_size, width, [&](auto ty, auto gs, auto pmax) {
    hipLaunchKernelGGL((code_search_kx8_kernel<decltype(ty), decltype(gs)::value, decltype(pmax)::value>), dim3(blocks), dim3(WAVE), 0, stream, a);
    return check_hip(hipGetLastError(), "code_search_kx8 launch");
  });
}

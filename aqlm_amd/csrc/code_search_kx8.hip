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
//   selection  by the 64-bit key (score bits, b * 256 + s): the tie rule (equal scores -> smaller flat index) falls out of the key.
//              One hypothesis to keep: a wave-wide minimum.  Several: the keep-th smallest of the lanes' own minima bounds the
//              scores that can be kept; the few keys within the bound are gathered in LDS and ranked there by counting (more
//              than 64 of them -- many equal scores -- take `keep` rounds of a wave-wide minimum over the keys above the last
//              one taken instead).  The index half of a key is built from lane and loop counters alone, LDS slots from lane
//              counts, and a source position is clamped to the positions that exist: no address is ever formed from a score,
//              whatever NaNs make of the order.
// No global atomics, no scratch, no workspace; the output is a function of the arguments alone.
#include "aqlm_common.h"

#pragma clang fp contract(off)

namespace aqlm {

// A product that the sum after it cannot absorb.  The pragma above stops the front end from forming fused multiply-adds, but the
// library is built with an explicit -ffp-contract=fast, under which the code generator fuses any product with the sum that uses it
// whatever the pragma says; a product that has passed through an (empty) asm operand is no longer a product to it.  No instruction
// is emitted for the barrier.
static __device__ __forceinline__ float kxs_mul(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));
  return p;
}

constexpr int kKxsEntries = 256;
constexpr int kKxsMaxBooks = 8;
constexpr int kKxsPerLane = kKxsEntries / WAVE;  // candidates per lane: 4
constexpr unsigned kKxsMaxBlocks = 256 * 32;     // grid-stride above this

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
  signed char order[kKxsMaxBooks];
};

static __device__ __forceinline__ float kxs_load_ref(const void* p, size_t idx, int dtype) {
  if (dtype == AQLM_HIP_F32) return reinterpret_cast<const float*>(p)[idx];
  const uint16_t u = reinterpret_cast<const uint16_t*>(p)[idx];
  return dtype == AQLM_HIP_BF16 ? BF16::to_float(u) : F16::to_float(u);
}

// the flat group id of output slot `slot` (wave-uniform), or -1: the slot writes nothing and no address is formed from its id
static __device__ __forceinline__ long kxs_group_of(const Kx8SearchArgs& a, long slot) {
  long gid = slot;
  if (a.group_ids) gid = a.ids_int64 ? (long)reinterpret_cast<const long long*>(a.group_ids)[slot] : (long)reinterpret_cast<const int*>(a.group_ids)[slot];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(unsigned long)gid);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long)gid >> 32));
  gid = (long)(((unsigned long)hi << 32) | lo);
  return gid >= 0 && gid < a.total_groups ? gid : -1;
}

// fp32 bits <-> unsigned integers in the order of the floats
static __device__ __forceinline__ uint32_t kxs_ordered(float s) {
  const uint32_t b = __float_as_uint(s);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
static __device__ __forceinline__ float kxs_unordered(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// minimum over the wave of a 64-bit key (DPP within the rows, scalar across them); wave-uniform result
template <int CTRL>
static __device__ __forceinline__ uint64_t kxs_dpp_min(uint64_t v) {
  const uint64_t o = ((uint64_t)dpp_u32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)v);
  return o < v ? o : v;
}
static __device__ __forceinline__ uint64_t kxs_wave_min(uint64_t v) {
  v = kxs_dpp_min<0xB1>(v);
  v = kxs_dpp_min<0x4E>(v);
  v = kxs_dpp_min<0x141>(v);
  v = kxs_dpp_min<0x140>(v);
  uint64_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 16 * i) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 16 * i);
  const uint64_t x = r[0] < r[1] ? r[0] : r[1], y = r[2] < r[3] ? r[2] : r[3];
  return x < y ? x : y;
}

static __device__ __forceinline__ uint32_t kxs_wave_min_u32(uint32_t v) {
  uint32_t o;
  o = dpp_u32<0xB1>(v);  v = o < v ? o : v;
  o = dpp_u32<0x4E>(v);  v = o < v ? o : v;
  o = dpp_u32<0x141>(v); v = o < v ? o : v;
  o = dpp_u32<0x140>(v); v = o < v ? o : v;
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  const uint32_t a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
  return a < b ? a : b;
}

// T: the codebook dtype, G: the group size, PMAX: the beam positions the registers are laid out for (beam_size <= PMAX)
template <class T, int G, int PMAX>
__global__ __launch_bounds__(WAVE) void code_search_kx8_kernel(Kx8SearchArgs a) {
  __shared__ __attribute__((aligned(16))) float res[PMAX][G];
  __shared__ float rn[PMAX];
  __shared__ uint32_t win[PMAX];               // the flat index b * 256 + s of rank i
  __shared__ uint8_t beams[2][PMAX][kKxsMaxBooks];
  __shared__ uint64_t cand[WAVE];              // the keys that reach the bound of a step with several hypotheses to keep
  const int lane = threadIdx.x;
  const int K = a.num_codebooks;
  const int e_own = lane & (G - 1);  // the element this lane serves in every element-wise pass (G divides 64)

  auto entry = [&](int c, int code, int e) { return T::to_float(a.codebooks[((size_t)c * kKxsEntries + (size_t)code) * G + e]); };

  for (long slot = blockIdx.x; slot < a.num_groups; slot += gridDim.x) {
    const long gid = kxs_group_of(a, slot);
    if (gid < 0) continue;  // wave-uniform
    const long o = gid / a.nj, j = gid - o * a.nj;

    // ---- res[0] = r - kept, one position whose beam is the previous codes ----
    if (lane < G) {
      const float x = kxs_load_ref(a.reference, (size_t)o * (size_t)a.ref_stride + (size_t)j * G + lane, a.ref_dtype);
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
      float cw[kKxsPerLane][G];
      {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.codebooks + ((size_t)c * kKxsEntries + (size_t)kKxsPerLane * lane) * G);
#pragma unroll
        for (int q = 0; q < kKxsPerLane; ++q)
#pragma unroll
          for (int p = 0; p < G / 8; ++p) {
            const u32x4 w = src[q * (G / 8) + p];
            cw[q][8 * p + 0] = T::lo(w.x); cw[q][8 * p + 1] = T::hi(w.x);
            cw[q][8 * p + 2] = T::lo(w.y); cw[q][8 * p + 3] = T::hi(w.y);
            cw[q][8 * p + 4] = T::lo(w.z); cw[q][8 * p + 5] = T::hi(w.z);
            cw[q][8 * p + 6] = T::lo(w.w); cw[q][8 * p + 7] = T::hi(w.w);
          }
      }
      float cn[kKxsPerLane];
#pragma unroll
      for (int q = 0; q < kKxsPerLane; ++q) {
        float acc = kxs_mul(cw[q][0], cw[q][0]);
#pragma unroll
        for (int e = 1; e < G; ++e) acc = acc + kxs_mul(cw[q][e], cw[q][e]);
        cn[q] = acc;
      }
      __syncthreads();
      if (lane < P) {
        float acc = kxs_mul(res[lane][0], res[lane][0]);
        for (int e = 1; e < G; ++e) acc = acc + kxs_mul(res[lane][e], res[lane][e]);
        rn[lane] = acc;
      }
      __syncthreads();

      // ---- scores: 4 per position, as ordered integers ----
      uint32_t u[PMAX * kKxsPerLane];
#pragma unroll
      for (int k = 0; k < PMAX * kKxsPerLane; ++k) u[k] = 0xffffffffu;
#pragma unroll
      for (int b = 0; b < PMAX; ++b) {
        if (b < P) {  // wave-uniform
          const float4* rp = reinterpret_cast<const float4*>(res[b]);
          float acc[kKxsPerLane];
#pragma unroll
          for (int p = 0; p < G / 4; ++p) {
            const float4 rv = rp[p];
            const float re[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int q = 0; q < kKxsPerLane; ++q) {
                const float prod = kxs_mul(re[t], cw[q][4 * p + t]);
                acc[q] = (p == 0 && t == 0) ? prod : acc[q] + prod;
              }
          }
          const float rnb = rn[b];
#pragma unroll
          for (int q = 0; q < kKxsPerLane; ++q) u[b * kKxsPerLane + q] = kxs_ordered((rnb - kxs_mul(2.0f, acc[q])) + cn[q]);
        }
      }

      // ---- the best `keep` keys, in order ----
      bool rounds = PMAX == 1 || keep == 1;
      if (!rounds) {
        // Several to keep: a round costs a pass over every key of the lane, so first cut the keys down.  T = the keep-th smallest of
        // the 64 lanes' own minima is a score that at least `keep` keys reach, so every key of the best `keep` scores <= T; the
        // keys that do (a few more than `keep`, as a rule) are gathered in LDS and ranked there by counting, on the full key.  More
        // than 64 of them (many equal scores) go the general way instead.
        uint32_t mine = 0xffffffffu;
#pragma unroll
        for (int b = 0; b < PMAX; ++b) {
          if (b < P) {
#pragma unroll
            for (int q = 0; q < kKxsPerLane; ++q) mine = u[b * kKxsPerLane + q] < mine ? u[b * kKxsPerLane + q] : mine;
          }
        }
        uint32_t bound = 0;
        for (int r = 0; r < keep; ++r) {
          bound = kxs_wave_min_u32(mine);
          const unsigned long long at = __builtin_amdgcn_ballot_w64(mine == bound);  // (never empty: some lane holds the minimum)
          if (lane == (int)__builtin_ctzll(at | (1ull << 63))) mine = 0xffffffffu;
        }
        int n = 0;  // wave-uniform
#pragma unroll
        for (int b = 0; b < PMAX; ++b) {
          if (b < P) {
#pragma unroll
            for (int q = 0; q < kKxsPerLane; ++q) {
              const bool in = u[b * kKxsPerLane + q] <= bound;
              const unsigned long long set = __builtin_amdgcn_ballot_w64(in);
              if (set != 0) {  // wave-uniform
                const int at = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(set >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)set, 0u));
                if (in && at < WAVE)
                  cand[at] = ((uint64_t)u[b * kKxsPerLane + q] << 32) | (uint32_t)(b * kKxsEntries + kKxsPerLane * lane + q);
                n += (int)__builtin_popcountll(set);
              }
            }
          }
        }
        if (n > WAVE) {
          rounds = true;
        } else {
          __syncthreads();
          const uint64_t key = lane < n ? cand[lane] : ~0ull;
          int rank = 0;
          for (int i = 0; i < n; ++i) rank += cand[i] < key ? 1 : 0;  // keys are distinct (their index halves are): so are the ranks
          if (lane < n && rank < keep) win[rank] = (uint32_t)key;
        }
      }
      // the general way: `keep` rounds, each the wave-wide minimum of the keys above the last one taken
      if (rounds) {
        uint64_t taken = 0;
        for (int r = 0; r < keep; ++r) {
          uint64_t best = ~0ull;
#pragma unroll
          for (int b = 0; b < PMAX; ++b) {
            if (b < P) {
#pragma unroll
              for (int q = 0; q < kKxsPerLane; ++q) {
                const uint64_t key = ((uint64_t)u[b * kKxsPerLane + q] << 32) | (uint32_t)(b * kKxsEntries + kKxsPerLane * lane + q);
                const bool ok = (r == 0 || key > taken) && key < best;
                best = ok ? key : best;
              }
            }
          }
          best = kxs_wave_min(best);
          taken = best;
          if (r == 0) top = (uint32_t)(best >> 32);
          if (lane == 0) win[r] = (uint32_t)best;
        }
      }
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
    if (lane == 0 && a.scores_out) a.scores_out[slot] = kxs_unordered(top);
    __syncthreads();
  }
}

static bool kxs_scheme_ok(int num_codebooks, int g, int beam_size) {
  return num_codebooks >= 1 && num_codebooks <= kKxsMaxBooks && (g == 8 || g == 16 || g == 32) && beam_size >= 1 &&
         beam_size <= AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM;
}
static bool kxs_ref_aligned(const void* p, int dt) { return (reinterpret_cast<uintptr_t>(p) & (dt == AQLM_HIP_F32 ? 3u : 1u)) == 0; }

template <class T, int G>
static int kxs_launch(const Kx8SearchArgs& a, unsigned blocks, hipStream_t stream) {
  // (with one codebook the only step is the last one, which keeps one hypothesis whatever beam_size says)
  const int width = a.num_codebooks == 1 ? 1 : a.beam;
  if (width == 1) hipLaunchKernelGGL((code_search_kx8_kernel<T, G, 1>), dim3(blocks), dim3(WAVE), 0, stream, a);
  else if (width <= 4) hipLaunchKernelGGL((code_search_kx8_kernel<T, G, 4>), dim3(blocks), dim3(WAVE), 0, stream, a);
  else if (width <= 8) hipLaunchKernelGGL((code_search_kx8_kernel<T, G, 8>), dim3(blocks), dim3(WAVE), 0, stream, a);
  else hipLaunchKernelGGL((code_search_kx8_kernel<T, G, 16>), dim3(blocks), dim3(WAVE), 0, stream, a);
  return check_hip(hipGetLastError(), "code_search_kx8 launch");
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_code_search_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size, int beam_size) {
  if (out_features < 1 || in_features < 1 || !kxs_scheme_ok(num_codebooks, in_group_size, beam_size) || in_features % in_group_size != 0) return 0;
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
                            kxs_ref_aligned(reference, reference_dtype) && (reinterpret_cast<uintptr_t>(scales) & 1u) == 0 && aligned16(codebooks) &&
                                ids_ok && (reinterpret_cast<uintptr_t>(scores_out) & 3u) == 0))
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
  if (!kxs_scheme_ok(num_codebooks, in_group_size, beam_size) || total > AQLM_HIP_CODE_SEARCH_MAX_GROUPS ||
      num_groups > AQLM_HIP_CODE_SEARCH_MAX_GROUPS) {
    set_last_error("%s: shape outside the kernel (1 to 8 codebooks, groups of 8, 16 or 32, beam_size 1 to %d, at most 2^31 - 1 groups; got "
                   "K=%d g=%d beam_size=%d out=%d in=%d, %ld groups)", who, AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM, num_codebooks, in_group_size,
                   beam_size, out_features, in_features, num_groups);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  Kx8SearchArgs a{};
  unsigned seen = 0;
  for (int i = 0; i < num_codebooks; ++i) {
    const int c = dim_order ? dim_order[i] : i;
    if (c < 0 || c >= num_codebooks || (seen >> c & 1u)) {
      set_last_error("%s: dim_order must be a permutation of 0 .. %d (entry %d is %d)", who, num_codebooks - 1, i, c);
      return AQLM_HIP_E_INVALID;
    }
    seen |= 1u << c;
    a.order[i] = (signed char)c;
  }
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
  const unsigned blocks = (unsigned)(num_groups < (long)kKxsMaxBlocks ? num_groups : (long)kKxsMaxBlocks);
  if (dtype == AQLM_HIP_F16) {
    if (in_group_size == 8) return kxs_launch<F16, 8>(a, blocks, stream);
    if (in_group_size == 16) return kxs_launch<F16, 16>(a, blocks, stream);
    return kxs_launch<F16, 32>(a, blocks, stream);
  }
  if (in_group_size == 8) return kxs_launch<BF16, 8>(a, blocks, stream);
  if (in_group_size == 16) return kxs_launch<BF16, 16>(a, blocks, stream);
  return kxs_launch<BF16, 32>(a, blocks, stream);
}

// The calibrated code search of the K x 8 schemes (1 to 8 codebooks of 256 entries, out_group_size 1, g = 8 / 16 / 32): one input group
// of the reference's src/beam_search_xtx.py -- the beam search that minimises ||X W_ref^T - X W_q^T||^2 through XTX = X^T X -- for every
// output row of one layer, all K codebook steps of the group in one launch (aqlm_hip_code_search_kx8_xtx; include/aqlm_hip.h has the
// definition, DESIGN.md 4.8o the locality argument, the mapping and the numbers).  The search is local to the group: with
// T_b = (W_ref - W_b) XTX per beam position b, the K steps read and write only the slice T_b[group] (g numbers), the g x g block
// H = XTX[group, group] and q_c[s] = C_c[s] H C_c[s]^T; what the group's change does to the other columns of T_b is the caller's
// (`delta`).  The entry is held to ITS OWN ARITHMETIC bit for bit (tests/kx8_xtx_model.py restates it in numpy): every product and
// every sum below is one IEEE fp32 operation, so this translation unit switches contraction off and passes every product through
// kxb_mul (kx8_beam.h, which holds everything this kernel shares with code_search_kx8.hip).
//
//   work       one wave (a workgroup of 64 threads) per output row, grid-stride over the rows; lane l owns the candidates
//              s = 4 l .. 4 l + 3 of the step's codebook, widened into registers once per step.
//   state      per position, in LDS: the slice t[g], the loss, the group's codes, the position at entry it descends from and the
//              weight change since entry; double-buffered, because a step's survivors are GATHERED from their source positions
//              (the reference re-dequantises every hypothesis: state follows the hypothesis, not the position).
//   scores     S(b, s) = (base[b] - 2 scale dot(C_c[s], u[b])) + scale^2 q_c[s]: 4 * positions values per lane, kept in registers as
//              order-preserving unsigned integers (a score of -0 is stored as +0 first).
//   selection  kx8_select_body.h: the best `keep` 64-bit keys (score bits, b * 256 + s) in order, with their scores; its comment has
//              the two ways and why no address is ever formed from a score.  A source position is clamped to the positions that
//              exist.
// No global atomics, no scratch, no workspace; the output is a function of the arguments alone.
#include "kx8_beam.h"

#pragma clang fp contract(off)

namespace aqlm {

struct Kx8XtxArgs {
  const float* t;             // [positions_in][out][g], strided
  const float* loss;          // [positions_in][out]
  const int8_t* codes_in;     // [positions_in][out][K]
  const float* h;             // [g][g]
  const float* q;             // [K][256]
  const uint16_t* codebooks;  // [K][256][g]
  const uint16_t* scales;     // [out] or null
  float* loss_out;            // [beam][out]
  int8_t* codes_out;          // [beam][out][K]
  uint8_t* source;            // [beam][out]
  float* delta;               // [beam][out][g]
  float* t_out;               // [beam][out][g] or null
  long t_pos_stride, t_row_stride;  // elements
  int out;
  int num_codebooks;
  int beam;
  int positions_in;
  signed char order[kKxbMaxBooks];
};

// equal floats must have equal keys: a score of -0 enters kxb_ordered as +0 (a test of the bit pattern, as the scores are integers next)
static __device__ __forceinline__ float kxx_plus_zero(float s) {
  const uint32_t b = __float_as_uint(s);
  return __uint_as_float(b == 0x80000000u ? 0u : b);
}

// T: the codebook dtype, G: the group size, PMAX: the beam positions the registers and LDS are laid out for
template <class T, int G, int PMAX>
__global__ __launch_bounds__(WAVE) void code_search_kx8_xtx_kernel(Kx8XtxArgs a) {
  __shared__ __attribute__((aligned(16))) float hm[G][G];
  __shared__ __attribute__((aligned(16))) float tt[2][PMAX][G];  // the slice of T per position
  __shared__ __attribute__((aligned(16))) float dl[2][PMAX][G];  // the weight change since entry
  __shared__ __attribute__((aligned(16))) float uu[PMAX][G];
  __shared__ float wb[PMAX][G];  // the scaled previous entry of a step, then the weight change of its survivors
  __shared__ float ls[2][PMAX];
  __shared__ float base[PMAX];
  __shared__ uint32_t win[PMAX];   // the flat index b * 256 + s of rank i
  __shared__ uint32_t wins[PMAX];  // its score, as an ordered integer
  __shared__ uint8_t beams[2][PMAX][kKxbMaxBooks];
  __shared__ uint8_t src[2][PMAX];
  __shared__ uint64_t cand[WAVE];
  const int lane = threadIdx.x;
  const int K = a.num_codebooks;
  const int keep = a.beam;           // (beam_size <= 16 < 256: min(beam_size, positions * 256) is beam_size, on every step)
  const int e_own = lane & (G - 1);  // the element this lane serves in every element-wise pass (G divides 64)
  if (keep > PMAX || a.positions_in > PMAX) return;  // (the launcher picks PMAX >= both; a guard for the LDS arrays, wave-uniform)

  auto entry = [&](int c, int code, int e) { return T::to_float(a.codebooks[((size_t)c * kKxbEntries + (size_t)code) * G + e]); };

  for (int idx = lane; idx < G * G; idx += WAVE) hm[idx / G][idx % G] = a.h[idx];

  for (long o = blockIdx.x; o < a.out; o += gridDim.x) {
    const float s = a.scales ? T::to_float(a.scales[o]) : 1.0f;
    const float two_s = kxb_mul(2.0f, s), ss = kxb_mul(s, s);
    int P = a.positions_in, cur = 0;
    for (int idx = lane; idx < P * G; idx += WAVE) {
      const int b = idx / G;
      tt[0][b][e_own] = a.t[(size_t)b * (size_t)a.t_pos_stride + (size_t)o * (size_t)a.t_row_stride + e_own];
      dl[0][b][e_own] = 0.0f;
    }
    if (lane < P) {
      ls[0][lane] = a.loss[(size_t)lane * a.out + o];
      src[0][lane] = (uint8_t)lane;
    }
    for (int idx = lane; idx < P * K; idx += WAVE) {
      const int b = idx / K, cc = idx - b * K;
      beams[0][b][cc] = (uint8_t)a.codes_in[((size_t)b * a.out + o) * K + cc];
    }
    __syncthreads();

    for (int step = 0; step < K; ++step) {
      const int c = a.order[step];
      const int nxt = cur ^ 1;

      // ---- w[b] = scale * C_c[beam[b][c]] ----
      for (int idx = lane; idx < P * G; idx += WAVE) {
        const int b = idx / G;
        wb[b][e_own] = kxb_mul(s, entry(c, beams[cur][b][c], e_own));
      }
      // ---- the lane's four candidates, widened, and their scaled q ----
      float cw[kKxbPerLane][G];
      kxb_load_candidates<T, G>(a.codebooks, c, lane, cw);
      float sq[kKxbPerLane];
#pragma unroll
      for (int q = 0; q < kKxbPerLane; ++q) sq[q] = kxb_mul(ss, a.q[(size_t)c * kKxbEntries + kKxbPerLane * lane + q]);
      __syncthreads();
      // ---- u[b][f'] = t[b][f'] + sum_f w[b][f] H[f][f'] ----
      for (int idx = lane; idx < P * G; idx += WAVE) {
        const int b = idx / G;
        float acc = kxb_mul(wb[b][0], hm[0][e_own]);
        for (int f = 1; f < G; ++f) acc = acc + kxb_mul(wb[b][f], hm[f][e_own]);
        uu[b][e_own] = tt[cur][b][e_own] + acc;
      }
      __syncthreads();
      // ---- base[b] = (L[b] + 2 scale <P, u[b]>) - scale^2 q_c[p] ----
      if (lane < P) {
        const int p = beams[cur][lane][c];
        float acc = kxb_mul(entry(c, p, 0), uu[lane][0]);
        for (int f = 1; f < G; ++f) acc = acc + kxb_mul(entry(c, p, f), uu[lane][f]);
        base[lane] = (ls[cur][lane] + kxb_mul(two_s, acc)) - kxb_mul(ss, a.q[(size_t)c * kKxbEntries + p]);
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
          kxb_dot4<G>(uu[b], cw, acc);
          const float bb = base[b];
#pragma unroll
          for (int q = 0; q < kKxbPerLane; ++q) u[b * kKxbPerLane + q] = kxb_ordered(kxx_plus_zero((bb - kxb_mul(two_s, acc[q])) + sq[q]));
        }
      }

      // ---- the best `keep` keys, in order, and their scores ----
      bool rounds = keep == 1;
#define KXB_SELECT_SCORES 1
#include "kx8_select_body.h"
#undef KXB_SELECT_SCORES
      __syncthreads();

      // ---- rank i descends from its source position: codes, entry position, loss, weight change ----
      for (int idx = lane; idx < keep * K; idx += WAVE) {
        const int i = idx / K, cc = idx - i * K;
        const uint32_t flat = win[i];
        uint32_t from = flat >> 8;
        from = from < (uint32_t)P ? from : 0u;  // (always in range for keys that were taken; a guard, not a rule)
        beams[nxt][i][cc] = cc == c ? (uint8_t)(flat & 255u) : beams[cur][from][cc];
      }
      if (lane < keep) {
        uint32_t from = win[lane] >> 8;
        from = from < (uint32_t)P ? from : 0u;
        src[nxt][lane] = src[cur][from];
        ls[nxt][lane] = kxb_unordered(wins[lane]);
      }
      for (int idx = lane; idx < keep * G; idx += WAVE) {
        const int i = idx / G;
        const uint32_t flat = win[i];
        uint32_t from = flat >> 8;
        from = from < (uint32_t)P ? from : 0u;
        const float dw = kxb_mul(s, entry(c, (int)(flat & 255u), e_own)) - kxb_mul(s, entry(c, beams[cur][from][c], e_own));
        wb[i][e_own] = dw;
        dl[nxt][i][e_own] = dl[cur][from][e_own] + dw;
      }
      __syncthreads();
      // ---- t[i][f'] = t[source][f'] - sum_f dw[i][f] H[f][f'] ----
      for (int idx = lane; idx < keep * G; idx += WAVE) {
        const int i = idx / G;
        uint32_t from = win[i] >> 8;
        from = from < (uint32_t)P ? from : 0u;
        float acc = kxb_mul(wb[i][0], hm[0][e_own]);
        for (int f = 1; f < G; ++f) acc = acc + kxb_mul(wb[i][f], hm[f][e_own]);
        tt[nxt][i][e_own] = tt[cur][from][e_own] - acc;
      }
      __syncthreads();
      cur = nxt;
      P = keep;
    }

    for (int idx = lane; idx < keep * K; idx += WAVE) {
      const int i = idx / K, cc = idx - i * K;
      a.codes_out[((size_t)i * a.out + o) * K + cc] = (int8_t)beams[cur][i][cc];  // the 8 bits as the checkpoint stores them
    }
    if (lane < keep) {
      a.loss_out[(size_t)lane * a.out + o] = ls[cur][lane];
      a.source[(size_t)lane * a.out + o] = src[cur][lane];
    }
    for (int idx = lane; idx < keep * G; idx += WAVE) {
      const int i = idx / G;
      a.delta[((size_t)i * a.out + o) * G + e_own] = dl[cur][i][e_own];
      if (a.t_out) a.t_out[((size_t)i * a.out + o) * G + e_own] = tt[cur][i][e_own];
    }
    __syncthreads();
  }
}

static bool kxx_scheme_ok(int num_codebooks, int g, int beam_size, int positions_in) {
  return kxb_search_scheme_ok(num_codebooks, g, beam_size) && positions_in >= 1 && positions_in <= AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_code_search_kx8_xtx_supported(int out_features, int num_codebooks, int in_group_size, int beam_size, int positions_in) {
  return out_features >= 1 && kxx_scheme_ok(num_codebooks, in_group_size, beam_size, positions_in) ? 1 : 0;
}

extern "C" size_t aqlm_hip_code_search_kx8_xtx_workspace_bytes(int out_features, int num_codebooks, int in_group_size, int beam_size) {
  (void)out_features; (void)num_codebooks; (void)in_group_size; (void)beam_size;
  return 0;  // the state of a row lives in the LDS of its wave
}

extern "C" int aqlm_hip_code_search_kx8_xtx(const void* t, long t_position_stride, long t_row_stride, const void* loss, const void* codes_in,
                                            const void* h, const void* q, const void* codebooks, int dtype, const void* scales,
                                            int out_features, int num_codebooks, int in_group_size, int beam_size, int positions_in,
                                            const int* dim_order, void* loss_out, void* codes_out, void* source_out, void* delta_out,
                                            void* t_out, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_code_search_kx8_xtx";
  (void)workspace; (void)workspace_bytes;
  if (int e = check_not_null(who, t && loss && codes_in && h && q && codebooks && loss_out && codes_out && source_out && delta_out)) return e;
  if (int e = check_aligned(who, "t / loss / H / q / scales / codebooks / loss_out / delta / t_out",
                            aligned4(t) && aligned4(loss) && aligned4(h) && aligned4(q) && aligned2(scales) && aligned16(codebooks) &&
                                aligned4(loss_out) && aligned4(delta_out) && aligned4(t_out)))
    return e;
  if (out_features < 1 || in_group_size < 1) {
    set_last_error("%s: bad sizes (out=%d g=%d)", who, out_features, in_group_size);
    return AQLM_HIP_E_INVALID;
  }
  if (t_row_stride < in_group_size || (positions_in > 1 && t_position_stride < in_group_size)) {
    set_last_error("%s: bad sizes (t row stride %ld or position stride %ld below the group size %d)", who, t_row_stride, t_position_stride,
                   in_group_size);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!kxx_scheme_ok(num_codebooks, in_group_size, beam_size, positions_in)) {
    set_last_error("%s: shape outside the kernel (1 to 8 codebooks, groups of 8, 16 or 32, beam_size and positions_in 1 to %d; got K=%d g=%d "
                   "beam_size=%d positions_in=%d)", who, AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM, num_codebooks, in_group_size, beam_size, positions_in);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  Kx8XtxArgs a{};
  if (int e = kxb_parse_dim_order(who, dim_order, num_codebooks, a.order)) return e;
  a.t = (const float*)t;
  a.loss = (const float*)loss;
  a.codes_in = (const int8_t*)codes_in;
  a.h = (const float*)h;
  a.q = (const float*)q;
  a.codebooks = (const uint16_t*)codebooks;
  a.scales = (const uint16_t*)scales;
  a.loss_out = (float*)loss_out;
  a.codes_out = (int8_t*)codes_out;
  a.source = (uint8_t*)source_out;
  a.delta = (float*)delta_out;
  a.t_out = (float*)t_out;
  a.t_pos_stride = positions_in > 1 ? t_position_stride : 0;
  a.t_row_stride = t_row_stride;
  a.out = out_features;
  a.num_codebooks = num_codebooks;
  a.beam = beam_size;
  a.positions_in = positions_in;
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = (unsigned)out_features < kKxbMaxBlocks ? (unsigned)out_features : kKxbMaxBlocks;
  // the positions the LDS and registers must hold: those at entry, and the beam_size survivors that EVERY step keeps (the only
  // step of a single codebook too)
  const int width = positions_in > beam_size ? positions_in : beam_size;
  return kxb_dispatch(dtype, in_group_size, width, [&](auto ty, auto gs, auto pmax) {
    hipLaunchKernelGGL((code_search_kx8_xtx_kernel<decltype(ty), decltype(gs)::value, decltype(pmax)::value>), dim3(blocks), dim3(WAVE), 0, stream, a);
    return check_hip(hipGetLastError(), "code_search_kx8_xtx launch");
  });
}

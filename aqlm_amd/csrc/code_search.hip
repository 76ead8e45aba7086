// The V step of PV-tuning for the 1x16 schemes (one codebook of 65536 entries, out_group_size 1, g = 8 / 16): for every group of g
// weights the nearest codeword,
//     code(n) = argmin over c of S(n, c),  S(n, c) = |C_c|^2 - 2 <r_n, C_c>,  r_n = reference[o, j*g : (j+1)*g] / scales[o]   (fp32, IEEE)
// (aqlm_hip_code_search_1x16; include/aqlm_hip.h has the contract, DESIGN.md 4.8m the derivation of its epsilon).  It is one skinny
// GEMM (K = g) whose 65536 x groups output never exists: codewords along M, groups along N of v_mfma_f32_32x32x16, so that a lane
// holds 16 codewords' scores of ONE group per accumulator tile and the running minimum is lane-local.
//
//   operands   A: lanes l and l + 32 load codeword row l % 32 of the tile (g = 8: the same 16 bytes; g = 16: the halves of its 32
//              bytes).  B: r is scaled by an exact power of two so that max|r| lies in [2^10, 2^11) and split into two 16-bit
//              operands, r' = hi + lo.  g = 8: lanes 0-31 carry hi, lanes 32-63 carry lo, ONE instruction sums <hi + lo, C_c> in
//              fp32; g = 16: two instructions on the same A fragment.  The scaling keeps both parts of an fp16 split in the normal
//              range whatever the magnitude of r (no group is out of range of the operand format).
//   scores     s = fma(acc, -2^(e - 9), |C_c|^2): one fp32 operation per score; |C_c|^2 in fp32 from the workspace (a launch of its
//              own fills it: one thread per codeword, fused multiply-adds over t ascending).
//   minimum    per tile the minimum of the lane's 16 scores (v_min3), compared with the running minimum; only when a lane of the
//              wave improves is the row resolved (the first of the 16 registers that holds the tile minimum -- registers ascend
//              with the row).  Strict "<" over ascending tiles: equal scores keep the smallest index.
//   work       a workgroup of 4 waves owns 128 groups (4 tiles of 32); wave w scans the codebook quarter [w * 16384, (w + 1) *
//              16384) for all of them -- one codeword load feeds 4 (g = 16: 8) MFMAs -- streaming it from L2, the next tile's
//              loads in flight under the current tile's arithmetic.  Then the two halves of a wave (xor 32) and the four waves
//              (LDS) are reduced, the smaller index winning equal scores.
// No atomics, no scratch; the output is a function of the inputs alone.  A group with a non-finite element searches with r = 0
// (the codeword of smallest norm): in range, and the Python layer keeps such a group's previous code.
#include "aqlm_common.h"

namespace aqlm {

constexpr int kCsThreads = 256;
constexpr int kCsWaves = kCsThreads / WAVE;
constexpr int kCsEntries = 65536;
constexpr int kCsTiles = 4;                               // group tiles of 32 per workgroup
constexpr int kCsBlockGroups = kCsTiles * 32;             // 128
constexpr int kCsCodeTiles = kCsEntries / 32 / kCsWaves;  // codeword tiles of 32 per wave: 512

typedef float cs_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 cs_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cs_bf16x8 __attribute__((ext_vector_type(8)));

template <class T>
static __device__ __forceinline__ cs_f32x16 cs_mfma(const u32x4& a, const u32x4& b, const cs_f32x16& c) {
  if constexpr (T::id == AQLM_HIP_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cs_f16x8, a), __builtin_bit_cast(cs_f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cs_bf16x8, a), __builtin_bit_cast(cs_bf16x8, b), c, 0, 0, 0);
}

// |C_c|^2 in fp32: fused multiply-adds over t ascending from 0
template <class T, int G>
__global__ __launch_bounds__(kCsThreads) void code_search_norms_kernel(const uint16_t* __restrict__ codebook, float* __restrict__ norms) {
  const int c = blockIdx.x * kCsThreads + threadIdx.x;  // grid = 65536 / 256
  const u32x4* row = reinterpret_cast<const u32x4*>(codebook + (size_t)c * G);
  float acc = 0.f;
#pragma unroll
  for (int p = 0; p < G / 8; ++p) {
    const u32x4 q = row[p];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = T::lo(w[i]), b = T::hi(w[i]);
      acc = __builtin_fmaf(a, a, acc);
      acc = __builtin_fmaf(b, b, acc);
    }
  }
  norms[c] = acc;
}

struct CodeSearchArgs {
  const void* reference;
  const uint16_t* scales;  // [out] or null
  const uint16_t* codebook;
  const float* norms;  // [65536]
  const void* group_ids;
  int16_t* codes_out;
  long ref_stride;  // elements
  long num_groups;
  long total_groups;  // out * in / g
  int nj;             // in / g
  int ref_dtype;
  int ids_int64;
};

// the flat group id of output slot `slot`, or -1: the slot writes nothing (no address is formed from such an id)
static __device__ __forceinline__ long cs_group_of(const CodeSearchArgs& a, long slot) {
  if (slot >= a.num_groups) return -1;
  long gid = slot;
  if (a.group_ids) gid = a.ids_int64 ? (long)reinterpret_cast<const long long*>(a.group_ids)[slot] : (long)reinterpret_cast<const int*>(a.group_ids)[slot];
  return gid >= 0 && gid < a.total_groups ? gid : -1;
}

template <class T, int G>
__global__ __launch_bounds__(kCsThreads) void code_search_1x16_kernel(CodeSearchArgs a) {
  __shared__ float red_m[kCsWaves][kCsBlockGroups];
  __shared__ int red_i[kCsWaves][kCsBlockGroups];
  const int l = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int col = l & 31, h = l >> 5;
  const long slot0 = (long)blockIdx.x * kCsBlockGroups;

  // ---- B fragments: the split of the scaled r, and the factor that undoes the scaling ----
  u32x4 bhi[kCsTiles], blo[kCsTiles];  // g = 8: bhi is the lane's ONE fragment (hi in lanes 0-31, lo in lanes 32-63); blo unused
  float negk[kCsTiles];
#pragma unroll
  for (int t = 0; t < kCsTiles; ++t) {
    const long gid = cs_group_of(a, slot0 + t * 32 + col);
    float r[G];
    bool bad = gid < 0;
    float mx = 0.f;
    if (gid >= 0) {
      const long o = gid / a.nj, j = gid - o * a.nj;
      const float s = a.scales ? (T::id == AQLM_HIP_BF16 ? BF16::to_float(a.scales[o]) : F16::to_float(a.scales[o])) : 1.f;
      const size_t base = (size_t)o * (size_t)a.ref_stride + (size_t)j * G;
#pragma unroll
      for (int e = 0; e < G; ++e) {
        const float x = load_ref(a.reference, base + e, a.ref_dtype);
        r[e] = a.scales ? x / s : x;  // IEEE division (correctly rounded: the compiler's default for HIP), as the definition divides
        const float ax = __builtin_fabsf(r[e]);
        bad = bad || !(ax < __builtin_inff());  // Inf or NaN
        mx = __builtin_fmaxf(mx, ax);
      }
    }
    // max|r| = m * 2^e, m in [1, 2); the exponent is clamped from below only (a subnormal or tiny maximum would ask for a factor
    // beyond fp32); up to e = 127 both powers of two below are normal numbers and r' stays below 2^11
    int e2 = (int)((__float_as_uint(mx) >> 23) & 0xffu) - 127;
    if (bad || mx == 0.f) e2 = 0;
    e2 = e2 < -100 ? -100 : e2;
    const float up = __uint_as_float((uint32_t)(127 + 10 - e2) << 23);  // r' = r * 2^(10 - e)
    negk[t] = -__uint_as_float((uint32_t)(127 + e2 - 9) << 23);          // S = |C|^2 - 2 * 2^(e - 10) * <r', C>
    uint32_t hi[G / 2], lo[G / 2];
#pragma unroll
    for (int p = 0; p < G / 2; ++p) {
      uint32_t hw[2], lw[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float x = bad ? 0.f : r[2 * p + q] * up;
        const uint16_t hb = T::from_float(x);
        const uint16_t lb = T::from_float(x - T::to_float(hb));
        hw[q] = hb;
        lw[q] = lb;
      }
      hi[p] = hw[0] | (hw[1] << 16);
      lo[p] = lw[0] | (lw[1] << 16);
    }
    if constexpr (G == 8) {
      bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{lo[0], lo[1], lo[2], lo[3]};
      blo[t] = bhi[t];
    } else {
      bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{hi[4], hi[5], hi[6], hi[7]};
      blo[t] = h == 0 ? u32x4{lo[0], lo[1], lo[2], lo[3]} : u32x4{lo[4], lo[5], lo[6], lo[7]};
    }
  }

  // ---- the scan of this wave's quarter of the codebook ----
  float best_m[kCsTiles];
  int best_i[kCsTiles];
  const int tile0 = w * kCsCodeTiles;
#pragma unroll
  for (int t = 0; t < kCsTiles; ++t) {
    best_m[t] = __builtin_inff();
    best_i[t] = tile0 * 32;
  }
  // lane's A piece of codeword tile ct: row col; g = 8: its 16 bytes, g = 16: half h of its 32 bytes
  const u32x4* cb = reinterpret_cast<const u32x4*>(a.codebook) + (G == 8 ? col : 2 * col + h);
  // the lane's 16 rows of a tile: (reg & 3) + 8 * (reg >> 2) + 4 * h  ->  four float4 of norms at 8 * q + 4 * h
  const float4* nr = reinterpret_cast<const float4*>(a.norms) + h;
  auto load_a = [&](int ct) { return cb[(size_t)ct * (32 * G / 8)]; };
  u32x4 a_next = load_a(tile0);
  float4 n_next[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) n_next[q] = nr[(size_t)tile0 * 8 + 2 * q];
  for (int i = 0; i < kCsCodeTiles; ++i) {
    const int ct = tile0 + i;
    const u32x4 a_cur = a_next;
    float n2[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      n2[4 * q] = n_next[q].x;
      n2[4 * q + 1] = n_next[q].y;
      n2[4 * q + 2] = n_next[q].z;
      n2[4 * q + 3] = n_next[q].w;
    }
    const int nx = i + 1 < kCsCodeTiles ? ct + 1 : ct;  // (the last iteration repeats its own addresses)
    a_next = load_a(nx);
#pragma unroll
    for (int q = 0; q < 4; ++q) n_next[q] = nr[(size_t)nx * 8 + 2 * q];
#pragma unroll
    for (int t = 0; t < kCsTiles; ++t) {
      cs_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      acc = cs_mfma<T>(a_cur, bhi[t], acc);
      if constexpr (G == 16) acc = cs_mfma<T>(a_cur, blo[t], acc);
      float s[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) s[v] = __builtin_fmaf(acc[v], negk[t], n2[v]);
      // fminf drops a NaN operand: a NaN score never wins
      float tm = __builtin_fminf(s[0], s[1]);
#pragma unroll
      for (int v = 2; v < 16; v += 2) tm = __builtin_fminf(__builtin_fminf(tm, s[v]), s[v + 1]);
      const bool better = tm < best_m[t];
      if (__builtin_amdgcn_ballot_w64(better) != 0) {  // wave-uniform branch
        int reg = 0;
#pragma unroll
        for (int v = 15; v >= 0; --v) reg = s[v] == tm ? v : reg;  // the first register that holds the minimum
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        best_i[t] = better ? ct * 32 + row : best_i[t];
        best_m[t] = better ? tm : best_m[t];
      }
    }
  }

  // ---- the two halves of the wave, then the four waves; equal scores: the smaller index ----
#pragma unroll
  for (int t = 0; t < kCsTiles; ++t) {
    const float om = __shfl_xor(best_m[t], 32);
    const int oi = __shfl_xor(best_i[t], 32);
    if (om < best_m[t] || (om == best_m[t] && oi < best_i[t])) {
      best_m[t] = om;
      best_i[t] = oi;
    }
    if (h == 0) {
      red_m[w][t * 32 + col] = best_m[t];
      red_i[w][t * 32 + col] = best_i[t];
    }
  }
  __syncthreads();
  if (threadIdx.x < kCsBlockGroups) {
    const long slot = slot0 + threadIdx.x;
    if (cs_group_of(a, slot) < 0) return;
    float m = red_m[0][threadIdx.x];
    int idx = red_i[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kCsWaves; ++k) {
      const float om = red_m[k][threadIdx.x];
      const int oi = red_i[k][threadIdx.x];
      if (om < m || (om == m && oi < idx)) {
        m = om;
        idx = oi;
      }
    }
    a.codes_out[slot] = (int16_t)(uint16_t)idx;  // the 16 bits as the checkpoint stores them
  }
}

static bool cs_shape_ok(int out_features, int in_features, int g) {
  if (out_features < 1 || in_features < 1 || (g != 8 && g != 16) || in_features % g != 0) return false;
  return (long)out_features * (long)(in_features / g) <= AQLM_HIP_CODE_SEARCH_MAX_GROUPS;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_code_search_1x16_supported(int out_features, int in_features, int in_group_size) {
  return cs_shape_ok(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" size_t aqlm_hip_code_search_1x16_workspace_bytes(long num_groups, int in_group_size) {
  if (num_groups < 1 || num_groups > AQLM_HIP_CODE_SEARCH_MAX_GROUPS || (in_group_size != 8 && in_group_size != 16)) return 0;
  return (size_t)kCsEntries * sizeof(float);
}

extern "C" int aqlm_hip_code_search_1x16(const void* reference, int reference_dtype, long reference_row_stride, const void* scales,
                                         const void* codebook, int dtype, int out_features, int in_features, int in_group_size,
                                         const void* group_ids, int group_ids_int64, long num_groups, void* codes_out, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_code_search_1x16";
  if (int e = check_not_null(who, reference && codebook && codes_out && workspace)) return e;
  const bool ids_ok = !group_ids || ids_aligned(group_ids, group_ids_int64);
  if (int e = check_aligned(who, "reference / scales / codebook / group_ids / codes_out / workspace",
                            ref_aligned(reference, reference_dtype) && (reinterpret_cast<uintptr_t>(scales) & 1u) == 0 && aligned16(codebook) &&
                                ids_ok && (reinterpret_cast<uintptr_t>(codes_out) & 1u) == 0 && aligned16(workspace)))
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
  if (int e = check_group_size(who, in_group_size)) return e;
  if (!cs_shape_ok(out_features, in_features, in_group_size) || num_groups > AQLM_HIP_CODE_SEARCH_MAX_GROUPS) {
    set_last_error("%s: shape outside the kernel (at most 2^31 - 1 groups; got out=%d in=%d g=%d, %ld groups)", who, out_features, in_features,
                   in_group_size, num_groups);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t need = (size_t)kCsEntries * sizeof(float);
  if (workspace_bytes < need) {
    set_last_error("%s: a workspace of %zu bytes where %zu bytes are needed", who, workspace_bytes, need);
    return AQLM_HIP_E_INVALID;
  }
  CodeSearchArgs a{};
  a.reference = reference;
  a.scales = (const uint16_t*)scales;
  a.codebook = (const uint16_t*)codebook;
  a.norms = (const float*)workspace;
  a.group_ids = group_ids;
  a.codes_out = (int16_t*)codes_out;
  a.ref_stride = reference_row_stride;
  a.num_groups = num_groups;
  a.total_groups = total;
  a.nj = in_features / in_group_size;
  a.ref_dtype = reference_dtype;
  a.ids_int64 = group_ids_int64 ? 1 : 0;
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = (unsigned)((num_groups + kCsBlockGroups - 1) / kCsBlockGroups);
  return dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto gs) {
    using T = decltype(t);
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((code_search_norms_kernel<T, G>), dim3(kCsEntries / kCsThreads), dim3(kCsThreads), 0, stream, a.codebook,
                       (float*)workspace);
    if (int e = check_hip(hipGetLastError(), "code_search_norms launch")) return e;
    hipLaunchKernelGGL((code_search_1x16_kernel<T, G>), dim3(blocks), dim3(kCsThreads), 0, stream, a);
    return check_hip(hipGetLastError(), "code_search_1x16 launch");
  });
}

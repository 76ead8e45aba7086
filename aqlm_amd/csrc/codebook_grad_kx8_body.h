// The kernels of the K x 8 codebook and scale gradients (codebook_grad_kx8.hip has the contract; calib_grad.hip launches the
// same bodies on fp32 operands).
#pragma once
#include "aqlm_common.h"

namespace aqlm {

constexpr int kKx8Threads = 256;
constexpr int kKx8Entries = 256;
constexpr int kKx8MaxK = AQLM_HIP_CODEBOOK_GRAD_KX8_MAX_CODEBOOKS;
constexpr int kKx8MaxBlocks = AQLM_HIP_CODEBOOK_GRAD_KX8_MAX_ROW_BLOCKS;
constexpr int kKx8MaximaBlocks = AQLM_HIP_CODEBOOK_GRAD_KX8_MAXIMA_BLOCKS;  // the maxima launch streams: its row blocks are its own
constexpr uint32_t kNonFinite = 0x7f800000u;  // fp32 patterns from here on (sign cleared) are Inf / NaN

template <class DW>
static __device__ __host__ __forceinline__ constexpr size_t kx8_elem_bytes() {
  return DW::id == AQLM_HIP_F32 ? 4 : 2;
}
// elements in a 16-byte piece of dW
template <class DW>
static constexpr int kx8_piece() {
  return DW::id == AQLM_HIP_F32 ? 4 : 8;
}

// one 16-byte piece at `p` as fp32
template <class DW>
static __device__ __forceinline__ void kx8_load_piece(const void* p, float (&v)[kx8_piece<DW>()]) {
  if constexpr (DW::id == AQLM_HIP_F32) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x;
    v[1] = f.y;
    v[2] = f.z;
    v[3] = f.w;
  } else {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
    v[0] = DW::lo(w.x);
    v[1] = DW::hi(w.x);
    v[2] = DW::lo(w.y);
    v[3] = DW::hi(w.y);
    v[4] = DW::lo(w.z);
    v[5] = DW::hi(w.z);
    v[6] = DW::lo(w.w);
    v[7] = DW::hi(w.w);
  }
}

static __device__ __forceinline__ void kx8_store_out(void* out, size_t idx, float v, int out_dtype) {
  if (out_dtype == AQLM_HIP_F32)
    reinterpret_cast<float*>(out)[idx] = v;
  else if (out_dtype == AQLM_HIP_BF16)
    reinterpret_cast<uint16_t*>(out)[idx] = BF16::from_float(v);
  else
    reinterpret_cast<uint16_t*>(out)[idx] = F16::from_float(v);
}

// maximum of two unsigned values over the workgroup (256 threads); every thread receives both
static __device__ __forceinline__ void kx8_block_max2(uint32_t& a, uint32_t& b) {
  __shared__ uint32_t red[2 * (kKx8Threads / WAVE)];
  a = wave_max_u32(a);
  b = wave_max_u32(b);
  const int w = threadIdx.x / WAVE;
  __syncthreads();  // (a previous use of red is over)
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[2 * w] = a;
    red[2 * w + 1] = b;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kKx8Threads / WAVE; ++i) {
    a = red[2 * i] > a ? red[2 * i] : a;
    b = red[2 * i + 1] > b ? red[2 * i + 1] : b;
  }
}

struct Kx8GradArgs {
  const void* dw;
  const void* scales;      // [M] in scales_dtype, or null
  const uint8_t* codes;    // [M][nj][K]
  void* out;               // [K][256][g]
  long long* partials;     // [B][K][256][g]
  uint32_t* maxima;        // [NM][2]: max|dW|, max|s| as fp32 patterns
  long dws;                // row stride of dW, elements
  int M;
  int nj;  // in_features / g
  int K;
  int g;
  int B;       // row blocks
  int NM;      // row blocks of the maxima launch: min(M, 1024)
  int passes;  // codebook passes
  int shift;   // 62 - bit_length(M * nj)
  int scales_dtype;  // fp16 / bf16 of the training entries, fp32 of the calibrated ones
  int out_dtype;
};

static __device__ __forceinline__ int kx8_row_begin(const Kx8GradArgs& a, int b) { return (int)((long)b * (long)a.M / (long)a.B); }

// what the layer's maxima say: 0 = finite and non-zero (E is set), 1 = every output is +0, 2 = every output is NaN
static __device__ __forceinline__ int kx8_reduce_maxima(const Kx8GradArgs& a, int& E) {
  uint32_t mdw = 0, ms = 0;
  for (int i = threadIdx.x; i < a.NM; i += kKx8Threads) {
    const uint32_t d = a.maxima[2 * i], s = a.maxima[2 * i + 1];
    mdw = d > mdw ? d : mdw;
    ms = s > ms ? s : ms;
  }
  kx8_block_max2(mdw, ms);
  E = 0;
  if (mdw >= kNonFinite || ms >= kNonFinite) return 2;
  const double bound = (double)__uint_as_float(ms) * (double)__uint_as_float(mdw);  // exact, and normal or zero in double
  if (bound == 0.0) return 1;
  E = (int)((__double_as_longlong(bound) >> 52) & 0x7ff) - 1022;  // bound = m * 2^E, m in [0.5, 1)
  return 0;
}

template <class DW>
__global__ __launch_bounds__(kKx8Threads) void codebook_grad_kx8_maxima_kernel(Kx8GradArgs a) {
  const int b = blockIdx.x;
  const int r0 = (int)((long)b * (long)a.M / (long)a.NM), r1 = (int)((long)(b + 1) * (long)a.M / (long)a.NM);
  constexpr int PE = kx8_piece<DW>();
  const uint32_t ppr = (uint32_t)(a.nj * a.g) / PE;  // 16-byte pieces per row
  const uint32_t total = (uint32_t)(r1 - r0) * ppr;  // < 2^30
  const char* dw = reinterpret_cast<const char*>(a.dw);
  uint32_t mdw = 0, ms = 0;
  for (uint32_t i = threadIdx.x; i < total; i += kKx8Threads) {
    const uint32_t r = i / ppr, p = i - r * ppr;
    float v[PE];
    kx8_load_piece<DW>(dw + ((size_t)(r0 + r) * (size_t)a.dws + (size_t)p * PE) * kx8_elem_bytes<DW>(), v);
#pragma unroll
    for (int e = 0; e < PE; ++e) {
      const uint32_t u = __float_as_uint(v[e]) & 0x7fffffffu;
      mdw = u > mdw ? u : mdw;
    }
  }
  if (a.scales) {
    for (int r = r0 + (int)threadIdx.x; r < r1; r += kKx8Threads) {
      const uint32_t u = __float_as_uint(load_ref(a.scales, r, a.scales_dtype)) & 0x7fffffffu;
      ms = u > ms ? u : ms;
    }
  } else {
    ms = 0x3f800000u;  // 1
  }
  kx8_block_max2(mdw, ms);
  if (threadIdx.x == 0) {
    a.maxima[2 * b] = mdw;
    a.maxima[2 * b + 1] = ms;
  }
}

template <class DW, int G>
__global__ __launch_bounds__(kKx8Threads) void codebook_grad_kx8_accumulate_kernel(Kx8GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long kx8_image[];  // [nc][256][G + 1]
  constexpr int KS = 64 / G;   // codebooks per pass
  constexpr int ES = G + 1;    // entry stride in LDS
  constexpr int PE = kx8_piece<DW>();
  const int b = blockIdx.x / a.passes, pass = blockIdx.x - b * a.passes;
  const int c0 = pass * KS;
  const int nc = a.K - c0 < KS ? a.K - c0 : KS;
  int E;
  if (kx8_reduce_maxima(a, E) != 0) return;  // uniform over the grid: the finish launch reads no partials then
  for (int i = threadIdx.x; i < nc * kKx8Entries * ES; i += kKx8Threads) kx8_image[i] = 0ull;
  __syncthreads();
  // 2^(shift - E): a normal double for every E the supported dtypes can produce (|E| <= 173, 32 <= shift <= 61)
  const double mul = __longlong_as_double((long long)(1023 + a.shift - E) << 52);
  const int r0 = kx8_row_begin(a, b), r1 = kx8_row_begin(a, b + 1);
  const uint32_t nj = (uint32_t)a.nj, total = (uint32_t)(r1 - r0) * nj;
  const char* dw = reinterpret_cast<const char*>(a.dw);
  // two positions of this thread in flight: both sets of loads are issued before the first add
  for (uint32_t i0 = threadIdx.x; i0 < total; i0 += 2 * kKx8Threads) {
    uint32_t base[2][KS];
    double s[2];
    const char* grp[2];
    bool has[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t i = i0 + u * kKx8Threads;
      has[u] = i < total;
      const uint32_t ic = has[u] ? i : i0;  // (the absent second position repeats the first one's addresses and adds nothing)
      const uint32_t r = ic / nj, j = ic - r * nj;
      const int o = r0 + (int)r;
      const uint8_t* cp = a.codes + ((size_t)o * nj + j) * (size_t)a.K + c0;
#pragma unroll
      for (int ci = 0; ci < KS; ++ci) base[u][ci] = ci < nc ? (uint32_t)(ci * kKx8Entries + cp[ci]) * ES : 0u;
      s[u] = a.scales ? (double)load_ref(a.scales, o, a.scales_dtype) : 1.0;
      grp[u] = dw + ((size_t)o * (size_t)a.dws + (size_t)j * G) * kx8_elem_bytes<DW>();
    }
#pragma unroll
    for (int p = 0; p < G / PE; ++p) {
      float v[2][PE];
      kx8_load_piece<DW>(grp[0] + (size_t)p * 16, v[0]);
      kx8_load_piece<DW>(grp[1] + (size_t)p * 16, v[1]);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!has[u]) continue;
#pragma unroll
        for (int e = 0; e < PE; ++e) {
          // the product is exact in double (24 x 11 significant bits), the scaling exact; round to nearest even
          const long long q = (long long)__builtin_rint(s[u] * (double)v[u][e] * mul);
#pragma unroll
          for (int ci = 0; ci < KS; ++ci)
            if (ci < nc) atomicAdd(&kx8_image[base[u][ci] + p * PE + e], (unsigned long long)q);
        }
      }
    }
  }
  __syncthreads();
  // partials[b][c0 + ci][v][t], contiguous over (ci, v, t)
  long long* dst = a.partials + ((size_t)b * a.K + c0) * kKx8Entries * G;
  for (int i = threadIdx.x; i < nc * kKx8Entries * G; i += kKx8Threads) dst[i] = (long long)kx8_image[(i / G) * ES + (i % G)];
}

// 64 output elements per workgroup; the four waves take the row blocks w, w + 4, ... and their int64 sums are added in LDS
// (a template only so that the two objects that include this file may both hold it)
template <int = 0>
__global__ __launch_bounds__(kKx8Threads) void codebook_grad_kx8_finish_kernel(Kx8GradArgs a) {
  __shared__ long long part[kKx8Threads];
  const int n_out = a.K * kKx8Entries * a.g;  // a multiple of 64
  const int idx = blockIdx.x * WAVE + (int)(threadIdx.x & (WAVE - 1));
  const int w = threadIdx.x / WAVE;
  int E;
  const int special = kx8_reduce_maxima(a, E);
  if (special != 0) {
    if (w == 0 && idx < n_out) kx8_store_out(a.out, (size_t)idx, special == 2 ? __uint_as_float(0x7fc00000u) : 0.f, a.out_dtype);
    return;
  }
  long long sum = 0;
  if (idx < n_out) {
    const long long* p = a.partials + idx;
    int blk = w;
    for (; blk + 12 < a.B; blk += 16) {  // four loads in flight
      const long long x0 = p[(size_t)blk * n_out], x1 = p[(size_t)(blk + 4) * n_out], x2 = p[(size_t)(blk + 8) * n_out],
                      x3 = p[(size_t)(blk + 12) * n_out];
      sum += (x0 + x1) + (x2 + x3);
    }
    for (; blk < a.B; blk += 4) sum += p[(size_t)blk * n_out];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  if (w != 0 || idx >= n_out) return;
  const long long S = (part[threadIdx.x] + part[threadIdx.x + WAVE]) + (part[threadIdx.x + 2 * WAVE] + part[threadIdx.x + 3 * WAVE]);
  // int64 -> fp32 round to nearest even, an exact power of two, then the storage rounding
  kx8_store_out(a.out, (size_t)idx, ldexpf((float)S, E - a.shift), a.out_dtype);
}

struct Kx8ScalesGradArgs {
  const void* dw;
  const uint8_t* codes;       // [M][nj][K]
  const uint16_t* codebooks;  // [K][256][g]
  void* out;                  // [M]
  long dws;
  int M;
  int nj;
  int K;
  int cb_bf16;
  int out_dtype;
};

// The codebooks staged once per workgroup in their storage dtype; one wave per row, rows grid-stride: lane l takes the groups l,
// l + 64 ... of the row, sums the K entries in fp32 in codebook order and adds the g products in order into one fp32 register;
// wave_sum adds the lanes.  Which wave takes a row does not enter the order.
template <class DW, int G>
__global__ __launch_bounds__(kKx8Threads) void scales_grad_kx8_kernel(Kx8ScalesGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t kx8_cb[];  // [K][256][G]
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(a.codebooks);
    u32x4* dst = reinterpret_cast<u32x4*>(kx8_cb);
    for (int i = threadIdx.x; i < a.K * kKx8Entries * G / 8; i += kKx8Threads) dst[i] = src[i];
  }
  __syncthreads();
  constexpr int PE = kx8_piece<DW>();
  const int l = threadIdx.x & (WAVE - 1);
  const int waves = gridDim.x * (kKx8Threads / WAVE);
  for (int o = blockIdx.x * (kKx8Threads / WAVE) + (int)(threadIdx.x / WAVE); o < a.M; o += waves) {  // wave-uniform
    const char* row = reinterpret_cast<const char*>(a.dw) + (size_t)o * (size_t)a.dws * kx8_elem_bytes<DW>();
    const uint8_t* codes = a.codes + (size_t)o * a.nj * (size_t)a.K;
    float acc = 0.f;
    for (int j = l; j < a.nj; j += WAVE) {
      const uint8_t* cp = codes + (size_t)j * a.K;
      uint32_t v[kKx8MaxK];
#pragma unroll
      for (int c = 0; c < kKx8MaxK; ++c) v[c] = c < a.K ? (uint32_t)cp[c] : 0u;
#pragma unroll
      for (int h = 0; h < G / 8; ++h) {  // eight features at a time
        float w[8];
#pragma unroll
        for (int c = 0; c < kKx8MaxK; ++c) {
          if (c < a.K) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(kx8_cb + ((size_t)(c * kKx8Entries) + v[c]) * G + h * 8);
            float e[8];
            if (a.cb_bf16) {
              e[0] = BF16::lo(q.x); e[1] = BF16::hi(q.x); e[2] = BF16::lo(q.y); e[3] = BF16::hi(q.y);
              e[4] = BF16::lo(q.z); e[5] = BF16::hi(q.z); e[6] = BF16::lo(q.w); e[7] = BF16::hi(q.w);
            } else {
              e[0] = F16::lo(q.x); e[1] = F16::hi(q.x); e[2] = F16::lo(q.y); e[3] = F16::hi(q.y);
              e[4] = F16::lo(q.z); e[5] = F16::hi(q.z); e[6] = F16::lo(q.w); e[7] = F16::hi(q.w);
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) w[t] = c == 0 ? e[t] : w[t] + e[t];
          }
        }
        const char* grp = row + ((size_t)j * G + h * 8) * kx8_elem_bytes<DW>();
#pragma unroll
        for (int p = 0; p < 8 / PE; ++p) {
          float d[PE];
          kx8_load_piece<DW>(grp + (size_t)p * 16, d);
#pragma unroll
          for (int e = 0; e < PE; ++e) acc = __builtin_fmaf(d[e], w[p * PE + e], acc);
        }
      }
    }
    acc = wave_sum(acc);
    if (l == 0) kx8_store_out(a.out, (size_t)o, acc, a.out_dtype);
  }
}

static bool kx8_shape_ok(int out_features, int in_features, int K, int g) {
  if (out_features < 1 || in_features < 1 || K < 1 || K > kKx8MaxK || (g != 8 && g != 16 && g != 32) || in_features % g != 0) return false;
  return (long)out_features * (long)(in_features / g) < (1L << 30);
}
static int kx8_passes(int K, int g) { return (K + 64 / g - 1) / (64 / g); }
static int kx8_row_blocks(int out_features, int K, int g) {
  return std::min(out_features, std::max(1, kKx8MaxBlocks / kx8_passes(K, g)));
}
static size_t kx8_partial_bytes(int out_features, int K, int g) {
  return (size_t)kx8_row_blocks(out_features, K, g) * (size_t)K * kKx8Entries * (size_t)g * 8;
}
static size_t kx8_workspace_bytes(int out_features, int K, int g) {
  return kx8_partial_bytes(out_features, K, g) + (size_t)kKx8MaximaBlocks * 8;
}
static int kx8_bit_length(long v) {
  int n = 0;
  for (; v > 0; v >>= 1) ++n;
  return n;
}

// f(DW{}, GroupSize<g>{}) for the three dW types and the three group sizes
template <class F>
static int kx8_dispatch(int dw_dtype, int g, F&& f) {
  auto by_group = [&](auto dwt) {
    if (g == 8) return f(dwt, GroupSize<8>{});
    if (g == 16) return f(dwt, GroupSize<16>{});
    return f(dwt, GroupSize<32>{});
  };
  if (dw_dtype == AQLM_HIP_F32) return by_group(F32{});
  if (dw_dtype == AQLM_HIP_BF16) return by_group(BF16{});
  return by_group(F16{});
}

// the checks both entries share after the pointers
static int kx8_check_shape(const char* who, long dw_row_stride, int dw_dtype, int dtype, int out_features, int in_features, int K, int g,
                           int out_dtype, bool has_workspace, size_t workspace_bytes) {
  if (int e = check_sizes(who, out_features, in_features, g)) return e;
  const bool shape_ok = kx8_shape_ok(out_features, in_features, K, g);
  const size_t need = has_workspace && shape_ok ? kx8_workspace_bytes(out_features, K, g) : 0;
  if (dw_row_stride < in_features || workspace_bytes < need) {
    set_last_error("%s: bad sizes (dW row stride %ld < in_features %d, or a workspace of %zu bytes where %zu bytes are needed)", who,
                   dw_row_stride, in_features, workspace_bytes, need);
    return AQLM_HIP_E_INVALID;
  }
  if (!dw_dtype_ok(dw_dtype) || !dw_dtype_ok(out_dtype)) {
    set_last_error("%s: dW and the output are float16, bfloat16 or float32 (dtype ids %d, %d)", who, dw_dtype, out_dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (K < 1 || K > kKx8MaxK) {
    set_last_error("%s: 1 to %d codebooks of 256 entries are supported, got %d", who, kKx8MaxK, K);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (g != 8 && g != 16 && g != 32) {
    set_last_error("%s: only codebooks with 8, 16 or 32 features are supported, got %d", who, g);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (!shape_ok || ((size_t)dw_row_stride * dtype_bytes(dw_dtype)) % 16 != 0) {
    set_last_error("%s: shape outside the kernel (fewer than 2^30 positions, dW rows 16-byte aligned; got out=%d in=%d g=%d, row stride %ld)",
                   who, out_features, in_features, g, dw_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return 0;
}

// the three launches of the codebook gradient on checked arguments (scales in `scales_dtype`: fp16 / bf16 / fp32, or null)
static int kx8_codebook_grad_launch(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int scales_dtype, const void* codes,
                                    int out_features, int in_features, int K, int g, void* out, int out_dtype, void* workspace,
                                    hipStream_t stream) {
  Kx8GradArgs a{};
  a.dw = dw;
  a.scales = scales;
  a.codes = (const uint8_t*)codes;
  a.out = out;
  a.partials = (long long*)workspace;
  a.maxima = (uint32_t*)((char*)workspace + kx8_partial_bytes(out_features, K, g));
  a.dws = dw_row_stride;
  a.M = out_features;
  a.nj = in_features / g;
  a.K = K;
  a.g = g;
  a.B = kx8_row_blocks(out_features, K, g);
  a.passes = kx8_passes(K, g);
  a.NM = std::min(out_features, kKx8MaximaBlocks);
  a.shift = 62 - kx8_bit_length((long)out_features * (long)a.nj);
  a.scales_dtype = scales_dtype;
  a.out_dtype = out_dtype;
  const size_t lds = (size_t)std::min(K, 64 / g) * kKx8Entries * (size_t)(g + 1) * 8;
  return kx8_dispatch(dw_dtype, g, [&](auto dwt, auto gs) {
    using DW = decltype(dwt);
    constexpr int G = decltype(gs)::value;
    auto acc = &codebook_grad_kx8_accumulate_kernel<DW, G>;
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(acc), lds)) return e;
    hipLaunchKernelGGL((codebook_grad_kx8_maxima_kernel<DW>), dim3(a.NM), dim3(kKx8Threads), 0, stream, a);
    if (int e = check_hip(hipGetLastError(), "codebook_grad_kx8_maxima launch")) return e;
    hipLaunchKernelGGL(acc, dim3(a.B * a.passes), dim3(kKx8Threads), lds, stream, a);
    if (int e = check_hip(hipGetLastError(), "codebook_grad_kx8_accumulate launch")) return e;
    hipLaunchKernelGGL(codebook_grad_kx8_finish_kernel<>, dim3(K * kKx8Entries * G / WAVE), dim3(kKx8Threads), 0, stream, a);
    return check_hip(hipGetLastError(), "codebook_grad_kx8_finish launch");
  });
}

}  // namespace aqlm

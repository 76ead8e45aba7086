// The kernels of the 1x16 codebook and scale gradients (codebook_grad.hip has the contract; calib_grad.hip launches the same
// bodies on fp32 operands).
#pragma once
#include "aqlm_common.h"

namespace aqlm {

constexpr int kCgChunk = AQLM_HIP_CODEBOOK_GRAD_CHUNK;
constexpr int kCgLanes = 16;
constexpr int kCgThreads = 256;
constexpr int kCgEntries = 65536;

// G consecutive elements at `p` (16-byte aligned) as fp32, loaded in 16-byte pieces
template <class DW, int G>
static __device__ __forceinline__ void load_group(const void* p, float (&v)[G]) {
  if constexpr (DW::id == AQLM_HIP_F32) {
    const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int i = 0; i < G / 4; ++i) {
      const float4 f = q[i];
      v[4 * i] = f.x;
      v[4 * i + 1] = f.y;
      v[4 * i + 2] = f.z;
      v[4 * i + 3] = f.w;
    }
  } else {
    const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < G / 8; ++i) {
      const u32x4 w = q[i];
      v[8 * i] = DW::lo(w.x);
      v[8 * i + 1] = DW::hi(w.x);
      v[8 * i + 2] = DW::lo(w.y);
      v[8 * i + 3] = DW::hi(w.y);
      v[8 * i + 4] = DW::lo(w.z);
      v[8 * i + 5] = DW::hi(w.z);
      v[8 * i + 6] = DW::lo(w.w);
      v[8 * i + 7] = DW::hi(w.w);
    }
  }
}

template <class DW>
static __device__ __forceinline__ size_t elem_bytes() {
  return DW::id == AQLM_HIP_F32 ? 4 : 2;
}

static __device__ __forceinline__ void store_out(void* out, size_t idx, float v, int out_dtype) {
  if (out_dtype == AQLM_HIP_F32)
    reinterpret_cast<float*>(out)[idx] = v;
  else if (out_dtype == AQLM_HIP_BF16)
    reinterpret_cast<uint16_t*>(out)[idx] = BF16::from_float(v);
  else
    reinterpret_cast<uint16_t*>(out)[idx] = F16::from_float(v);
}

struct CodebookGradArgs {
  const void* dw;
  const void* scales;       // [M] in scales_dtype, or null
  const int* starts;        // [65537]
  const int* order;         // [n_codes]
  const int* chunks;        // [max_chunks][3]: entry, begin, end
  const int* chunk_starts;  // [65537]
  void* out;                // [65536][g]
  float* ws;                // [max_chunks][g]
  long dws;                 // row stride of dW, elements
  int nj;                   // in_features / g
  int n_codes;
  int max_chunks;
  int scales_dtype;         // fp16 / bf16 of the training entries, fp32 of the calibrated ones
  int out_dtype;
};

template <class DW, int G>
__global__ __launch_bounds__(kCgThreads) void codebook_grad_chunk_kernel(CodebookGradArgs a) {
  const int unit = blockIdx.x * (kCgThreads / kCgLanes) + (int)(threadIdx.x / kCgLanes);
  const int l = threadIdx.x & (kCgLanes - 1);
  // every lane runs to the reduction (a chunk that is absent or malformed has n = 0): the DPP butterfly reads its neighbours
  int e = -1, b = 0, n = 0;
  if (unit < a.max_chunks) {
    const int ce = a.chunks[3 * (size_t)unit], cb = a.chunks[3 * (size_t)unit + 1], cend = a.chunks[3 * (size_t)unit + 2];
    if (ce >= 0 && ce < kCgEntries && cb >= 0 && cend >= cb && cend <= a.n_codes && cend - cb <= kCgChunk) {
      e = ce;
      b = cb;
      n = cend - cb;
    }
  }
  float acc[G];
#pragma unroll
  for (int t = 0; t < G; ++t) acc[t] = 0.f;
  const uint32_t nj = (uint32_t)a.nj, n_codes = (uint32_t)a.n_codes;
  const char* dw = reinterpret_cast<const char*>(a.dw);
  for (int i = l; i < n; i += 2 * kCgLanes) {
    // two positions of this lane in flight; they are added in list order
    const uint32_t p0 = (uint32_t)a.order[b + i];
    const bool has1 = i + kCgLanes < n;
    const uint32_t p1 = has1 ? (uint32_t)a.order[b + i + kCgLanes] : 0xffffffffu;
    const bool ok0 = p0 < n_codes, ok1 = p1 < n_codes;  // a position outside the layer is skipped, never dereferenced
    float v0[G], v1[G], s0 = 1.f, s1 = 1.f;
    if (ok0) {
      const uint32_t o = p0 / nj, j = p0 - o * nj;
      load_group<DW, G>(dw + ((size_t)o * (size_t)a.dws + (size_t)j * G) * elem_bytes<DW>(), v0);
      if (a.scales) s0 = load_ref(a.scales, o, a.scales_dtype);
    }
    if (ok1) {
      const uint32_t o = p1 / nj, j = p1 - o * nj;
      load_group<DW, G>(dw + ((size_t)o * (size_t)a.dws + (size_t)j * G) * elem_bytes<DW>(), v1);
      if (a.scales) s1 = load_ref(a.scales, o, a.scales_dtype);
    }
    if (ok0) {
#pragma unroll
      for (int t = 0; t < G; ++t) acc[t] = __builtin_fmaf(s0, v0[t], acc[t]);
    }
    if (ok1) {
#pragma unroll
      for (int t = 0; t < G; ++t) acc[t] = __builtin_fmaf(s1, v1[t], acc[t]);
    }
  }
  float mine = 0.f;
#pragma unroll
  for (int t = 0; t < G; ++t) {
    const float total = row16_sum(acc[t]);
    if (l == t) mine = total;
  }
  if (e < 0 || l >= G) return;
  const int nc = a.chunk_starts[e + 1] - a.chunk_starts[e];
  if (nc == 1)
    store_out(a.out, (size_t)e * G + l, mine, a.out_dtype);
  else
    a.ws[(size_t)unit * G + l] = mine;
}

// one thread per output element: +0 for an unused entry, nothing for an entry of one chunk (written above), the partials in
// chunk order for the others
template <int G>
__global__ __launch_bounds__(kCgThreads) void codebook_grad_finish_kernel(CodebookGradArgs a) {
  const int idx = blockIdx.x * kCgThreads + (int)threadIdx.x;
  if (idx >= kCgEntries * G) return;
  const int e = idx / G, t = idx % G;
  const int uses = a.starts[e + 1] - a.starts[e];
  const int cs = a.chunk_starts[e], cend = a.chunk_starts[e + 1];
  if (uses <= 0 || cs < 0 || cend <= cs || cend > a.max_chunks) {
    store_out(a.out, (size_t)idx, 0.f, a.out_dtype);
    return;
  }
  if (cend - cs == 1) return;
  const float* p = a.ws + (size_t)cs * G + t;
  float sum = 0.f;
  int i = 0;
  const int nc = cend - cs;
  for (; i + 4 <= nc; i += 4) {  // four loads in flight, added in chunk order
    const float x0 = p[(size_t)i * G], x1 = p[(size_t)(i + 1) * G], x2 = p[(size_t)(i + 2) * G], x3 = p[(size_t)(i + 3) * G];
    sum += x0;
    sum += x1;
    sum += x2;
    sum += x3;
  }
  for (; i < nc; ++i) sum += p[(size_t)i * G];
  store_out(a.out, (size_t)idx, sum, a.out_dtype);
}

struct ScalesGradArgs {
  const void* dw;
  const uint16_t* codes;     // [M][nj], canonical
  const uint16_t* codebook;  // [65536][g]
  void* out;                 // [M]
  long dws;
  int M;
  int nj;
  int cb_bf16;
  int out_dtype;
};

// one wave per output row: lane l takes the groups l, l + 64 ... of the row (dW and codes stream coalesced, the codebook entry
// is gathered in 16-byte pieces from L2), adds their g products in order into one fp32 register; wave_sum adds the lanes
template <class DW, int G>
__global__ __launch_bounds__(kCgThreads) void scales_grad_kernel(ScalesGradArgs a) {
  const int o = blockIdx.x * (kCgThreads / WAVE) + (int)(threadIdx.x / WAVE);
  const int l = threadIdx.x & (WAVE - 1);
  if (o >= a.M) return;  // wave-uniform
  const char* row = reinterpret_cast<const char*>(a.dw) + (size_t)o * (size_t)a.dws * elem_bytes<DW>();
  const uint16_t* codes = a.codes + (size_t)o * a.nj;
  float acc = 0.f;
  for (int j = l; j < a.nj; j += WAVE) {
    const uint32_t c = codes[j];
    float v[G], w[G];
    load_group<DW, G>(row + (size_t)j * G * elem_bytes<DW>(), v);
    if (a.cb_bf16)
      load_group<BF16, G>(a.codebook + (size_t)c * G, w);
    else
      load_group<F16, G>(a.codebook + (size_t)c * G, w);
#pragma unroll
    for (int t = 0; t < G; ++t) acc = __builtin_fmaf(v[t], w[t], acc);
  }
  acc = wave_sum(acc);
  if (l == 0) store_out(a.out, (size_t)o, acc, a.out_dtype);
}

static bool cg_shape_ok(int out_features, int in_features, int g) {
  if (out_features < 1 || in_features < 1 || (g != 8 && g != 16) || in_features % g != 0) return false;
  return (long)out_features * (long)(in_features / g) <= (long)AQLM_HIP_CODEBOOK_GRAD_MAX_CODES;
}

static long cg_max_chunks(int out_features, int in_features, int g) {
  const long n = (long)out_features * (long)(in_features / g);
  return std::min<long>(n, kCgEntries) + n / kCgChunk;
}

// f(DW{}, GroupSize<g>{}) for the three dW types
template <class F>
static int dispatch_dw_group(int dw_dtype, int g, F&& f) {
  if (dw_dtype == AQLM_HIP_F32) return g == 8 ? f(F32{}, GroupSize<8>{}) : f(F32{}, GroupSize<16>{});
  return dispatch_dtype_group(dw_dtype, g, f);
}

// the two launches of the codebook gradient on checked arguments (scales in `scales_dtype`: fp16 / bf16 / fp32, or null)
static int cg_codebook_grad_launch(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int scales_dtype, const void* starts,
                                   const void* order, const void* chunks, const void* chunk_starts, int out_features, int in_features,
                                   int in_group_size, void* out, int out_dtype, void* workspace, hipStream_t stream) {
  CodebookGradArgs a{};
  a.dw = dw;
  a.scales = scales;
  a.starts = (const int*)starts;
  a.order = (const int*)order;
  a.chunks = (const int*)chunks;
  a.chunk_starts = (const int*)chunk_starts;
  a.out = out;
  a.ws = (float*)workspace;
  a.dws = dw_row_stride;
  a.nj = in_features / in_group_size;
  a.n_codes = out_features * a.nj;
  a.max_chunks = (int)cg_max_chunks(out_features, in_features, in_group_size);
  a.scales_dtype = scales_dtype;
  a.out_dtype = out_dtype;
  const int per_block = kCgThreads / kCgLanes;
  const dim3 grid((a.max_chunks + per_block - 1) / per_block);
  return dispatch_dw_group(dw_dtype, in_group_size, [&](auto dwt, auto gs) {
    using DW = decltype(dwt);
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((codebook_grad_chunk_kernel<DW, G>), grid, dim3(kCgThreads), 0, stream, a);
    if (int e = check_hip(hipGetLastError(), "codebook_grad_chunk launch")) return e;
    hipLaunchKernelGGL((codebook_grad_finish_kernel<G>), dim3(kCgEntries * G / kCgThreads), dim3(kCgThreads), 0, stream, a);
    return check_hip(hipGetLastError(), "codebook_grad_finish launch");
  });
}

}  // namespace aqlm

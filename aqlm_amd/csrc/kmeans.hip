// Residual k-means initialisation of AQLM layers (the reference's init_aq_kmeans: src/aq.py:288-356, src/kmeans.py:24-117, 162-186):
// one Lloyd iteration as two entries.
//
//   aqlm_hip_kmeans_assign   code(n) = argmin over c of S(n, c),  S(n, c) = |C_c|^2 - 2 <x_n, C_c>,  x [N, d] and C [k, d] in fp32,
//                            d = 8 / 16, k a multiple of 128 up to 65536 -- and, fused into the same launch, the sums and counts of
//                            the points of every cluster as fixed-point integers.
//   aqlm_hip_kmeans_update   centroid = sum / count where count > 0; an empty cluster keeps its centroid bit for bit.
//
// The assignment is code_search.hip's scan (include/aqlm_hip.h has the contract, DESIGN.md 4.8r the derivation of its epsilon):
// centroids along M, points along N of v_mfma_f32_32x32x16_f16, the running minimum lane-local, the index resolved only on a
// wave-uniform improvement, strict "<" over ascending tiles.  What differs:
//   operands   BOTH sides are fp32, so both reach the matrix unit as split pairs of fp16 values, v' = hi + lo.  A point is scaled by
//              its own power of two (max|x_n| into [2^10, 2^11)), the centroids by ONE power of two for the whole table (max over c, t
//              of |C_ct| into [2^10, 2^11): a first launch finds it, a second writes the split image and |C_c|^2 into the workspace).
//              d = 8: B = [x_hi | x_lo], A = [C_hi | C_hi] gives <x, C_hi> in one K = 16 instruction, A = [C_lo | C_lo] adds <x, C_lo>.
//              d = 16: three instructions, hi.hi + lo.hi + hi.lo (lo.lo is below 2^-22 of |x||C| and is left out).
//   work       a workgroup of 4 waves owns 128 points at a time; wave w scans the tiles [w * k / 128, (w + 1) * k / 128) of 32 centroids.
//   sums       when the scan ends thread p of the first 128 knows the winner of point p and adds q_t = rint(x_t * 2^s) to
//              sums[winner][t] (64-bit) and 1 to counts[winner]: integer adds commute, so the result does not depend on arrival
//              order.  With k * d * 8 bytes <= 64 KiB the adds go to LDS, a workgroup walks many blocks of points and flushes its
//              non-zero cells once; above that they go straight to memory.
// No scratch.  A point with a non-finite element searches with x = 0; such a point, and one with an element above data_absmax, adds
// nothing to the sums.
#include <math.h>

#include "aqlm_common.h"

namespace aqlm {

constexpr int kKmThreads = 256;
constexpr int kKmWaves = kKmThreads / WAVE;
constexpr int kKmTiles = 4;                    // point tiles of 32 per workgroup
constexpr int kKmBlockPoints = kKmTiles * 32;  // 128
constexpr int kKmHeaderBytes = 256;            // workspace: header (max|C| as bits), |C_c|^2, the hi image, the lo image
constexpr int kKmRedBytes = 2 * kKmWaves * kKmBlockPoints * 4;
constexpr int kKmLdsSumBytes = 64 * 1024;
constexpr int kKmLdsGrid = 1024;  // workgroups of the LDS pre-reduced launch (each walks its share of the point blocks)
constexpr int kKmExpClamp = 50;

typedef float km_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 km_f16x8 __attribute__((ext_vector_type(8)));

static __device__ __forceinline__ km_f32x16 km_mfma(const u32x4& a, const u32x4& b, const km_f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(km_f16x8, a), __builtin_bit_cast(km_f16x8, b), c, 0, 0, 0);
}

// the exponent e of a maximum m * 2^e (bits of |m|, finite), clamped: both 2^(10 - e) and the product of two such factors stay normal
static __device__ __forceinline__ int km_exponent(uint32_t bits) {
  int e = bits ? (int)(bits >> 23) - 127 : 0;
  e = e < -kKmExpClamp ? -kKmExpClamp : e;
  return e > kKmExpClamp ? kKmExpClamp : e;
}

// x * 2^(10 - e) for D values as an fp16 pair per value: hi[p] / lo[p] hold elements 2p and 2p + 1
template <int D>
static __device__ __forceinline__ void km_split(const float (&v)[D], float up, bool zero, uint32_t (&hi)[D / 2], uint32_t (&lo)[D / 2]) {
#pragma unroll
  for (int p = 0; p < D / 2; ++p) {
    uint32_t hw[2], lw[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float x = zero ? 0.f : v[2 * p + q] * up;
      const uint16_t hb = F16::from_float(x);
      hw[q] = hb;
      lw[q] = F16::from_float(x - F16::to_float(hb));
    }
    hi[p] = hw[0] | (hw[1] << 16);
    lo[p] = lw[0] | (lw[1] << 16);
  }
}

// max over the finite elements of |C|, as the bits of a float, into header[0] (zeroed by the entry)
__global__ __launch_bounds__(kKmThreads) void kmeans_absmax_kernel(const float* __restrict__ c, long count, uint32_t* __restrict__ header) {
  uint32_t m = 0;
  for (long i = (long)blockIdx.x * kKmThreads + threadIdx.x; i < count; i += (long)gridDim.x * kKmThreads) {
    const uint32_t b = __float_as_uint(c[i]) & 0x7fffffffu;
    m = (b < 0x7f800000u && b > m) ? b : m;
  }
  m = wave_max_u32(m);
  if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicMax(header, m);
}

// |C_c|^2 in fp32 (fused multiply-adds over t ascending from 0) and the split image of centroid c; grid = k / 128
template <int D>
__global__ __launch_bounds__(128) void kmeans_split_kernel(const float* __restrict__ c, const uint32_t* __restrict__ header,
                                                           float* __restrict__ norms, uint16_t* __restrict__ chi, uint16_t* __restrict__ clo) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  float v[D];
#pragma unroll
  for (int p = 0; p < D / 4; ++p) {
    const float4 q = reinterpret_cast<const float4*>(c + (size_t)i * D)[p];
    v[4 * p] = q.x;
    v[4 * p + 1] = q.y;
    v[4 * p + 2] = q.z;
    v[4 * p + 3] = q.w;
  }
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < D; ++t) acc = __builtin_fmaf(v[t], v[t], acc);
  norms[i] = acc;
  const float up = __uint_as_float((uint32_t)(127 + 10 - km_exponent(header[0])) << 23);
  uint32_t hi[D / 2], lo[D / 2];
  km_split<D>(v, up, false, hi, lo);
#pragma unroll
  for (int p = 0; p < D / 8; ++p) {
    reinterpret_cast<u32x4*>(chi + (size_t)i * D)[p] = u32x4{hi[4 * p], hi[4 * p + 1], hi[4 * p + 2], hi[4 * p + 3]};
    reinterpret_cast<u32x4*>(clo + (size_t)i * D)[p] = u32x4{lo[4 * p], lo[4 * p + 1], lo[4 * p + 2], lo[4 * p + 3]};
  }
}

struct KmeansArgs {
  const float* data;
  const uint32_t* header;
  const float* norms;
  const uint16_t* chi;
  const uint16_t* clo;
  int* codes_out;
  unsigned long long* sums;  // [k][d] two's complement, or null
  int* counts;               // [k], or null
  double scale;              // 2^s
  float data_absmax;
  long n;
  long num_blocks;  // blocks of 128 points
  int k;
};

constexpr int KM_NO_SUMS = 0, KM_DIRECT = 1, KM_LDS = 2;

template <int D, int MODE>
__global__ __launch_bounds__(kKmThreads) void kmeans_assign_kernel(KmeansArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
  float(*red_m)[kKmBlockPoints] = reinterpret_cast<float(*)[kKmBlockPoints]>(km_smem);
  int(*red_i)[kKmBlockPoints] = reinterpret_cast<int(*)[kKmBlockPoints]>(km_smem + kKmRedBytes / 2);
  unsigned long long* lsum = reinterpret_cast<unsigned long long*>(km_smem + kKmRedBytes);
  int* lcnt = reinterpret_cast<int*>(km_smem + kKmRedBytes + (size_t)a.k * D * 8);
  const int l = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int col = l & 31, h = l >> 5;
  if constexpr (MODE == KM_LDS) {
    for (int i = threadIdx.x; i < a.k * D; i += kKmThreads) lsum[i] = 0ull;
    for (int i = threadIdx.x; i < a.k; i += kKmThreads) lcnt[i] = 0;
    __syncthreads();
  }
  const int ec = km_exponent(a.header[0]);
  const int tiles = a.k / (32 * kKmWaves);  // centroid tiles of 32 per wave
  const int tile0 = w * tiles;
  // lane's A pieces of centroid tile ct: row col; d = 8: its 16 bytes, d = 16: half h of its 32 bytes
  const u32x4* cbh = reinterpret_cast<const u32x4*>(a.chi) + (D == 8 ? col : 2 * col + h);
  const u32x4* cbl = reinterpret_cast<const u32x4*>(a.clo) + (D == 8 ? col : 2 * col + h);
  // the lane's 16 rows of a tile: (reg & 3) + 8 * (reg >> 2) + 4 * h  ->  four float4 of norms at 8 * q + 4 * h
  const float4* nr = reinterpret_cast<const float4*>(a.norms) + h;

  for (long pb = blockIdx.x; pb < a.num_blocks; pb += gridDim.x) {
    const long slot0 = pb * kKmBlockPoints;
    // ---- B fragments: the split of the scaled point, and the factor that undoes both scalings ----
    u32x4 bhi[kKmTiles], blo[kKmTiles];  // d = 8: bhi is the lane's ONE fragment (hi in lanes 0-31, lo in lanes 32-63)
    float negk[kKmTiles];
#pragma unroll
    for (int t = 0; t < kKmTiles; ++t) {
      const long slot = slot0 + t * 32 + col;
      float r[D];
      bool bad = slot >= a.n;
      float mx = 0.f;
#pragma unroll
      for (int e = 0; e < D; ++e) r[e] = 0.f;
      if (slot < a.n) {
#pragma unroll
        for (int p = 0; p < D / 4; ++p) {
          const float4 q = reinterpret_cast<const float4*>(a.data + (size_t)slot * D)[p];
          r[4 * p] = q.x;
          r[4 * p + 1] = q.y;
          r[4 * p + 2] = q.z;
          r[4 * p + 3] = q.w;
        }
#pragma unroll
        for (int e = 0; e < D; ++e) {
          const float ax = __builtin_fabsf(r[e]);
          bad = bad || !(ax < __builtin_inff());  // Inf or NaN
          mx = __builtin_fmaxf(mx, ax);
        }
      }
      const int ex = bad ? 0 : km_exponent(__float_as_uint(mx));
      const float up = __uint_as_float((uint32_t)(127 + 10 - ex) << 23);  // x' = x * 2^(10 - ex)
      negk[t] = -__uint_as_float((uint32_t)(127 + ex + ec - 19) << 23);   // S = |C|^2 - 2 * 2^(ex + ec - 20) * <x', C'>
      uint32_t hi[D / 2], lo[D / 2];
      km_split<D>(r, up, bad, hi, lo);
      if constexpr (D == 8) {
        bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{lo[0], lo[1], lo[2], lo[3]};
        blo[t] = bhi[t];
      } else {
        bhi[t] = h == 0 ? u32x4{hi[0], hi[1], hi[2], hi[3]} : u32x4{hi[4], hi[5], hi[6], hi[7]};
        blo[t] = h == 0 ? u32x4{lo[0], lo[1], lo[2], lo[3]} : u32x4{lo[4], lo[5], lo[6], lo[7]};
      }
    }

    // ---- the scan of this wave's share of the centroids ----
    float best_m[kKmTiles];
    int best_i[kKmTiles];
#pragma unroll
    for (int t = 0; t < kKmTiles; ++t) {
      best_m[t] = __builtin_inff();
      best_i[t] = tile0 * 32;
    }
    u32x4 ah_next = cbh[(size_t)tile0 * (32 * D / 8)], al_next = cbl[(size_t)tile0 * (32 * D / 8)];
    float4 n_next[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) n_next[q] = nr[(size_t)tile0 * 8 + 2 * q];
    for (int i = 0; i < tiles; ++i) {
      const int ct = tile0 + i;
      const u32x4 ah = ah_next, al = al_next;
      float n2[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        n2[4 * q] = n_next[q].x;
        n2[4 * q + 1] = n_next[q].y;
        n2[4 * q + 2] = n_next[q].z;
        n2[4 * q + 3] = n_next[q].w;
      }
      const int nx = i + 1 < tiles ? ct + 1 : ct;  // (the last iteration repeats its own addresses)
      ah_next = cbh[(size_t)nx * (32 * D / 8)];
      al_next = cbl[(size_t)nx * (32 * D / 8)];
#pragma unroll
      for (int q = 0; q < 4; ++q) n_next[q] = nr[(size_t)nx * 8 + 2 * q];
#pragma unroll
      for (int t = 0; t < kKmTiles; ++t) {
        km_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc = km_mfma(ah, bhi[t], acc);
        if constexpr (D == 16) acc = km_mfma(ah, blo[t], acc);
        acc = km_mfma(al, bhi[t], acc);
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
    for (int t = 0; t < kKmTiles; ++t) {
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
    const long slot = slot0 + threadIdx.x;
    if (threadIdx.x < kKmBlockPoints && slot < a.n) {
      float m = red_m[0][threadIdx.x];
      int idx = red_i[0][threadIdx.x];
#pragma unroll
      for (int k = 1; k < kKmWaves; ++k) {
        const float om = red_m[k][threadIdx.x];
        const int oi = red_i[k][threadIdx.x];
        if (om < m || (om == m && oi < idx)) {
          m = om;
          idx = oi;
        }
      }
      a.codes_out[slot] = idx;
      if constexpr (MODE != KM_NO_SUMS) {
        // ---- the point joins its cluster's sums: q_t = rint(x_t * 2^s), exact in double, round half to even ----
        float x[D];
        bool ok = true;
#pragma unroll
        for (int p = 0; p < D / 4; ++p) {
          const float4 q = reinterpret_cast<const float4*>(a.data + (size_t)slot * D)[p];
          x[4 * p] = q.x;
          x[4 * p + 1] = q.y;
          x[4 * p + 2] = q.z;
          x[4 * p + 3] = q.w;
        }
#pragma unroll
        for (int t = 0; t < D; ++t) ok = ok && (__builtin_fabsf(x[t]) <= a.data_absmax);  // false for NaN, and for Inf (data_absmax is finite)
        if (ok) {
          unsigned long long* dst = (MODE == KM_LDS ? lsum : a.sums) + (size_t)idx * D;
#pragma unroll
          for (int t = 0; t < D; ++t) {
            const long long q = __double2ll_rn((double)x[t] * a.scale);
            if (q != 0) atomicAdd(dst + t, (unsigned long long)q);
          }
          atomicAdd((MODE == KM_LDS ? lcnt : a.counts) + idx, 1);
        }
      }
    }
    __syncthreads();  // the next block of points rewrites red_m / red_i
  }

  if constexpr (MODE == KM_LDS) {
    for (int i = threadIdx.x; i < a.k * D; i += kKmThreads) {
      const unsigned long long v = lsum[i];
      if (v != 0ull) atomicAdd(a.sums + i, v);
    }
    for (int i = threadIdx.x; i < a.k; i += kKmThreads) {
      const int v = lcnt[i];
      if (v != 0) atomicAdd(a.counts + i, v);
    }
  }
}

// one thread per (c, t); grid = k * d / 256
__global__ __launch_bounds__(kKmThreads) void kmeans_update_kernel(const long long* __restrict__ sums, const int* __restrict__ counts,
                                                                   float* __restrict__ centroids, int log2_d, double inv_scale) {
  const int i = blockIdx.x * kKmThreads + threadIdx.x;
  const int count = counts[i >> log2_d];
  if (count > 0) centroids[i] = (float)((double)sums[i] * inv_scale / (double)count);
}

static bool km_shape_ok(long n, int k, int d) {
  return (d == 8 || d == 16) && k >= 128 && k <= AQLM_HIP_KMEANS_MAX_CENTROIDS && k % 128 == 0 && n >= 1 && n <= AQLM_HIP_KMEANS_MAX_POINTS;
}

static size_t km_workspace(int k, int d) { return (size_t)kKmHeaderBytes + (size_t)k * 4 + (size_t)k * d * 4; }

// s of the fixed-point unit 2^-s: min(40, 62 - ceil_log2(n)) - E, data_absmax = m * 2^E with m in [1, 2) (zero and subnormals: E = -126)
static int km_shift(long n, float data_absmax) {
  int clog2 = 0;
  while (clog2 < 62 && (1L << clog2) < n) ++clog2;
  uint32_t bits;
  memcpy(&bits, &data_absmax, 4);
  const int field = (int)((bits >> 23) & 0xffu);
  const int e = (field ? field : 1) - 127;
  const int top = 62 - clog2 < 40 ? 62 - clog2 : 40;
  return top - e;
}

static bool km_absmax_ok(float v) { return v >= 0.f && v <= 3.4028234663852886e38f; }  // finite, not negative, not NaN

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_kmeans_supported(long n, int k, int d) { return km_shape_ok(n, k, d) ? 1 : 0; }

extern "C" size_t aqlm_hip_kmeans_workspace_bytes(long n, int k, int d) { return km_shape_ok(n, k, d) ? km_workspace(k, d) : 0; }

extern "C" int aqlm_hip_kmeans_assign(const void* data, long n, const void* centroids, int k, int d, float data_absmax, void* codes_out,
                                      void* sums_out, void* counts_out, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_kmeans_assign";
  if (int e = check_not_null(who, data && centroids && codes_out && workspace && (!sums_out == !counts_out))) return e;
  if (int e = check_aligned(who, "data / centroids / codes_out / sums_out / counts_out / workspace",
                            aligned16(data) && aligned16(centroids) && aligned4(codes_out) && aligned8(sums_out) && aligned4(counts_out) &&
                                aligned16(workspace)))
    return e;
  if (n < 1 || k < 1 || d < 1 || !km_absmax_ok(data_absmax)) {
    set_last_error("%s: bad sizes (n=%ld k=%d d=%d), or data_absmax %g is negative or not finite", who, n, k, d, (double)data_absmax);
    return AQLM_HIP_E_INVALID;
  }
  if (!km_shape_ok(n, k, d)) {
    set_last_error("%s: shape outside the kernel (d 8 or 16, k a multiple of 128 up to 65536, n below 2^31; got n=%ld k=%d d=%d)", who, n, k, d);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t need = km_workspace(k, d);
  if (workspace_bytes < need) {
    set_last_error("%s: a workspace of %zu bytes where %zu bytes are needed", who, workspace_bytes, need);
    return AQLM_HIP_E_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  unsigned char* ws = (unsigned char*)workspace;
  KmeansArgs a{};
  a.data = (const float*)data;
  a.header = (const uint32_t*)ws;
  a.norms = (const float*)(ws + kKmHeaderBytes);
  a.chi = (const uint16_t*)(ws + kKmHeaderBytes + (size_t)k * 4);
  a.clo = a.chi + (size_t)k * d;
  a.codes_out = (int*)codes_out;
  a.sums = (unsigned long long*)sums_out;
  a.counts = (int*)counts_out;
  a.scale = ldexp(1.0, km_shift(n, data_absmax));
  a.data_absmax = data_absmax;
  a.n = n;
  a.num_blocks = (n + kKmBlockPoints - 1) / kKmBlockPoints;
  a.k = k;
  if (int e = check_hip(hipMemsetAsync(ws, 0, kKmHeaderBytes, stream), "kmeans header memset")) return e;
  if (sums_out) {
    if (int e = check_hip(hipMemsetAsync(sums_out, 0, (size_t)k * d * 8, stream), "kmeans sums memset")) return e;
    if (int e = check_hip(hipMemsetAsync(counts_out, 0, (size_t)k * 4, stream), "kmeans counts memset")) return e;
  }
  const long elems = (long)k * d;
  const unsigned max_blocks = (unsigned)((elems + kKmThreads - 1) / kKmThreads);
  hipLaunchKernelGGL(kmeans_absmax_kernel, dim3(max_blocks < 256u ? max_blocks : 256u), dim3(kKmThreads), 0, stream, (const float*)centroids,
                     elems, (uint32_t*)ws);
  if (int e = check_hip(hipGetLastError(), "kmeans_absmax launch")) return e;
  const int mode = !sums_out ? KM_NO_SUMS : ((size_t)k * d * 8 <= (size_t)kKmLdsSumBytes ? KM_LDS : KM_DIRECT);
  const size_t lds = (size_t)kKmRedBytes + (mode == KM_LDS ? (size_t)k * d * 8 + (size_t)k * 4 : 0);
  const unsigned blocks = (unsigned)(mode == KM_LDS && a.num_blocks > kKmLdsGrid ? kKmLdsGrid : a.num_blocks);
  auto run = [&](auto dim) -> int {
    constexpr int D = decltype(dim)::value;
    hipLaunchKernelGGL((kmeans_split_kernel<D>), dim3(k / 128), dim3(128), 0, stream, (const float*)centroids, a.header, (float*)a.norms,
                       (uint16_t*)a.chi, (uint16_t*)a.clo);
    if (int e = check_hip(hipGetLastError(), "kmeans_split launch")) return e;
    auto launch = [&](auto kernel) -> int {
      if (int e = ensure_dynamic_lds((const void*)kernel, lds)) return e;
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kKmThreads), lds, stream, a);
      return check_hip(hipGetLastError(), "kmeans_assign launch");
    };
    if (mode == KM_NO_SUMS) return launch(kmeans_assign_kernel<D, KM_NO_SUMS>);
    if (mode == KM_LDS) return launch(kmeans_assign_kernel<D, KM_LDS>);
    return launch(kmeans_assign_kernel<D, KM_DIRECT>);
  };
  return d == 8 ? run(std::integral_constant<int, 8>{}) : run(std::integral_constant<int, 16>{});
}

extern "C" int aqlm_hip_kmeans_update(const void* sums, const void* counts, long n, int k, int d, float data_absmax, void* centroids_inout,
                                      void* stream_) {
  static const char* who = "aqlm_hip_kmeans_update";
  if (int e = check_not_null(who, sums && counts && centroids_inout)) return e;
  if (int e = check_aligned(who, "sums / counts / centroids_inout", aligned8(sums) && aligned4(counts) && aligned4(centroids_inout))) return e;
  if (n < 1 || k < 1 || d < 1 || !km_absmax_ok(data_absmax)) {
    set_last_error("%s: bad sizes (n=%ld k=%d d=%d), or data_absmax %g is negative or not finite", who, n, k, d, (double)data_absmax);
    return AQLM_HIP_E_INVALID;
  }
  if (!km_shape_ok(n, k, d)) {
    set_last_error("%s: shape outside the kernel (d 8 or 16, k a multiple of 128 up to 65536, n below 2^31; got n=%ld k=%d d=%d)", who, n, k, d);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((long)k * d / kKmThreads)), dim3(kKmThreads), 0, (hipStream_t)stream_,
                     (const long long*)sums, (const int*)counts, (float*)centroids_inout, d == 8 ? 3 : 4, ldexp(1.0, -km_shift(n, data_absmax)));
  return check_hip(hipGetLastError(), "kmeans_update launch");
}

// One step of the calibrated training of codebooks and scales (the reference's AQEngine._compute_mse, aq_engine.py:108-131, and its
// backward), on fp32 master parameters: codebooks [K][S][g], scales [out], canonical codes (int16 [out][in / g] for 1x16, int8
// [out][in / g][K] for K x 8), out_group_size 1.  With D = W_q - W_ref and G = D XTX (XTX symmetric; one library GEMM between the
// first entry and the others):
//     loss = sum_o rowloss[o] / out,   d loss / d s[o] = 2 / out * ds_raw[o],   d loss / d C = 2 / out * dC
//   aqlm_hip_calib_delta               D[o][j*g + t] = s[o] * w_j[t] - W_ref[o][j*g + t],  w_j[t] = ((C_0[v_0][t] + C_1[v_1][t]) + ...):
//                                      every operation one fp32 operation (no contraction), so D equals torch's fp32
//                                      `_dequantize_weight(...) - W_ref` bit for bit; a thread per 16-byte piece of D
//   aqlm_hip_calib_rows                ds_raw[o] = sum G * w,  rowloss[o] = sum G * D (the stored D): a wave per row, the order of
//                                      scales_grad_kernel
//   aqlm_hip_calib_codebook_grad_1x16  the kernels of aqlm_hip_codebook_grad_1x16 (codebook_grad_body.h) on fp32 G and fp32 scales
//   aqlm_hip_calib_codebook_grad_kx8   the kernels of aqlm_hip_codebook_grad_kx8 (codebook_grad_kx8_body.h) likewise
// The fp32 codebooks of a K x 8 layer are staged in LDS where they fit 64 KiB (1x8 / 2x8 g8 ... 8x8 g8, 4x8 g16); an 8x8 g32 table
// (256 KiB) and the 1x16 table (2 / 4 MiB) are gathered from L2 in 16-byte pieces.  No kernel applies the factor 2 / out.
#include "codebook_grad_body.h"
#include "codebook_grad_kx8_body.h"

namespace aqlm {

constexpr int kCalThreads = 256;
constexpr size_t kCalLdsBytes = 64 * 1024;  // codebooks up to here are staged (the default dynamic-LDS limit)

struct CalibArgs {
  const void* codes;       // int16 [M][nj] or int8 [M][nj][K]
  const float* codebooks;  // [K][S][G]
  const float* scales;     // [M]
  const void* wref;        // [M][..] in wref_dtype
  float* d;                // [M][..]; read by the rows kernel
  const float* gmat;       // [M][..]
  float* ds_raw;           // [M]
  float* rowloss;          // [M]
  long wrs, dstride, gstride;  // row strides, elements
  int M;
  int nj;  // in_features / g
  int K;
  int wref_dtype;
};

// w_j[t0 .. t0 + 3] of position `pos` = o * nj + j: the entries summed in fp32 in codebook order
template <int G, bool WIDE>
static __device__ __forceinline__ void calib_w4(const float* cb, const void* codes, size_t pos, int K, int t0, float (&w)[4]) {
  if constexpr (WIDE) {
    const uint32_t c = reinterpret_cast<const uint16_t*>(codes)[pos];
    const float4 f = *reinterpret_cast<const float4*>(cb + (size_t)c * G + t0);
    w[0] = f.x;
    w[1] = f.y;
    w[2] = f.z;
    w[3] = f.w;
  } else {
    const uint8_t* cp = reinterpret_cast<const uint8_t*>(codes) + pos * (size_t)K;
#pragma unroll
    for (int c = 0; c < kKx8MaxK; ++c) {
      if (c < K) {
        const float4 f = *reinterpret_cast<const float4*>(cb + ((size_t)(c * kKx8Entries) + cp[c]) * G + t0);
        w[0] = c == 0 ? f.x : w[0] + f.x;
        w[1] = c == 0 ? f.y : w[1] + f.y;
        w[2] = c == 0 ? f.z : w[2] + f.z;
        w[3] = c == 0 ? f.w : w[3] + f.w;
      }
    }
  }
}

// the codebooks into LDS, 16 bytes per thread and step (K * 256 * G * 4 bytes: a multiple of 16)
template <int G>
static __device__ __forceinline__ void calib_stage(float* lds, const float* codebooks, int K) {
  const float4* src = reinterpret_cast<const float4*>(codebooks);
  float4* dst = reinterpret_cast<float4*>(lds);
  for (int i = threadIdx.x; i < K * kKx8Entries * G / 4; i += kCalThreads) dst[i] = src[i];
  __syncthreads();
}

// rows grid-stride over the workgroups; a thread per 16-byte piece of the row
template <int G, bool WIDE, bool LDS>
__global__ __launch_bounds__(kCalThreads) void calib_delta_kernel(CalibArgs a) {
  extern __shared__ __attribute__((aligned(16))) float calib_cb[];
  const float* cb = a.codebooks;
  if constexpr (LDS) {
    calib_stage<G>(calib_cb, a.codebooks, a.K);
    cb = calib_cb;
  }
  const int pieces = a.nj * (G / 4);
  for (int o = blockIdx.x; o < a.M; o += gridDim.x) {
    const float s = a.scales[o];
    for (int q = threadIdx.x; q < pieces; q += kCalThreads) {
      const int j = q / (G / 4), t0 = (q % (G / 4)) * 4;
      float w[4], r[4];
      calib_w4<G, WIDE>(cb, a.codes, (size_t)o * a.nj + j, a.K, t0, w);
      const size_t col = (size_t)q * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = load_ref(a.wref, (size_t)o * (size_t)a.wrs + col + e, a.wref_dtype);
      float4 out;
      // a multiply, then a subtract, as torch runs them: the products pass through an empty asm so that they cannot be contracted
      // into fused multiply-adds (the build's -ffp-contract=fast fuses in the back end, past any pragma)
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = s * w[e];
        asm volatile("" : "+v"(p[e]));
      }
      out.x = p[0] - r[0];
      out.y = p[1] - r[1];
      out.z = p[2] - r[2];
      out.w = p[3] - r[3];
      *reinterpret_cast<float4*>(a.d + (size_t)o * (size_t)a.dstride + col) = out;
    }
  }
}

// one wave per row, rows grid-stride: lane l takes the groups l, l + 64 ... of the row and adds their products over t ascending
// (fused multiply-add) into two fp32 registers; wave_sum adds the lanes.  Which wave takes a row does not enter the order.
template <int G, bool WIDE, bool LDS>
__global__ __launch_bounds__(kCalThreads) void calib_rows_kernel(CalibArgs a) {
  extern __shared__ __attribute__((aligned(16))) float calib_cb[];
  const float* cb = a.codebooks;
  if constexpr (LDS) {
    calib_stage<G>(calib_cb, a.codebooks, a.K);
    cb = calib_cb;
  }
  const int l = threadIdx.x & (WAVE - 1);
  const int waves = gridDim.x * (kCalThreads / WAVE);
  for (int o = blockIdx.x * (kCalThreads / WAVE) + (int)(threadIdx.x / WAVE); o < a.M; o += waves) {  // wave-uniform
    const float* grow = a.gmat + (size_t)o * (size_t)a.gstride;
    const float* drow = a.d + (size_t)o * (size_t)a.dstride;
    float ds = 0.f, rl = 0.f;
    for (int j = l; j < a.nj; j += WAVE) {
#pragma unroll
      for (int p = 0; p < G / 4; ++p) {
        float w[4];
        calib_w4<G, WIDE>(cb, a.codes, (size_t)o * a.nj + j, a.K, p * 4, w);
        const float4 gv = *reinterpret_cast<const float4*>(grow + (size_t)j * G + p * 4);
        const float4 dv = *reinterpret_cast<const float4*>(drow + (size_t)j * G + p * 4);
        ds = __builtin_fmaf(gv.x, w[0], ds);
        ds = __builtin_fmaf(gv.y, w[1], ds);
        ds = __builtin_fmaf(gv.z, w[2], ds);
        ds = __builtin_fmaf(gv.w, w[3], ds);
        rl = __builtin_fmaf(gv.x, dv.x, rl);
        rl = __builtin_fmaf(gv.y, dv.y, rl);
        rl = __builtin_fmaf(gv.z, dv.z, rl);
        rl = __builtin_fmaf(gv.w, dv.w, rl);
      }
    }
    ds = wave_sum(ds);
    rl = wave_sum(rl);
    if (l == 0) {
      a.ds_raw[o] = ds;
      a.rowloss[o] = rl;
    }
  }
}

// the scheme of a calibrated entry: one codebook of 16 bits with g 8 / 16, or 1..8 codebooks of 8 bits with g 8 / 16 / 32
static bool calib_shape_ok(int out_features, int in_features, int K, int nbits, int g) {
  if (nbits == 16) return K == 1 && cg_shape_ok(out_features, in_features, g);
  return nbits == 8 && kx8_shape_ok(out_features, in_features, K, g);
}

// the checks the delta and rows entries share after the pointers; `stride_ok`: every row stride reaches in_features; `ref_dtype`:
// W_ref's (the rows entry has none: fp32)
static int calib_check_shape(const char* who, bool stride_ok, int ref_dtype, int out_features, int in_features, int K, int nbits, int g,
                             bool rows_aligned) {
  if (int e = check_sizes(who, out_features, in_features, g)) return e;
  if (!stride_ok) {
    set_last_error("%s: bad sizes (a row stride below in_features %d)", who, in_features);
    return AQLM_HIP_E_INVALID;
  }
  if (!dw_dtype_ok(ref_dtype)) {
    set_last_error("%s: W_ref is float16, bfloat16 or float32 (dtype id %d)", who, ref_dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (nbits != 8 && nbits != 16) {
    set_last_error("%s: codebooks of 256 or 65536 entries are supported, got %d bits", who, nbits);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (nbits == 16 ? K != 1 : (K < 1 || K > kKx8MaxK)) {
    set_last_error("%s: one codebook of 65536 entries or 1 to %d codebooks of 256 entries are supported, got %d x %d bits", who, kKx8MaxK, K,
                   nbits);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (g != 8 && g != 16 && !(nbits == 8 && g == 32)) {
    set_last_error("%s: only codebooks with 8 or 16 features (256 entries: 32 too) are supported, got %d", who, g);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (!calib_shape_ok(out_features, in_features, K, nbits, g) || !rows_aligned) {
    set_last_error("%s: shape outside the kernel (fewer than 2^30 positions, fp32 rows 16-byte aligned; got out=%d in=%d g=%d)", who,
                   out_features, in_features, g);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return 0;
}

// f(GroupSize<g>{}, wide, staged) for a checked scheme
template <class F>
static int calib_dispatch(int K, int nbits, int g, F&& f) {
  if (nbits == 16) return g == 8 ? f(GroupSize<8>{}, std::true_type{}, std::false_type{}) : f(GroupSize<16>{}, std::true_type{}, std::false_type{});
  const bool staged = (size_t)K * kKx8Entries * (size_t)g * 4 <= kCalLdsBytes;
  auto by_stage = [&](auto gs) { return staged ? f(gs, std::false_type{}, std::true_type{}) : f(gs, std::false_type{}, std::false_type{}); };
  if (g == 8) return by_stage(GroupSize<8>{});
  if (g == 16) return by_stage(GroupSize<16>{});
  return by_stage(GroupSize<32>{});
}

static size_t calib_lds_bytes(int K, int nbits, int g) {
  const size_t bytes = (size_t)K * kKx8Entries * (size_t)g * 4;
  return nbits == 8 && bytes <= kCalLdsBytes ? bytes : 0;
}

}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_calib_delta_supported(int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size) {
  return calib_shape_ok(out_features, in_features, num_codebooks, nbits_per_codebook, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_calib_delta(const void* codes, const void* codebooks, const void* scales, const void* w_ref, int w_ref_dtype,
                                    long w_ref_row_stride, int out_features, int in_features, int num_codebooks, int nbits_per_codebook,
                                    int in_group_size, void* d, long d_row_stride, void* stream_) {
  static const char* who = "aqlm_hip_calib_delta";
  if (int e = check_not_null(who, codes && codebooks && scales && w_ref && d)) return e;
  if (int e = check_aligned(who, "codes / codebooks / scales / w_ref / d",
                            (nbits_per_codebook == 16 ? aligned2(codes) : true) && aligned16(codebooks) && aligned4(scales) &&
                                ref_aligned(w_ref, w_ref_dtype) && aligned16(d)))
    return e;
  if (int e = calib_check_shape(who, w_ref_row_stride >= in_features && d_row_stride >= in_features, w_ref_dtype, out_features, in_features,
                                num_codebooks, nbits_per_codebook, in_group_size, d_row_stride % 4 == 0))
    return e;
  CalibArgs a{};
  a.codes = codes;
  a.codebooks = (const float*)codebooks;
  a.scales = (const float*)scales;
  a.wref = w_ref;
  a.d = (float*)d;
  a.wrs = w_ref_row_stride;
  a.dstride = d_row_stride;
  a.M = out_features;
  a.nj = in_features / in_group_size;
  a.K = num_codebooks;
  a.wref_dtype = w_ref_dtype;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t lds = calib_lds_bytes(num_codebooks, nbits_per_codebook, in_group_size);
  const dim3 grid(std::min(out_features, 2048));
  return calib_dispatch(num_codebooks, nbits_per_codebook, in_group_size, [&](auto gs, auto wide, auto staged) {
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((calib_delta_kernel<G, decltype(wide)::value, decltype(staged)::value>), grid, dim3(kCalThreads), lds, stream, a);
    return check_hip(hipGetLastError(), "calib_delta launch");
  });
}

extern "C" int aqlm_hip_calib_rows_supported(int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size) {
  return calib_shape_ok(out_features, in_features, num_codebooks, nbits_per_codebook, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_calib_rows(const void* g, long g_row_stride, const void* d, long d_row_stride, const void* codes, const void* codebooks,
                                   int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size,
                                   void* ds_raw, void* rowloss, void* stream_) {
  static const char* who = "aqlm_hip_calib_rows";
  if (int e = check_not_null(who, g && d && codes && codebooks && ds_raw && rowloss)) return e;
  if (int e = check_aligned(who, "g / d / codes / codebooks / ds_raw / rowloss",
                            aligned16(g) && aligned16(d) && (nbits_per_codebook == 16 ? aligned2(codes) : true) && aligned16(codebooks) &&
                                aligned4(ds_raw) && aligned4(rowloss)))
    return e;
  if (int e = calib_check_shape(who, g_row_stride >= in_features && d_row_stride >= in_features, AQLM_HIP_F32, out_features, in_features,
                                num_codebooks, nbits_per_codebook, in_group_size, g_row_stride % 4 == 0 && d_row_stride % 4 == 0))
    return e;
  CalibArgs a{};
  a.codes = codes;
  a.codebooks = (const float*)codebooks;
  a.d = (float*)d;
  a.gmat = (const float*)g;
  a.ds_raw = (float*)ds_raw;
  a.rowloss = (float*)rowloss;
  a.dstride = d_row_stride;
  a.gstride = g_row_stride;
  a.M = out_features;
  a.nj = in_features / in_group_size;
  a.K = num_codebooks;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t lds = calib_lds_bytes(num_codebooks, nbits_per_codebook, in_group_size);
  const int per_block = kCalThreads / WAVE;
  // with a staged table as many workgroups as stay resident on the 256 CUs beside it, at most one wave per row
  const int per_cu = lds ? (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + 1024))) : 8;
  const dim3 grid(std::min((out_features + per_block - 1) / per_block, 256 * per_cu));
  return calib_dispatch(num_codebooks, nbits_per_codebook, in_group_size, [&](auto gs, auto wide, auto staged) {
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((calib_rows_kernel<G, decltype(wide)::value, decltype(staged)::value>), grid, dim3(kCalThreads), lds, stream, a);
    return check_hip(hipGetLastError(), "calib_rows launch");
  });
}

extern "C" int aqlm_hip_calib_codebook_grad_1x16_supported(int out_features, int in_features, int in_group_size) {
  return cg_shape_ok(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" size_t aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(int out_features, int in_features, int in_group_size) {
  if (!cg_shape_ok(out_features, in_features, in_group_size)) return 0;
  return (size_t)cg_max_chunks(out_features, in_features, in_group_size) * (size_t)in_group_size * 4;
}

extern "C" int aqlm_hip_calib_codebook_grad_1x16(const void* g, long g_row_stride, const void* scales, const void* starts, const void* order,
                                                 const void* chunks, const void* chunk_starts, int out_features, int in_features,
                                                 int in_group_size, void* out, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_calib_codebook_grad_1x16";
  if (int e = check_not_null(who, g && scales && starts && order && chunks && chunk_starts && out && workspace)) return e;
  if (int e = check_aligned(who, "g / scales / index / out / workspace",
                            aligned16(g) && aligned4(scales) && aligned4(starts) && aligned4(order) && aligned4(chunks) &&
                                aligned4(chunk_starts) && aligned16(out) && aligned16(workspace)))
    return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  const bool shape_ok = cg_shape_ok(out_features, in_features, in_group_size);
  const size_t need = shape_ok ? (size_t)cg_max_chunks(out_features, in_features, in_group_size) * (size_t)in_group_size * 4 : 0;
  if (g_row_stride < in_features || workspace_bytes < need) {
    set_last_error("%s: bad sizes (G row stride %ld < in_features %d, or a workspace of %zu bytes where %zu bytes are needed)", who,
                   g_row_stride, in_features, workspace_bytes, need);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_group_size(who, in_group_size)) return e;
  if (!shape_ok || g_row_stride % 4 != 0) {
    set_last_error("%s: shape outside the kernel (at most %d codes, G rows 16-byte aligned; got out=%d in=%d g=%d, row stride %ld)", who,
                   AQLM_HIP_CODEBOOK_GRAD_MAX_CODES, out_features, in_features, in_group_size, g_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return cg_codebook_grad_launch(g, g_row_stride, AQLM_HIP_F32, scales, AQLM_HIP_F32, starts, order, chunks, chunk_starts, out_features,
                                 in_features, in_group_size, out, AQLM_HIP_F32, workspace, (hipStream_t)stream_);
}

extern "C" int aqlm_hip_calib_codebook_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size) {
  return kx8_shape_ok(out_features, in_features, num_codebooks, in_group_size) ? 1 : 0;
}

extern "C" size_t aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(int out_features, int in_features, int num_codebooks, int in_group_size) {
  if (!kx8_shape_ok(out_features, in_features, num_codebooks, in_group_size)) return 0;
  return kx8_workspace_bytes(out_features, num_codebooks, in_group_size);
}

extern "C" int aqlm_hip_calib_codebook_grad_kx8(const void* g, long g_row_stride, const void* scales, const void* codes, int out_features,
                                                int in_features, int num_codebooks, int in_group_size, void* out, void* workspace,
                                                size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_calib_codebook_grad_kx8";
  if (int e = check_not_null(who, g && scales && codes && out && workspace)) return e;
  if (int e = check_aligned(who, "g / scales / out / workspace", aligned16(g) && aligned4(scales) && aligned16(out) && aligned16(workspace)))
    return e;
  // (the scales' dtype is fixed here: the fp16 id passes the sibling's dtype check, which has nothing to refuse)
  if (int e = kx8_check_shape(who, g_row_stride, AQLM_HIP_F32, AQLM_HIP_F16, out_features, in_features, num_codebooks, in_group_size,
                              AQLM_HIP_F32, true, workspace_bytes))
    return e;
  return kx8_codebook_grad_launch(g, g_row_stride, AQLM_HIP_F32, scales, AQLM_HIP_F32, codes, out_features, in_features, num_codebooks,
                                  in_group_size, out, AQLM_HIP_F32, workspace, (hipStream_t)stream_);
}

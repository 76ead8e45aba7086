// Gradients of the continuous parameters of a 1x16 layer (one codebook of 65536 entries, out_group_size 1, g = 8 / 16) from
// dW = grad_y^T @ x [out][in]:
//     dC[c][t] = sum over the positions (o, j) with code(o, j) == c of s[o] * dW[o, j*g + t]        (aqlm_hip_codebook_grad_1x16)
//     ds[o]    = sum over j, t of dW[o, j*g + t] * C[code(o, j)][t]                                 (aqlm_hip_scales_grad_1x16)
// dC is a scatter-add of out * in / g short vectors into 65536 destinations.  The codes are fixed while codebooks and scales
// train, so the scatter is turned round once per layer into an inverted index (per entry the ascending list of its positions,
// cut into chunks of at most kCgChunk positions) and the gradient becomes a gather and a sum in a fixed order: no atomics, no
// arrival order, reproducible bits.
//
// Summation tree of dC -- a function of the index and the two constants alone, never of the grid or of timing:
//   * a chunk is summed by kCgLanes = 16 lanes (one DPP row; 4 chunks per wave, 16 per workgroup): lane l adds the chunk's
//     positions l, l + 16, l + 32 ... in that order into g fp32 registers (s[o] * dW, fused multiply-add), then the 16 lanes are
//     added by the fixed butterfly of row16_sum;
//   * an entry of one chunk writes that sum; an entry of several chunks has its fp32 partials (workspace, one row per chunk)
//     added in chunk order by the second launch, which also writes +0 for every entry that no position uses.
#include "codebook_grad_body.h"

using namespace aqlm;

extern "C" int aqlm_hip_codebook_grad_chunk(void) { return kCgChunk; }

extern "C" int aqlm_hip_codebook_grad_1x16_supported(int out_features, int in_features, int in_group_size) {
  return cg_shape_ok(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_codebook_grad_1x16_max_chunks(int out_features, int in_features, int in_group_size) {
  return cg_shape_ok(out_features, in_features, in_group_size) ? (int)cg_max_chunks(out_features, in_features, in_group_size) : 0;
}

extern "C" size_t aqlm_hip_codebook_grad_1x16_workspace_bytes(int out_features, int in_features, int in_group_size) {
  if (!cg_shape_ok(out_features, in_features, in_group_size)) return 0;
  return (size_t)cg_max_chunks(out_features, in_features, in_group_size) * (size_t)in_group_size * 4;
}

extern "C" int aqlm_hip_codebook_grad_1x16(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int dtype,
                                           const void* starts, const void* order, const void* chunks, const void* chunk_starts,
                                           int out_features, int in_features, int in_group_size, void* out, int out_dtype,
                                           void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_codebook_grad_1x16";
  if (int e = check_not_null(who, dw && starts && order && chunks && chunk_starts && out && workspace)) return e;
  if (int e = check_aligned(who, "dw / scales / index / out / workspace",
                            aligned16(dw) && aligned2(scales) && aligned4(starts) && aligned4(order) && aligned4(chunks) &&
                                aligned4(chunk_starts) && aligned16(out) && aligned16(workspace)))
    return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  const bool shape_ok = cg_shape_ok(out_features, in_features, in_group_size);
  const size_t need = shape_ok ? (size_t)cg_max_chunks(out_features, in_features, in_group_size) * (size_t)in_group_size * 4 : 0;
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
  if (int e = check_group_size(who, in_group_size)) return e;
  if (!shape_ok || ((size_t)dw_row_stride * dtype_bytes(dw_dtype)) % 16 != 0) {
    set_last_error("%s: shape outside the kernel (at most %d codes, dW rows 16-byte aligned; got out=%d in=%d g=%d, row stride %ld)",
                   who, AQLM_HIP_CODEBOOK_GRAD_MAX_CODES, out_features, in_features, in_group_size, dw_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return cg_codebook_grad_launch(dw, dw_row_stride, dw_dtype, scales, dtype, starts, order, chunks, chunk_starts, out_features, in_features,
                                 in_group_size, out, out_dtype, workspace, (hipStream_t)stream_);
}

extern "C" int aqlm_hip_scales_grad_1x16_supported(int out_features, int in_features, int in_group_size) {
  return cg_shape_ok(out_features, in_features, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_scales_grad_1x16(const void* dw, long dw_row_stride, int dw_dtype, const void* codes, const void* codebook,
                                         int dtype, int out_features, int in_features, int in_group_size, void* out, int out_dtype,
                                         void* stream_) {
  static const char* who = "aqlm_hip_scales_grad_1x16";
  if (int e = check_not_null(who, dw && codes && codebook && out)) return e;
  if (int e = check_aligned(who, "dw / codes / codebook / out", aligned16(dw) && aligned2(codes) && aligned16(codebook) && aligned4(out)))
    return e;
  if (int e = check_sizes(who, out_features, in_features, in_group_size)) return e;
  if (dw_row_stride < in_features) {
    set_last_error("%s: bad sizes (dW row stride %ld < in_features %d)", who, dw_row_stride, in_features);
    return AQLM_HIP_E_INVALID;
  }
  if (!dw_dtype_ok(dw_dtype) || !dw_dtype_ok(out_dtype)) {
    set_last_error("%s: dW and the output are float16, bfloat16 or float32 (dtype ids %d, %d)", who, dw_dtype, out_dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_group_size(who, in_group_size)) return e;
  if (!cg_shape_ok(out_features, in_features, in_group_size) || ((size_t)dw_row_stride * dtype_bytes(dw_dtype)) % 16 != 0) {
    set_last_error("%s: shape outside the kernel (at most %d codes, dW rows 16-byte aligned; got out=%d in=%d g=%d, row stride %ld)",
                   who, AQLM_HIP_CODEBOOK_GRAD_MAX_CODES, out_features, in_features, in_group_size, dw_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  ScalesGradArgs a{};
  a.dw = dw;
  a.codes = (const uint16_t*)codes;
  a.codebook = (const uint16_t*)codebook;
  a.out = out;
  a.dws = dw_row_stride;
  a.M = out_features;
  a.nj = in_features / in_group_size;
  a.cb_bf16 = dtype == AQLM_HIP_BF16;
  a.out_dtype = out_dtype;
  hipStream_t stream = (hipStream_t)stream_;
  const int per_block = kCgThreads / WAVE;
  const dim3 grid((out_features + per_block - 1) / per_block);
  return dispatch_dw_group(dw_dtype, in_group_size, [&](auto dwt, auto gs) {
    using DW = decltype(dwt);
    constexpr int G = decltype(gs)::value;
    hipLaunchKernelGGL((scales_grad_kernel<DW, G>), grid, dim3(kCgThreads), 0, stream, a);
    return check_hip(hipGetLastError(), "scales_grad launch");
  });
}

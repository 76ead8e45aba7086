// Gradients of the continuous parameters of a K x 8 layer (K = 1..8 codebooks of 256 entries, out_group_size 1, g = 8 / 16 / 32)
// from dW = grad_y^T @ x [out][in]:
//     dC[c][v][t] = sum over the positions (o, j) with code(o, j, c) == v of s[o] * dW[o, j*g + t]   (aqlm_hip_codebook_grad_kx8)
//     ds[o]       = sum over j, t of dW[o, j*g + t] * (C_0[v_0][t] + C_1[v_1][t] + ...)               (aqlm_hip_scales_grad_kx8)
// A K x 8 codebook gradient is K * 256 * g numbers: it lives in LDS while a workgroup streams its rows of dW once, coalesced --
// no inverted index (every list would hold thousands of positions and every position would sit in K lists).  The scatter-add
// into LDS is made order-independent by taking the sums as FIXED-POINT INTEGERS (include/aqlm_hip.h has the arithmetic): integer
// adds commute, so LDS atomics (ds_add_u64, two's-complement wrap = the signed sum) give the same bits under any schedule, and
// the sum of the quantised terms is exact.  No float atomics anywhere.
//
// Launches of the codebook gradient:
//   1. maxima      up to 1024 workgroups, each over a block of rows: max|dW| and max|s| of its rows as fp32 bit patterns (a pattern
//                  >= 0x7f800000 is an Inf or a NaN: the exponent bits tell, fmaxf would drop a NaN), two words per block in the
//                  workspace;
//   2. accumulate  grid = row blocks x codebook passes (64 / g codebooks per pass: the int64 image [KS][256][g] is at most
//                  128 KiB): zero the image, reduce the block maxima to the exponent E, stream the rows -- per position one
//                  group of dW in 16-byte pieces, the code bytes, the exact double product, llrint, ds_add_u64 -- and write the
//                  image to the workspace with plain stores;
//   3. finish      one thread per output element and quarter of the row blocks adds the int64 partials (any order: the same
//                  bits), converts and stores; it also writes the NaN / +0 special cases.
// The image rows are padded by one int64 in LDS (entry stride g + 1): without it the entries of a codebook start at only four
// distinct banks for g = 8.
#include "codebook_grad_kx8_body.h"

using namespace aqlm;

extern "C" int aqlm_hip_codebook_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size) {
  return kx8_shape_ok(out_features, in_features, num_codebooks, in_group_size) ? 1 : 0;
}

extern "C" size_t aqlm_hip_codebook_grad_kx8_workspace_bytes(int out_features, int in_features, int num_codebooks, int in_group_size) {
  if (!kx8_shape_ok(out_features, in_features, num_codebooks, in_group_size)) return 0;
  return kx8_workspace_bytes(out_features, num_codebooks, in_group_size);
}

extern "C" int aqlm_hip_codebook_grad_kx8(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int dtype,
                                          const void* codes, int out_features, int in_features, int num_codebooks, int in_group_size,
                                          void* out, int out_dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_codebook_grad_kx8";
  if (int e = check_not_null(who, dw && codes && out && workspace)) return e;
  if (int e = check_aligned(who, "dw / scales / out / workspace", aligned16(dw) && aligned2(scales) && aligned16(out) && aligned16(workspace)))
    return e;
  if (int e = kx8_check_shape(who, dw_row_stride, dw_dtype, dtype, out_features, in_features, num_codebooks, in_group_size, out_dtype, true,
                              workspace_bytes))
    return e;
  return kx8_codebook_grad_launch(dw, dw_row_stride, dw_dtype, scales, dtype, codes, out_features, in_features, num_codebooks, in_group_size,
                                  out, out_dtype, workspace, (hipStream_t)stream_);
}

extern "C" int aqlm_hip_scales_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size) {
  return kx8_shape_ok(out_features, in_features, num_codebooks, in_group_size) ? 1 : 0;
}

extern "C" int aqlm_hip_scales_grad_kx8(const void* dw, long dw_row_stride, int dw_dtype, const void* codes, const void* codebooks,
                                        int dtype, int out_features, int in_features, int num_codebooks, int in_group_size, void* out,
                                        int out_dtype, void* stream_) {
  static const char* who = "aqlm_hip_scales_grad_kx8";
  if (int e = check_not_null(who, dw && codes && codebooks && out)) return e;
  if (int e = check_aligned(who, "dw / codebooks / out", aligned16(dw) && aligned16(codebooks) && aligned4(out))) return e;
  if (int e = kx8_check_shape(who, dw_row_stride, dw_dtype, dtype, out_features, in_features, num_codebooks, in_group_size, out_dtype, false,
                              0))
    return e;
  Kx8ScalesGradArgs a{};
  a.dw = dw;
  a.codes = (const uint8_t*)codes;
  a.codebooks = (const uint16_t*)codebooks;
  a.out = out;
  a.dws = dw_row_stride;
  a.M = out_features;
  a.nj = in_features / in_group_size;
  a.K = num_codebooks;
  a.cb_bf16 = dtype == AQLM_HIP_BF16;
  a.out_dtype = out_dtype;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t lds = (size_t)num_codebooks * kKx8Entries * (size_t)in_group_size * 2;
  // as many workgroups as stay resident on the 256 CUs beside their codebook image, at most one wave per row
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / (lds + 1024)));
  const int per_block = kKx8Threads / WAVE;
  const dim3 grid(std::min((out_features + per_block - 1) / per_block, 256 * per_cu));
  return kx8_dispatch(dw_dtype, in_group_size, [&](auto dwt, auto gs) {
    using DW = decltype(dwt);
    constexpr int G = decltype(gs)::value;
    auto kern = &scales_grad_kx8_kernel<DW, G>;
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(kKx8Threads), lds, stream, a);
    return check_hip(hipGetLastError(), "scales_grad_kx8 launch");
  });
}

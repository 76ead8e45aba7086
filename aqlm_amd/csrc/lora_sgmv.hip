// Segmented LoRA adapter GEMM on top of a quantized layer's output at any row count (aqlm_hip_lora_sgmv), gfx950, wave64: the
// prefill counterpart of the per-row matvec of lora_bgmv.hip, on v_mfma_f32_16x16x32_{f16,bf16}.
//
// For every row b < rows with adapter a = ids[b] (include/aqlm_hip.h states the definition):
//     t[b, r] = sum_k A_a[r, k] * x[b, k]                                    r < rank_a, fp32
//     hi = round_T(t), lo = round_T(t - float(hi))                           T = the storage type
//     y[b, i] = round_T(float(y[b, i]) + scaling_a * sum_r B_a[i, r] * (hi[b, r] + lo[b, r]))
// in two launches whose grids depend on rows, max_rank, in_features and out_features only: the ids stay on the device, nothing is
// synchronised or allocated, a captured launch stays valid when the ids change.  Which rows have an adapter is decided by the
// id and rank rules of lora_common.h, shared with lora_bgmv.hip: the others are never written and nothing is loaded through their
// table slot.
//
// Rows are cut into tiles of 16.  A workgroup reads its tile's 16 ids and serves the distinct valid adapters among them one after
// the other: the first unserved lane's id, the rows that share it by ballot, one pass, until no row is left.  In every pass ALL 16
// rows go through the MFMA (rows of other adapters produce values nobody stores; rows past `rows` load from the last row's
// address); only the rows of the pass's adapter are stored, so a row is written exactly once per launch.  Cost: one pass per
// distinct adapter of a tile -- per-sequence ids at prefill give one pass per tile and two at a seam; the worst case, 16 rows with
// 16 different adapters, is 16 passes.
//
// x [rows][in], A_a [rank][in], B_a [out][rank] and t [rows][rank] are all row-major along the summed index, and a lane's operand
// fragment of the 16x16x32 MFMA is 8 consecutive k of one row: one 16-byte global load, no LDS staging, no transposition.
//   * shrink: A operand = x rows (M = the tile's rows), B operand = A_a rows (N = 16 ranks).  K is cut into sgmv_splits(in_features)
//     slices over workgroups and each slice into fixed contiguous shares of its 4 waves; the wave sums meet in LDS and are added in
//     wave order, the slice sums go to the fp32 workspace [rows][splits][max_rank] and are added in slice order by the expand.  The
//     cut is a function of in_features alone, never of rows: a row's bits do not depend on how many rows travel with it.
//   * expand + add: A operand = B_a rows (M = 16 outputs i), B operand = hi / lo of t (N = the tile's rows), formed in registers;
//     two MFMAs per k-step, and that K is only the rank.  The C/D layout (col = lane & 15, row = (lane >> 4) * 4 + reg) then gives
//     a lane 4 consecutive i of one row b: one 8-byte read-modify-write of y; a partial last group goes element by element.
// K tails are masked at the use (both operands zeroed), loads are unconditional from clamped addresses.  No atomics; every sum has
// a fixed order that depends on the shapes only, and the rows and columns of an MFMA do not mix: a row's bits depend on its own x
// row, its own y row and its adapter.  fp16 only: |t| above 65504 has no hi / lo pair (hi is infinite) and turns the row into NaN.
// The two bodies are lora_sgmv_body.h's, which lora_sgmv_routed.hip runs too on tiles gathered through the expert bucket.
#include "lora_sgmv_body.h"

namespace aqlm {

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_shrink_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                           const uint16_t* x, float* t, long xs, int ids_int64,
                                                                           int nadapters, int max_rank, int rows, int K8, int splits,
                                                                           int steps_per_wave) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b0 = blockIdx.z * 16;
  const int myid = lora_tile_id(ids, ids_int64, b0, rows, nadapters, lane);
  // rows past `rows` load from the last row's address; the t row of such a row is never written
  const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (long)std::min(b0 + (lane & 15), rows - 1) * xs);
  float* trow = t + (long)std::min(b0 + (lane >> 4) * 4 + wave, rows - 1) * splits * max_rank;
  lora_sgmv_shrink_body<T>(table, 1, myid, xrow, trow, blockIdx.x, blockIdx.y * 16, max_rank, K8, steps_per_wave);
}

template <class T>
__global__ __launch_bounds__(kSgmvWaves * 64) void lora_sgmv_expand_kernel(const aqlm_hip_lora_entry* table, const void* ids,
                                                                           const float* t, uint16_t* y, long ys, int ids_int64,
                                                                           int nadapters, int max_rank, int rows, int M, int splits) {
  const int lane = threadIdx.x & 63;
  const int b0 = blockIdx.y * 16;
  const int myid = lora_tile_id(ids, ids_int64, b0, rows, nadapters, lane);
  const int b = std::min(b0 + (lane & 15), rows - 1);  // (a row past `rows` has no id: its y row is never touched)
  lora_sgmv_expand_body<T>(table, 1, myid, t + (long)b * splits * max_rank, y + (long)b * ys, blockIdx.x * kSgmvSpan, max_rank, M,
                           splits);
}

template <class T>
static int launch_sgmv(const aqlm_hip_lora_entry* table, int nadapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const uint16_t* x, long xs, uint16_t* y, long ys, int M, int K, float* t, hipStream_t stream) {
  const int K8 = K / 8;
  const int splits = sgmv_splits(K);
  const int steps_per_wave = sgmv_steps_per_wave(K);
  const int row_tiles = (rows + 15) / 16;
  hipLaunchKernelGGL(lora_sgmv_shrink_kernel<T>, dim3(splits, (max_rank + 15) / 16, row_tiles), dim3(kSgmvWaves * 64), 0, stream,
                     table, ids, x, t, xs, ids_int64, nadapters, max_rank, rows, K8, splits, steps_per_wave);
  if (int e = check_hip(hipGetLastError(), "lora_sgmv_shrink launch")) return e;
  hipLaunchKernelGGL(lora_sgmv_expand_kernel<T>, dim3((M + 16 * kSgmvSpan - 1) / (16 * kSgmvSpan), row_tiles), dim3(kSgmvWaves * 64),
                     0, stream, table, ids, (const float*)t, y, ys, ids_int64, nadapters, max_rank, rows, M, splits);
  return check_hip(hipGetLastError(), "lora_sgmv_expand launch");
}

}  // namespace aqlm

using namespace aqlm;

extern "C" size_t aqlm_hip_lora_sgmv_workspace_bytes(int rows, int max_rank, int in_features) {
  if (!lora_shape_ok(1, in_features, max_rank, rows, AQLM_HIP_MAX_LORA_SGMV_ROWS)) return 0;
  return (size_t)rows * (size_t)sgmv_splits(in_features) * (size_t)max_rank * 4;
}

extern "C" int aqlm_hip_lora_sgmv_supported(int out_features, int in_features, int max_rank, int rows) {
  return lora_shape_ok(out_features, in_features, max_rank, rows, AQLM_HIP_MAX_LORA_SGMV_ROWS) ? 1 : 0;
}

extern "C" int aqlm_hip_lora_sgmv(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids, int ids_int64,
                                  int rows, const void* x, long x_row_stride, void* y, long y_row_stride, int out_features,
                                  int in_features, int dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  static const char* who = "aqlm_hip_lora_sgmv";
  if (int e = lora_check_args(who, table, num_adapters, max_rank, ids, ids_int64, rows, x, x_row_stride, y, y_row_stride, out_features,
                              in_features, dtype, workspace, AQLM_HIP_MAX_LORA_SGMV_ROWS))
    return e;
  if ((reinterpret_cast<uintptr_t>(y) & 7u) || (rows > 1 && y_row_stride % 4 != 0)) {
    set_last_error("%s: y rows not 8-byte aligned (y %p, stride %ld elements): the expand writes groups of 4 outputs", who, y,
                   y_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = lora_check_workspace(who, workspace_bytes, aqlm_hip_lora_sgmv_workspace_bytes(rows, max_rank, in_features))) return e;
  auto go = [&](auto t) {
    return launch_sgmv<decltype(t)>(table, num_adapters, max_rank, ids, ids_int64 ? 1 : 0, rows, (const uint16_t*)x, x_row_stride,
                                    (uint16_t*)y, y_row_stride, out_features, in_features, (float*)workspace, (hipStream_t)stream_);
  };
  return dtype == AQLM_HIP_F16 ? go(F16{}) : go(BF16{});
}

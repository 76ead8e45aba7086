// What the fused transposed MFMA GEMMs of the dense layers share (gemm_kx8_transposed.hip, gemm_1x16_transposed.hip):
//
//   gx[b, :] = sum_o gy[b, o] * Wq[o, :]          gy [rows][out], gx [rows][in], fp16 / bf16
//
// A block of 4 waves owns a tile of TP = 16 NPT batch rows x 128 columns of gx and walks the output rows in steps of 32, the k of one
// v_mfma_f32_16x16x32.  For every step it BUILDS the image W[32 rows][128 columns] in LDS and stages the step's gy tile beside it.
// How a step's W image is produced (and how far ahead) is each file's own; the layout of both images, the common arguments, the sum
// over slices and the host-side rules of a call are here, once.
//   * W image.  A thread owns two (row, 16-byte piece) cells: piece ch = tid & 15 of rows wr = tid >> 4 and wr + 16.  The product
//     sums over the image's ROWS, so the waves read it column-major with ds_read_b64_tr_b16 (two reads make the 8 k values of one
//     MFMA operand).  Rows are 256 bytes; piece ch of row r lies at 16-byte slot ch ^ ((r & 3) << 2), and rows with bit 3 set hold
//     the two 8-byte halves of every piece exchanged.  The addresses of one read: lane (kg = lane >> 4, li = lane & 15) of wave w
//     asks for row 8 kg + 4 h + (li >> 2), piece 4 w + (li & 3), logical half nn.  A 32-lane half is kg in {2 k, 2 k + 1}: rows
//     r0 .. r0 + 3 and r0 + 8 .. r0 + 11 with r0 a multiple of 4.  Within one kg the 16 lanes meet slots (4 w + p) ^ (q << 2),
//     q = li >> 2, p = li & 3 -- the XOR moves bits 2..3 of the slot, p its bits 0..1: 16 distinct 16-byte slots, which are the whole
//     256-byte bank row.  The two kg differ in row bit 3, so they read the SAME slots but opposite physical halves
//     (8 (nn ^ (kg & 1))): 32 distinct 8-byte slots, no bank shared.  An image write of 16 lanes (one wr, 16 ch) covers one whole row.
//   * gy image ([TP][32] per step): 64-byte rows, piece c (8 output rows) of batch row b at slot c ^ ((b >> 2) & 3) -- rows
//     b, b + 4, b + 8, b + 12 share a quarter of the banks and the XOR tells them apart for the 16 lanes (16 batch rows, one piece)
//     of a consumer's 16-byte read.
//     (Freedom from bank conflicts is argued from these addresses, for both images: no counter run has measured it.)
//   * Rows of gy past `rows`, output rows past `out` in the last step and columns past `in` enter as ZEROS: the transposed reads
//     need EXEC all ones, so the data is masked, never the lanes, and every wave runs the same control flow.
//   * The operands are swapped (A = W^T, B = gy^T) and the columns of a wave's two MFMA blocks are interleaved in fours, so a lane
//     ends with 8 consecutive columns of one batch row: fp32 accumulators, one rounding, one 16-byte store.
//
// Splitting the output rows.  With few batch rows the grid (row tiles x column blocks) cannot fill the device: the steps are dealt
// to `splits` blocks per tile, whose fp32 tiles go to a workspace [splits][rows][in] and are added in slice order by a second kernel
// before the one rounding -- deterministic, no atomics; a slice without steps writes zeros.  splits == 1 writes gx directly.
//
// Numerics: exact products of storage-type operands, fp32 accumulation over o ascending (per slice).  An MFMA output column
// depends on its own gy row only: a row's bits depend neither on the other rows of the call nor on their number, for given splits.
//
// What is NOT here.  A thread's shares of the two images, the consumer (the two transposed reads and the MFMAs of a step), the
// zeroing of the accumulators and the epilogue read the same in both kernels and stay written out in each.  Behind shared inlined
// functions -- each of them tried alone, a helper for the two reads included -- hipcc schedules the kernels differently (the
// 1x16 kernel of the 256-row tile lost 2 % at 4096 rows, the 64-row one moved its accumulators between AGPRs and VGPRs in every
// step), while with the parts below the instruction streams are those of the kernels before.  Keep the two copies in step by hand.
// moe_grouped_bwd.hip is a deliberate SECOND layout and is not built on this header at all: its W image XORs a piece by
// ((row & 3) << 2) | ((row >> 2) & 3) with no half exchange, its gy image by b >> 1, its columns are not interleaved (a lane ends
// with 4 columns of each block, written as fp32) and it has no slices.  Moving it here would change what its kernel computes
// where, not where its code lives.
#pragma once
#include <algorithm>

#include "gemm_rows16.h"

namespace aqlm {

constexpr int kTCols = 128;     // columns of gx per block
constexpr int kTRows = 32;      // output rows of W per step (the k of one MFMA)
constexpr int kTThreads = 256;  // 4 waves, 32 columns each
constexpr uint32_t kTWBytes = kTRows * kTCols * 2;
constexpr int kTMaxSplits = 16;
constexpr int kTFullGrid = 256;  // blocks from which the device counts as filled (one per CU)

// what every transposed kernel is told about gy, gx and the walk over the output rows (the 1x16 kernel's arguments end in it; the
// K x 8 kernel's spell it out around their K, which keeps its place)
struct TArgs {
  const uint16_t* gy;        // [rows][gys]
  uint16_t* gx;              // [rows][gxs]
  float* partial;            // [splits][rows][N], splits > 1
  long gys, gxs;
  int rows, M, N, in_groups, nsteps, steps_per_slice, splits;
};

// what ds_read_b64_tr_b16 takes and gives
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* glds_s16x4_ptr;

// byte offset of 16-byte piece ch (8 columns) of row `row` in the W image
__device__ __forceinline__ uint32_t timg(int row, int ch) { return 256u * row + 16u * (ch ^ ((row & 3) << 2)); }
// ... and of piece c (8 rows of W) of batch row b in the gy image
__device__ __forceinline__ uint32_t tgy(int b, int c) { return 64u * b + 16u * (c ^ ((b >> 2) & 3)); }

template <class T>
__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)T::from_float(a) | ((uint32_t)T::from_float(b) << 16); }

// the slices meet: fp32 sums in slice order, one rounding; a thread owns 8 columns of a row
template <class T>
static __global__ __launch_bounds__(256) void gemm_transposed_finalize_kernel(const float* partial, uint16_t* gx, long gxs, int rows, int N, int splits) {
  const size_t n8 = (size_t)N / 8, total = (size_t)rows * n8, plane = (size_t)rows * N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / n8, c = (i - b * n8) * 8;
    const float* src = partial + b * N + c;
    f32x4 x = *reinterpret_cast<const f32x4*>(src), y = *reinterpret_cast<const f32x4*>(src + 4);
    for (int z = 1; z < splits; ++z) {
      x += *reinterpret_cast<const f32x4*>(src + z * plane);
      y += *reinterpret_cast<const f32x4*>(src + z * plane + 4);
    }
    *reinterpret_cast<u32x4*>(gx + b * gxs + c) = u32x4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
  }
}

// (`what` names the launch in a HIP error)
inline int launch_finalize(int dtype, const TArgs& a, hipStream_t stream, const char* what) {
  const size_t items = (size_t)a.rows * (a.N / 8);
  const unsigned blocks = (unsigned)std::min<size_t>((items + 255) / 256, 256u * 16u);
  if (dtype == AQLM_HIP_F16)
    hipLaunchKernelGGL(gemm_transposed_finalize_kernel<F16>, dim3(blocks), dim3(256), 0, stream, a.partial, a.gx, a.gxs, a.rows, a.N, a.splits);
  else
    hipLaunchKernelGGL(gemm_transposed_finalize_kernel<BF16>, dim3(blocks), dim3(256), 0, stream, a.partial, a.gx, a.gxs, a.rows, a.N, a.splits);
  return check_hip(hipGetLastError(), what);
}

// splits == 0: enough slices to give every CU a block, while the workspace stays within a quarter of the W it replaces
// (splits * rows * in * 4 <= out * in * 2 / 4) and every slice has steps
inline int choose_splits(int rows, int M, int N, int tile_rows) {
  const long blocks = (long)((rows + tile_rows - 1) / tile_rows) * ((N + kTCols - 1) / kTCols);
  const long nsteps = (M + kTRows - 1) / kTRows;
  const long s = std::min<long>({(kTFullGrid + blocks - 1) / blocks, nsteps, (long)M / (8L * rows), (long)kTMaxSplits});
  return s < 2 ? 1 : (int)s;
}

// the fp32 partial tiles of a call (which rows and splits a *_workspace_bytes entry accepts is that entry's own rule)
inline size_t transposed_workspace_bytes(int rows, int N, int splits) { return splits <= 1 ? 0 : (size_t)splits * rows * N * sizeof(float); }

inline int check_transposed_workspace(const char* who, int rows, int N, int splits, const void* workspace, size_t workspace_bytes) {
  const size_t need = transposed_workspace_bytes(rows, N, splits);
  if (need == 0 || (workspace && aligned16(workspace) && workspace_bytes >= need)) return 0;
  set_last_error("%s: %d slices need a 16-B aligned workspace of %zu bytes, got %zu", who, splits, need, workspace ? workspace_bytes : (size_t)0);
  return AQLM_HIP_E_INVALID;
}

// what a call asks of rows, splits, gy and gx whatever the scheme: 16-byte aligned rows that hold the matrix's width
inline bool transposed_call_ok(int rows, int M, int N, int splits, const void* gy, const void* gx, long gys, long gxs) {
  return rows <= 65536 && splits >= 0 && splits <= kTMaxSplits && aligned16(gy) && aligned16(gx) && gys % 8 == 0 && gxs % 8 == 0 && gys >= M && gxs >= N;
}

// (splits: chosen, >= 1)
inline TArgs transposed_args(const void* gy, void* gx, void* workspace, long gys, long gxs, int rows, int M, int N, int in_group_size, int splits) {
  TArgs a{};
  a.gy = (const uint16_t*)gy;
  a.gx = (uint16_t*)gx;
  a.partial = (float*)workspace;
  a.gys = gys;
  a.gxs = gxs;
  a.rows = rows;
  a.M = M;
  a.N = N;
  a.in_groups = N / in_group_size;
  a.nsteps = (M + kTRows - 1) / kTRows;
  a.splits = splits;
  a.steps_per_slice = (a.nsteps + splits - 1) / splits;
  return a;
}

}  // namespace aqlm

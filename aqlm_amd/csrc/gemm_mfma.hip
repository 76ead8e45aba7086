// Fused dequant-tile -> MFMA GEMM for the 1x16 scheme at large batch (prefill / bs=128) on gfx950.
//
// Replaces (behaviour, not code): code1x16_matmat_dequant = Code1x16Dequant (W[out,in] materialised in HBM,
// reference cuda_kernel.cu:98-142) + F::linear / cuBLAS (cuda_kernel.cpp:249-301) + scale/bias epilogue launches.
//
// Key observation: with v_mfma_f32_32x32x16_{f16,bf16} the A operand of lane l is 8 consecutive k of row l%32
// (k-half l/32) -- which is exactly one 16-byte AQLM codebook vector (g=8), or one half of one (g=16).  So a
// gathered codebook entry IS an MFMA fragment: W is never written anywhere, not even to LDS.  Per 16-deep k step
// a wave issues ONE 16-B gather per lane (32 rows x 2 k-halves) and reuses it for every 32-column batch tile.
//
//   C[row = W row][col = batch]  +=  A = W[32 rows][16 k]  x  B = X^T[16 k][32 batch]
//
// Block = 4 waves = 128 output rows (one 32-row tile per wave, waves independent) x one K slice x all batch
// columns (<= 128, as NBT tiles of 32).  X is staged in 64-deep chunks through a double-buffered, XOR-swizzled
// LDS image shared by the 4 waves.  K is split over `ksplit` blocks so that the grid fills 256 CUs; fp32
// partials go to a workspace [ksplit][out][Bpad] and a second small kernel sums them, applies
// scales/bias, transposes to Y[B][out] and rounds once.
//
// Roofline: MFMA-bound in principle (2*B*out*in flop), but for out=in=4096, B=128 the 2.1 M random 16-B gathers
// (~1 lane/clk/CU) take ~2x the MFMA time, so this kernel is L2-gather bound like the gemv.
#include <algorithm>
#include <type_traits>

#include "aqlm_common.h"
#include "gemm_rows16.h"

// The rest of this file is its six parts, kept in files of their own.  They are not headers: no include guards and no #include of
// their own (gemm_1x16_rows16.h reads the kernel body it shares with moe_grouped.hip), each is read once, and the order of the
// #include lines below, with the order of the kernels inside each part, is the order of the kernels in the code object.
namespace aqlm {
#include "gemm_1x16_staged.h"  // register-staged 1x16 kernel (the one described above), its finalize, plan_gemm, launch_gemm
#include "gemm_1x16_glds.h"    // K-split LDS-DMA pipeline of the 1x16 scheme, its finalize (shared with K x 8), plan_glds, both launches
#include "gemm_1x16_rows16.h"  // 16-row 1x16 kernel and launch_rows16
#include "gemm_kx8_rows16.h"   // streaming 16-row kernel of the K x 8 schemes, plan_kx8, launch_kx8
}  // namespace aqlm

using namespace aqlm;

#include "gemm_kx8_xres.h"      // X-resident K x 8 kernels (whole image, phased), xres_fits, device_cus, their launches
#include "gemm_mfma_entries.h"  // aqlm_hip_workspace_bytes, gemm_kx8_xres_multi, the C entries of the K x 8 and 1x16 ops

// Part of gemm_mfma.hip (read there, inside namespace aqlm): the 16-row 1x16 kernel -- types, LDS map and plan in gemm_rows16.h, body in
// gemm_rows16_body.h, both shared with moe_grouped.hip -- and its launch.
// ---------------------------------------------------------------------------------------------------------------------------
// 16-row blocks, no K split (round 4).  The pipeline above minimises what goes through a CU's L1 (X is read once per K slice)
// and pays for it with two launches, 16.8 MB of fp32 partials and a finalize: 8.3 + 3.9 us of a 23 us op at 128 rows, and the
// same 8.3 us at 16 rows.  Here a block owns 16 output rows over ALL of K: no partials, no workspace, no second kernel -- and
// every block streams all of X (B x K x 2 bytes) through its L1 next to its 8192 gathers.  That trade wins when X is small
// next to the gathers' 128-B lines (16 x 8 KiB rows of X = 128 KiB against 1 MiB of lines) and is about even at 128 rows.
//   wave 0            codes -> LDS -> 2 gathers per 64-k chunk (one 1-KiB MFMA A fragment per 32 k), NSW - 1 steps ahead: the
//                     gathers are latency-bound (a few hundred must be in flight), the fragments are small (2 KiB per chunk)
//   waves 1..NXP      the X chunks (B rows x 128 B each, XOR-swizzled slots as above) by LDS-DMA, NSX - 1 steps ahead
//   R16_NC consumers  wave c multiplies the block's ONE A fragment with its batch tiles; fp32 accumulators over all of K,
//                     scale + bias + one rounding in the epilogue (16 x 16 tile: 4 rows x 1 batch column per lane)
// One s_barrier per STEP of CPB chunks joins the three roles (counted vmcnt on the DMA waves, as above).  A step lasts only
// 0.15-0.35 us per chunk, and between "my DMA of this step is accepted" and "everybody has passed the barrier" the texture
// addresser has nothing queued: with one chunk per step that gap was a quarter of the time (measured: 0.30 gathers / clk / CU
// against the 0.43 of the flat-out microbenchmark), so small batches take 4 chunks per step.
// where the op takes this kernel (measured, profiles/r04_gemm_rows16_shapes.json): every block streams all of X, so the trade
// turns with batch x layer size -- up to 16 rows everywhere, up to 64 rows for layers of <= 4096 x 4096
constexpr int R16_ROWS_ANY = 16, R16_ROWS_SMALL = 64;
constexpr long R16_SMALL_LAYER = 1L << 24;

template <class T, int G, int NBT, int CPB>
__global__ __launch_bounds__((R16Lds<NBT, CPB>::WAVES * 64)) void gemm_1x16_rows16_kernel(const R16Params p)
#define R16_ROW0 ((int)blockIdx.x * 16)
#define R16_X_ROW(b) ((b) < p.B ? (b) : p.B - 1)
#define R16_Y_ROW(b) (b)
#include "gemm_rows16_body.h"


template <class T, int G>
static int launch_rows16(const R16Params& p, const R16Plan& r, hipStream_t stream) {
  const dim3 grid((unsigned)((p.M + 15) / 16));
  auto go = [&](auto kern, size_t lds, int waves) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(waves * 64), lds, stream, p);
    return check_hip(hipGetLastError(), "gemm_1x16_rows16 launch");
  };
#define AQLM_R16_CASE(NBT_, CPB_) return go(gemm_1x16_rows16_kernel<T, G, NBT_, CPB_>, R16Lds<NBT_, CPB_>::TOTAL, R16Lds<NBT_, CPB_>::WAVES)
  if (r.cpb == 1) {
    switch (r.nbt) {
      case 1: AQLM_R16_CASE(1, 1);
      case 2: AQLM_R16_CASE(2, 1);
      case 4: AQLM_R16_CASE(4, 1);
      default: AQLM_R16_CASE(8, 1);
    }
  }
  switch (r.nbt) {
    case 1: AQLM_R16_CASE(1, 4);
    case 2: AQLM_R16_CASE(2, 4);
    case 4: AQLM_R16_CASE(4, 2);
    default: AQLM_R16_CASE(8, 2);
  }
#undef AQLM_R16_CASE
}

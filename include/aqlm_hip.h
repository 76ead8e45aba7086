/*
 * aqlm_hip.h -- C ABI of libaqlm_hip.so: the MI355X (gfx950 / CDNA4) implementation of the AQLM
 * additive-codebook dequant-fused matvec / matmul path.
 *
 * This is the drop-in boundary for the ONE hot path of Vahe1994/AQLM that this repository replaces
 * (SURVEY.md section 8).  Each entry point names the reference interface it replaces; paths are relative
 * to the reference tree (inference_lib/src/aqlm/inference_kernels/).  INTEGRATION.md shows the binding
 * a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - raw device pointers, caller-owned, never retained; inputs are never written (one documented exception: the
 *     accumulator cells inside a prepacked buffer, see aqlm_hip_gemv_1x16_packed; the *_cells entries avoid it);
 *   - stream-ordered on `stream` (a hipStream_t passed as void*; NULL = the null stream), asynchronous,
 *     no allocation, no synchronisation -> hipGraph-capturable and re-entrant (the packed 1x16 matvec entries order
 *     themselves by data flow inside a capture: "Capture overlap" below);
 *   - tensors use the reference's checkpoint layout unchanged:
 *       codes      [out_features][in_features/in_group_size][num_codebooks]  int8 (nbits<=8) / int16 (nbits<=16)
 *                  two's-complement containers holding UNSIGNED indices (utils.py:11-31)
 *       codebooks  [num_codebooks][2**nbits][1][in_group_size]               fp16 / bf16
 *       scales     [out_features]   (the reference's [out,1,1,1], contiguous)  fp16 / bf16
 *       bias       [out_features] or NULL
 *     out_group_size is 1 (as in every reference kernel, kernel_selector.py:27-94);
 *   - every kernel fuses the epilogue  y = acc * scales[row] + bias[row]  (replaces
 *     scale_bias_unflatten_output, cuda_kernel.cpp:95-111); accumulation is fp32;
 *   - dtype: AQLM_HIP_F16 or AQLM_HIP_BF16 for x / y / codebooks / scales / bias alike
 *     (check_use_bfloat16, cuda_kernel.cpp:9-25);
 *   - output of the dense forward entries (aqlm_hip_gemv_1x16 / _kx8 / _generic and their _multi forms, the aqlm_hip_gemv_1x16_packed*
 *     and aqlm_hip_gemv_8x8_lut* matvecs, aqlm_hip_gemm_1x16_mfma, aqlm_hip_gemm_1x16_scan, aqlm_hip_gemm_kx8_mfma[_ws],
 *     aqlm_hip_gemm_8x8_mfma): x / y row strides in elements; y 2-byte aligned with y_row_stride >= out_features (columns past
 *     out_features are not touched): exactly the batch x out_features windows [b * y_row_stride, b * y_row_stride + out_features) are
 *     written, whatever y's alignment and the stride's residue -- no other alignment of y is required and the layout of y selects no
 *     kernel, so a row's bits do not depend on it.  The segments of a _multi entry carry their own y and y_row_stride and may lie
 *     side by side in one buffer (q / k / v).  A workspace is used only up to the advertised size (aqlm_hip_workspace_bytes,
 *     aqlm_hip_gemm_1x16_scan_workspace_bytes) and accumulator cells only up to batch x out_features x 8 bytes; nothing behind them is
 *     written (tests/test_y_layout_gpu.py);
 *   - input of the same dense forward entries: exactly the batch windows [b * x_row_stride, b * x_row_stride + in_features) of x are
 *     read and nothing else of it.  Any x_row_stride >= in_features is legal, and so are 0 (every row is row 0) and
 *     0 < x_row_stride < in_features (overlapping rows), as long as the alignment rule below holds.  A negative x_row_stride at
 *     batch > 1 is AQLM_HIP_E_INVALID on every entry, refused by one shared check before anything is launched.  At batch == 1
 *     x_row_stride is not read and selects no kernel: any value gives the result of x_row_stride == in_features.
 *     Alignment: aqlm_hip_gemv_1x16 / _kx8 / _generic and aqlm_hip_gemv_1x16_multi / _kx8_multi accept any 2-byte aligned x and any
 *     stride; an x that is not 16-byte aligned, or at batch > 1 a stride that is no multiple of 8, takes the generic kernel (the
 *     bits of the same call under the tuning key force_generic).  Every other entry needs a 16-byte aligned x and, at batch > 1,
 *     x_row_stride % 8 == 0; otherwise it writes nothing to y, names x in the message and returns AQLM_HIP_E_UNSUPPORTED
 *     (aqlm_hip_gemm_1x16_mfma, aqlm_hip_gemm_1x16_scan, aqlm_hip_gemm_kx8_mfma[_ws], aqlm_hip_gemm_8x8_mfma, and the
 *     aqlm_hip_gemv_8x8_lut* matvecs for the pointer) or AQLM_HIP_E_INVALID (the aqlm_hip_gemv_1x16_packed* matvecs; the stride of
 *     aqlm_hip_gemv_8x8_lut_batch, which must also be below 2^31).
 *     Routing: a row's value does not depend on x_row_stride; its bits may, because the route does.  The K x 8 entries
 *     (aqlm_hip_gemm_kx8_mfma[_ws], and through them aqlm_hip_gemv_kx8 from kx8_mfma_min_rows rows and aqlm_hip_gemv_kx8_multi) take the X-resident
 *     kernel only for 0 < x_row_stride < 2^22 and the phased kernel only for 0 < x_row_stride < 2^21; at 0 and from those limits on
 *     the streaming kernel runs (the bits of the same call under kx8_xres 0).  Every other entry gives the same bits at every legal
 *     stride, up to rows that lie more than 4 GiB behind x (tests/test_x_layout_gpu.py);
 *   - return 0 on success; a positive value is a hipError_t from the launch; negative values are
 *     AQLM_HIP_E_*.  aqlm_hip_last_error() returns a thread-local human-readable message.
 */
#ifndef AQLM_HIP_H_
#define AQLM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQLM_HIP_ABI_VERSION 9

#define AQLM_HIP_F16 0
#define AQLM_HIP_BF16 1
#define AQLM_HIP_F32 2 /* dW and the outputs of the gradient entries (aqlm_hip_codebook_grad_1x16, aqlm_hip_scales_grad_1x16) and the
                          reference of aqlm_hip_code_search_1x16 only */

#define AQLM_HIP_E_INVALID (-1)     /* bad argument (null pointer, non-positive size, misaligned buffer) */
#define AQLM_HIP_E_UNSUPPORTED (-2) /* shape / scheme outside what the entry point implements */

#define AQLM_HIP_MAX_GEMV_BATCH 8

/* ABI version of the loaded library (== AQLM_HIP_ABI_VERSION of the header it was built from). */
int aqlm_hip_abi_version(void);

/* Thread-local message describing the last non-zero return on this thread ("" if none). */
const char* aqlm_hip_last_error(void);

/*
 * y[b, :] = (W x[b, :]) * scales + bias   for b < batch (1..AQLM_HIP_MAX_GEMV_BATCH), 1x16 scheme
 * (one codebook of 65536 entries, in_group_size 8 or 16).  ONE launch for all batch rows: codes and the
 * gathered codebook vectors are reused across the rows of x.
 *
 * Replaces: code1x16_matvec_cuda<bf16,g> + launcher (cuda_kernel.cu:7-95, 476-521), the per-row host loop of
 *           code1x16_matmat (cuda_kernel.cpp:148-182) and its 3-4 epilogue launches (cuda_kernel.cpp:95-111).
 * x_row_stride / y_row_stride are in elements.  Requirements: in_features % in_group_size == 0.
 */
int aqlm_hip_gemv_1x16(const void* codes_i16, const void* codebook, const void* scales, const void* bias,
                       const void* x, void* y, int out_features, int in_features, int in_group_size, int batch,
                       long x_row_stride, long y_row_stride, int dtype, void* stream);

/*
 * One launch for up to AQLM_HIP_MAX_SEGMENTS 1x16 layers that multiply the SAME x (q/k/v or gate/up of a decoder
 * layer): y_s[b, :] = (W_s x[b, :]) * scales_s + bias_s for every segment s.  Each segment has its own codes,
 * codebook, scales, bias and output; all share in_features, in_group_size, batch, dtype.  Results are bit-identical to
 * num_segments calls of aqlm_hip_gemv_1x16.
 *
 * Replaces: the three (two) consecutive code1x16_matmat calls a decoder layer issues on one hidden state
 *           (cuda_kernel.cpp:148-182 called from inference.py:68-76 once per projection); SURVEY.md section 8(f)2.
 */
typedef struct aqlm_hip_segment {
  const void* codes;     /* [out_features][in_features/in_group_size] int16 (aqlm_hip_gemv_1x16_multi), or the
                            prepacked buffer of aqlm_hip_prepack_1x16 (aqlm_hip_gemv_1x16_packed_multi) */
  const void* codebook;  /* [65536][in_group_size] */
  const void* scales;    /* [out_features] */
  const void* bias;      /* [out_features] or NULL */
  void* y;               /* [batch][out_features], row stride y_row_stride elements */
  long y_row_stride;
  int out_features;
  int reserved;          /* set to 0 */
} aqlm_hip_segment;

#define AQLM_HIP_MAX_SEGMENTS 4

int aqlm_hip_gemv_1x16_multi(const aqlm_hip_segment* segments, int num_segments, const void* x, int in_features,
                             int in_group_size, int batch, long x_row_stride, int dtype, void* stream);

/*
 * Expert-routed 1x16 matvec of a mixture-of-experts block (Mixtral decode).  `table` is a DEVICE array of
 * num_experts * num_segments entries, entry [e * num_segments + s] = projection s of expert e (w1, w3 for the
 * gate/up launch: num_segments 2; w2: num_segments 1).  All entries share out_features, in_features, in_group_size
 * (8 or 16) and dtype; codes and codebook 16-byte aligned.  expert_ids: DEVICE [num_pairs] (= [T, top_k] row-major)
 * int64 (ids_int64 != 0, what torch.topk returns) or int32.  For every pair p < num_pairs and segment s:
 *     y[(p * num_segments + s) * out_features + o] = (W[e_p, s] x_row(p))[o] * scales[o] + bias[o]
 * with x_row(p) = x + (x_per_pair ? p : p / top_k) * x_row_stride: fp32 sums, one rounding -- bit-identical to
 * aqlm_hip_gemv_1x16 of that expert on that row.  Ids are only ever compared for equality with an expert index: a
 * pair whose id lies outside [0, num_experts) gets a zero row, whatever the ids hold (duplicates, one expert for
 * every pair, garbage).  The grid (row blocks x segments x experts) depends on the shapes only, so a captured launch
 * stays valid when the routing changes; a workgroup whose expert has no pair exits at once.  num_pairs <=
 * AQLM_HIP_MAX_ROUTED_PAIRS; more than AQLM_HIP_MAX_GEMV_BATCH pairs on one expert are taken in passes.
 * AQLM_HIP_E_UNSUPPORTED for shapes outside the direct kernel (in_features / in_group_size % 8 != 0, x row > 64 KiB,
 * unaligned x): the caller runs those per expert.
 */
typedef struct aqlm_hip_routed_entry {
  const void* codes;     /* [out_features][in_features/in_group_size] int16 */
  const void* codebook;  /* [65536][in_group_size] */
  const void* scales;    /* [out_features] */
  const void* bias;      /* [out_features] or NULL */
} aqlm_hip_routed_entry;

#define AQLM_HIP_MAX_ROUTED_PAIRS 64
#define AQLM_HIP_MAX_ROUTED_EXPERTS 256

int aqlm_hip_gemv_1x16_routed(const aqlm_hip_routed_entry* table, int num_experts, int num_segments,
                              const void* expert_ids, int ids_int64, int num_pairs, int top_k, const void* x,
                              long x_row_stride, int x_per_pair, void* y, int out_features, int in_features,
                              int in_group_size, int dtype, void* stream);

/*
 * Expert-grouped 1x16 GEMM of a mixture-of-experts block (Mixtral prefill, batched decode, training): the same
 * projection as aqlm_hip_gemv_1x16_routed for any number of pairs, in two launches whose grids depend on the shapes only.
 *
 * aqlm_hip_moe_bucket groups the pairs by expert on the device, in ONE workgroup: expert_ids DEVICE [num_pairs]
 * (= [T, top_k] row-major) int64 (ids_int64 != 0) or int32, as for the routed entry.  `bucket` is a 16-byte aligned DEVICE
 * buffer of aqlm_hip_moe_bucket_bytes(num_pairs, num_experts, tile_pairs) bytes (a size that depends on these three only)
 * that receives each expert's pairs in ascending pair order and a table of tiles (expert, first pair, <= tile_pairs
 * pairs).  Ids outside [0, num_experts) join no expert: they are only compared, never used to form an address.
 * aqlm_hip_moe_bucket_bytes returns 0 for arguments the entries refuse.
 *
 * aqlm_hip_gemm_1x16_grouped reads a bucket made with the same num_pairs, num_experts and tile_pairs and the routed
 * entries' table, and writes, like aqlm_hip_gemv_1x16_routed, for every pair p < num_pairs and segment s:
 *     y[(p * num_segments + s) * out_features + o] = (W[e_p, s] x_row(p))[o] * scales[o] + bias[o]
 * with x_row(p) = x + (x_per_pair ? p : p / top_k) * x_row_stride; fp32 sums, one rounding; pairs with an id outside
 * [0, num_experts) get zero rows.  A block owns 16 output rows of one tile over all of K (the 16-row kernel of
 * aqlm_hip_gemm_1x16_mfma): each expert's rows are bit-identical to aqlm_hip_gemm_1x16_mfma on that expert's rows where
 * that op runs its 16-row kernel (tuning key gemm_variant = 2), and a pair's bits depend neither on the other pairs nor on
 * their number.  Grid: out_features / 16 x (ceil(num_pairs / tile_pairs) + min(num_experts, num_pairs)) tile slots x
 * num_segments; a captured launch stays valid when the routing changes.  tile_pairs is 16, 32, 64 or 128 (the caller
 * picks it from num_pairs and num_experts, never from the routing).  AQLM_HIP_E_UNSUPPORTED outside the 16-row kernel:
 * aqlm_hip_gemm_1x16_grouped_supported(out_features, in_features, in_group_size) says beforehand (out_features % 16,
 * in_features % 64, in_group_size 8 / 16, K long enough for the kernel's rings).
 */
#define AQLM_HIP_MAX_GROUPED_PAIRS (1 << 18)

size_t aqlm_hip_moe_bucket_bytes(int num_pairs, int num_experts, int tile_pairs);
int aqlm_hip_moe_bucket(const void* expert_ids, int ids_int64, int num_pairs, int num_experts, int tile_pairs, void* bucket,
                        void* stream);
int aqlm_hip_gemm_1x16_grouped_supported(int out_features, int in_features, int in_group_size);
int aqlm_hip_gemm_1x16_grouped(const aqlm_hip_routed_entry* table, int num_experts, int num_segments, const void* bucket,
                               int tile_pairs, int num_pairs, int top_k, const void* x, long x_row_stride, int x_per_pair,
                               void* y, int out_features, int in_features, int in_group_size, int dtype, void* stream);

/*
 * Input gradient of aqlm_hip_gemm_1x16_grouped: the transposed product, on the bucket and the table of the forward launch.
 * For every pair p < num_pairs, in fp32:
 *     gx[p * in_features + i] = sum_s sum_o (gy[p * gy_pair_stride + s * out_features + o] * scales[e_p, s][o]) * Wq[e_p, s][o][i]
 * Wq is the unscaled dequantised matrix of expert e_p (the expert the bucket lists pair p under), segment s; the bias does
 * not enter.  Pairs with an id outside [0, num_experts) get zero rows.  gy * scales is formed in fp32 and rounded once to
 * the storage type (the one rounding this route adds); the products are exact, the sums fp32 in a fixed order (segment, then
 * output row ascending), so a pair's bits depend on its own gy row and its expert only -- not on the other pairs, the
 * tile size or the slot.  W is never written to memory: a block owns one tile's pairs x 128 columns over all output rows
 * and segments, gathers the codebook vectors of 32 rows at a time into LDS and reads them column-major
 * (ds_read_b64_tr_b16) as an operand of v_mfma_f32_16x16x32.  Grid: ceil(in_features / 128) x the forward's tile slots; no
 * allocation, no synchronisation, no workspace: a captured launch stays valid when the routing changes.  gy and gx 16-byte
 * aligned, gy_pair_stride (in elements) a multiple of 8 and >= num_segments * out_features.  AQLM_HIP_E_UNSUPPORTED outside
 * aqlm_hip_gemm_1x16_grouped_transposed_supported (out_features % 16 == 0, in_features % 16 == 0, in_group_size 8 / 16): the
 * caller runs those per expert on the dequantise + matmul ops.
 *
 * Replaces: the dequantise + matmul of cuda_kernel.cpp's *_transposed functions (code1x16_matmat_dequant_transposed,
 *           cuda_kernel.cpp:303 ff.: input * scales rounded to the storage type, Code1x16Dequant into a whole weight matrix
 *           in memory, then a library matmul), which a mixture-of-experts backward would run once per expert and projection.
 */
int aqlm_hip_gemm_1x16_grouped_transposed_supported(int out_features, int in_features, int in_group_size);
int aqlm_hip_gemm_1x16_grouped_transposed(const aqlm_hip_routed_entry* table, int num_experts, int num_segments,
                                          const void* bucket, int tile_pairs, int num_pairs, const void* gy, long gy_pair_stride,
                                          void* gx, int out_features, int in_features, int in_group_size, int dtype,
                                          void* stream);

/*
 * Same contract for K x 8-bit schemes (256-entry codebooks held in LDS): num_codebooks in 1..16, any
 * in_group_size that is a multiple of 8 (tuned instances: 1x8 g8, 2x8 g8, 8x8 g32; other shapes run a generic kernel).
 *
 * Replaces: Code2x8MatVec / CodeKx8MatVec + launchers (cuda_kernel.cu:144-233, 296-390, 555-620, 709-758),
 *           code2x8_matmat / code1x8_matmat (cuda_kernel.cpp:387-421, 552-586), and the Triton generic gemv the
 *           reference falls back to for 8x8 etc. (triton_kernel.py:30-205).
 */
int aqlm_hip_gemv_kx8(const void* codes_i8, const void* codebooks, const void* scales, const void* bias,
                      const void* x, void* y, int out_features, int in_features, int num_codebooks,
                      int in_group_size, int batch, long x_row_stride, long y_row_stride, int dtype, void* stream);

/*
 * aqlm_hip_gemv_kx8 for up to AQLM_HIP_MAX_SEGMENTS layers of one K x 8-bit scheme that multiply the same x, in one
 * launch (tuned: 1x8 / 2x8 g8; other schemes run one launch per segment).  segment.codes is int8
 * [out_features][in_features/in_group_size][num_codebooks], segment.codebook is [num_codebooks][256][in_group_size].
 * Results agree with separate aqlm_hip_gemv_kx8 calls to fp32 rounding (a segment may run on a different kernel of
 * the family than it would alone: replicated-LDS vs plain LDS).  2 .. 16 rows of 1x8 / 2x8 g8 (ABI 8): ONE launch of the X-resident
 * fused MFMA kernel over all layers when their codebooks and the X image fit one LDS together (X loaded once, tile walk over the
 * layers back to back) -- bit-identical to the layers' own calls; else one launch per layer.
 * Replaces: consecutive code2x8_matmat / code1x8_matmat calls on one hidden state (cuda_kernel.cpp:387-421, 552-586).
 */
int aqlm_hip_gemv_kx8_multi(const aqlm_hip_segment* segments, int num_segments, const void* x, int in_features,
                            int num_codebooks, int in_group_size, int batch, long x_row_stride, int dtype,
                            void* stream);

/*
 * Fully generic gemv (any num_codebooks, nbits <= 16, any in_group_size, codes in 8- or 16-bit containers):
 * the slow-but-correct path for every scheme without a tuned kernel (the role of triton_kernel.py in the
 * reference, kernel_selector.py:91-94).
 */
int aqlm_hip_gemv_generic(const void* codes, const void* codebooks, const void* scales, const void* bias,
                          const void* x, void* y, int out_features, int in_features, int num_codebooks, int nbits,
                          int in_group_size, int batch, long x_row_stride, long y_row_stride, int dtype,
                          void* stream);

/*
 * W[out_features][in_features] = sum_c codebooks[c][codes[.., c]]  (* scales[row] if scales != NULL), row-major.
 * Replaces: Code1x16Dequant / code1x16_dequant_cuda (cuda_kernel.cu:98-142, 523-553), and with scales the
 *           pybind `code1x16_dequant` (cuda_kernel.cpp:184-227).
 */
int aqlm_hip_dequant_1x16(const void* codes_i16, const void* codebook, const void* scales /* nullable */, void* W,
                          int out_features, int in_features, int in_group_size, int dtype, void* stream);

/*
 * Replaces: Code2x8Dequant / CodeKx8Dequant (cuda_kernel.cu:235-294, 392-468, 622-707, 760-817) and the pybind
 *           `code2x8_dequant` / `code1x8_dequant` (cuda_kernel.cpp:423-448, 588-613).  Unlike the reference's
 *           CodeKx8Dequant there is no read-modify-write of W: all codebooks are summed in registers.
 */
int aqlm_hip_dequant_kx8(const void* codes_i8, const void* codebooks, const void* scales /* nullable */, void* W,
                         int out_features, int in_features, int num_codebooks, int in_group_size, int dtype,
                         void* stream);

/*
 * The same for ANY scheme (num_codebooks, nbits <= 16 in 8- / 16-bit containers, any in_group_size): the role of the
 * reference's torch fallback `_dequantize_weight` (utils.py:43-70) for schemes without a tuned kernel -- used by the
 * large-batch and backward ops of such schemes.
 */
int aqlm_hip_dequant_generic(const void* codes, const void* codebooks, const void* scales /* nullable */, void* W,
                             int out_features, int in_features, int num_codebooks, int nbits, int in_group_size,
                             int dtype, void* stream);

/*
 * Large-batch path: Y[B][out] = (X[B][in] @ W^T) * scales + bias with W dequantised tile-by-tile into LDS and
 * contracted on the matrix cores (v_mfma_f32_16x16x32_f16/bf16: a gathered codebook vector IS a fragment lane); W never
 * touches HBM.  Two kernels behind the entry, chosen by batch and layer size (tuning key `gemm_variant` forces one): a K-split
 * pipeline with fp32 partials in `workspace` + a finalize launch, and (<= 16 rows; <= 64 rows on layers of <= 4096 x 4096) a
 * single launch of 16-row blocks over all of K that uses no workspace.  (`gemm_variant` = 4 / `scan_max_rows` > 0: the slice-scan
 * kernel of aqlm_hip_gemm_1x16_scan instead, where it applies.)
 * Replaces: code1x16_matmat_dequant = Code1x16Dequant + F::linear(cuBLAS) + epilogue (cuda_kernel.cpp:249-301).
 * X and Y are row-major with the given row strides (elements).  workspace: aqlm_hip_workspace_bytes(...) bytes
 * (may be 0 -> NULL allowed).
 */
int aqlm_hip_gemm_1x16_mfma(const void* codes_i16, const void* codebook, const void* scales, const void* bias,
                            const void* X, void* Y, int batch, int out_features, int in_features,
                            int in_group_size, long x_row_stride, long y_row_stride, int dtype, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * 1x16, in_group_size 8, at 2 .. any number of rows WITHOUT gathers from L2 (round 6; gemm_1x16_scan.hip): the codebook is cut into 8
 * slices of 8192 entries (128 KiB); a workgroup keeps one slice in LDS, scans the canonical codes [out][in / 8] of its row group and
 * feeds v_mfma_f32_16x16x32 with W fragments whose lanes read their entry when it lives in the workgroup's slice and a zero vector
 * when it does not; x stays in registers (every wave owns a K range), the eight slices' partial sums (x K chunks for long rows) go to
 * `workspace` as fp32 planes [8 * chunks][batch][out] and a second launch adds them in plane order, applies scales + bias and rounds
 * once.  Data-oblivious (no prepacked copy, no dependence on the code histogram), deterministic, batch-invariant; rows are processed
 * in passes of 16.  Needs in_features % 256 == 0, 16-B aligned codes / codebook / X rows / workspace.
 * NOT on a default route: measured slower than the L2-gather kernels of aqlm_hip_gemm_1x16_mfma at Llama layer sizes (8-fold
 * redundant scan + 11.5 us fixed: profiles/r06_scan_kernel_*.log); that entry takes it with tuning key `gemm_variant` = 4 or up to
 * `scan_max_rows` (default 0) rows.
 * Replaces: the per-row relaunch of the matvec for 2 .. 6 rows (cuda_kernel.cpp:165-175) and code1x16_matmat_dequant =
 * Code1x16Dequant + cuBLAS + epilogue above (cuda_kernel.cpp:249-301; cuda_kernel.cu:98-142).
 * workspace: aqlm_hip_gemm_1x16_scan_workspace_bytes(batch, out_features, in_features) bytes (0 = the shape has no plan).
 */
size_t aqlm_hip_gemm_1x16_scan_workspace_bytes(int batch, int out_features, int in_features);
int aqlm_hip_gemm_1x16_scan(const void* codes_i16, const void* codebook, const void* scales, const void* bias, const void* X, void* Y,
                            int batch, int out_features, int in_features, long x_row_stride, long y_row_stride, int dtype,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * Load-time repack of 1x16 codes (g 8 or 16) into the slice-bucketed format v7 consumed by aqlm_hip_gemv_1x16_packed (layout:
 * aqlm_amd/csrc/packed_format.h and the head of gemv_packed.hip, specification tests/packed_model.py, the repack itself
 * packed_repack_kernels.h and packed_repack_entries.h; 4 bytes per code + ~6 bytes
 * per (row, slice), plus 64 bytes per output row of zero-at-rest accumulator cells for the fused finalize).
 * The reference does the analogous thing for its CPU kernel: a one-off permutation of `codes` at first use
 * (inference.py:78-83).
 *
 * The packed kernels give every workgroup one slice of the codebook (`code >> 12`) and the codes that fall into it, so their
 * speed depends on how evenly the codes use the slices; the reference's kernels are data-oblivious (one warp per output row,
 * cuda_kernel.cu:16-27, launcher :496-507), and real checkpoints (k-means + beam search, src/aq.py:286-356) are not uniform.
 * Format v7 therefore balances at pack time, losslessly:
 *   * RELABELLING (AQLM_HIP_PACKED_RELABELLED): the repack counts how often every codebook entry is used and deals the entries
 *     to the slices so that the slices carry equal numbers of codes (longest-processing-time greedy, at most 65536 / slices
 *     entries per slice).  The permutation is kept inside the buffer (aqlm_hip_unpack_1x16 undoes it: bit-exact codes), and the
 *     kernels read a PERMUTED IMAGE of the codebook that also lives in the buffer: the caller writes it with
 *     aqlm_hip_packed_set_codebook (again whenever the codebook changes) -- the `codebook` argument of the matvec entries is then
 *     ignored.  Codes that already use the slices evenly (within 2 %) are not relabelled: no permutation, no image, and the
 *     buffer is what format v6 held.
 *   * VARIABLE GEOMETRY (AQLM_HIP_PACKED_VARGEOM; 16-byte vectors only): a single entry used by more than 1 / 16 of all codes
 *     cannot be balanced by any labelling.  The 256 workgroups are then dealt to the slices in proportion to their work
 *     (slice_groups[s] workgroups for slice s, each owning out_features / slice_groups[s] consecutive rows; >= 8 per slice), instead
 *     of 16 row groups for every slice.  Every row still receives exactly one contribution per slice, so the finalize is
 *     unchanged.  Such buffers run on the single-layer entries (the shared-input / chain / publish entries run them one layer per
 *     launch or refuse with AQLM_HIP_E_UNSUPPORTED); AQLM_HIP_PREPACK_UNIFORM_ONLY asks the repack not to use it.
 *   aqlm_hip_prepack_1x16_bytes  capacity the caller must provide (0: shape not covered -- in_group_size not 8 or 16, more
 *                                input groups than an entry's 12 / 11-bit slot field addresses, or rows whose tables fit no LDS
 *                                image); more than the result needs: the repack uses the tail as scratch.
 *                                in_group_size 16 = the second instantiation (32 slices of 2048 x 32 B).
 *   aqlm_hip_prepack_1x16[_ex]   fills `packed` and `*desc`; desc->used_bytes <= capacity is what has to be kept (the
 *                                buffer may be trimmed / copied; the descriptor travels with it and is also stored in the
 *                                buffer's first bytes).  Synchronises `stream` (load-time call, not graph-capturable).
 *                                AQLM_HIP_E_UNSUPPORTED when even the balanced streams do not fit the capacity (rows that differ
 *                                wildly from one another); `flags`: AQLM_HIP_PREPACK_* below (0 = everything allowed).
 *   aqlm_hip_packed_set_codebook writes the permuted codebook image of a relabelled buffer (no-op for others) and sets
 *                                AQLM_HIP_PACKED_HAS_CODEBOOK in `*desc`; stream-ordered, no synchronisation.
 *   aqlm_hip_packed_desc_read    descriptor from the first sizeof(desc) bytes of a packed buffer copied to the host.
 *   aqlm_hip_unpack_1x16         the inverse: canonical int16 codes [out][in/8] from a packed buffer (lossless).
 *   aqlm_hip_dequant_1x16_packed W[out_features][in_features] (row-major, fp16 / bf16: `dtype`) straight from a packed buffer, without
 *                                the int16 codes in between: W[r, j*g:(j+1)*g] = codebook[label(r, j)], times scales[r] in fp32 with
 *                                one rounding when `scales` is not NULL -- bit-identical to aqlm_hip_dequant_1x16 on the output of
 *                                aqlm_hip_unpack_1x16.  Covers what the unpack entry covers (g 8 / 16, 4- and 3-byte entries, uniform
 *                                and variable geometry, relabelled or not).  W depends on the entries, on the permutation stored in
 *                                the buffer and on the `codebook` passed in (the checkpoint's labelling, [65536][g]) only: the
 *                                permuted codebook image, AQLM_HIP_PACKED_HAS_CODEBOOK and desc->codebook_absmax are not looked at.
 *                                Every element of W is written exactly once, nothing else is written.  `packed`, `codebook` and W
 *                                must be 16-byte aligned.  Stream-ordered: no allocation, no synchronisation, no workspace
 *                                (hipGraph-capturable).  AQLM_HIP_E_INVALID: null / misaligned pointer or a descriptor that does
 *                                not describe a packed buffer; AQLM_HIP_E_UNSUPPORTED: dtype other than fp16 / bf16.
 *   aqlm_hip_packed_plan_*       the two host-side planning steps of the repack (pure functions, exposed for tests and tools).
 */
#define AQLM_HIP_PACKED_RELABELLED 1u   /* codebook entries were dealt to the slices: permutation + codebook image inside the buffer */
#define AQLM_HIP_PACKED_VARGEOM 2u      /* slice_groups[] is not uniform: the variable-geometry kernels serve the buffer */
#define AQLM_HIP_PACKED_HAS_CODEBOOK 4u /* the codebook image has been written (aqlm_hip_packed_set_codebook) */

#define AQLM_HIP_PREPACK_NO_RELABEL 1   /* keep the checkpoint's labelling (format v6 behaviour) */
#define AQLM_HIP_PREPACK_UNIFORM_ONLY 2 /* 16 row groups for every slice (what the shared-input / publish kernels need) */

typedef struct aqlm_hip_packed_desc {
  uint32_t magic;   /* "AQP7" */
  uint32_t version; /* 7 */
  int32_t out_features, in_features;
  int32_t slices_log2; /* 4: 16 codebook slices of 4096 entries */
  int32_t waves;       /* wave ranges per stream = waves per workgroup of the gemv kernel */
  int32_t steps;       /* KiB steps per wave range */
  int32_t entry_bytes; /* 4 */
  uint64_t used_bytes;
  uint32_t x_copies;   /* rotated copies of x the batch-1 kernel keeps in LDS (1..4); entries name the copy they read */
  float codebook_absmax; /* max |codebook entry| of the layer, set by the CALLER after prepack (prepack does not see the
                            codebook; 0 = unknown).  > 0 enables the fused finalize of aqlm_hip_gemv_1x16_packed[_multi]:
                            it bounds the slice sums, from which the kernel derives an overflow-free fixed-point scale.
                            Must be >= the true maximum (update it when the codebook is retrained); any finite value
                            that is too large only costs resolution (the sums keep ~47 bits below the bound).
                            The value travels as a kernel argument: a hipGraph that captured the launch replays with
                            the bound it was captured with -- re-capture (or capture with a generous bound) if the
                            codebook's range can grow afterwards.  A sum beyond the bound is not wrapped silently:
                            the row's result is NaN (the kernel checks |sum| <= 2 * bound). */
  uint32_t flags;        /* AQLM_HIP_PACKED_* */
  int32_t rows_per_group; /* most rows any workgroup owns (sizes the row tables; uniform geometry: ceil(out_features / row groups)) */
  uint8_t slice_groups[32]; /* workgroups (= row groups) of every slice; their sum is 256 */
} aqlm_hip_packed_desc;

size_t aqlm_hip_prepack_1x16_bytes(int out_features, int in_features, int in_group_size);
int aqlm_hip_prepack_1x16(const void* codes_i16, int out_features, int in_features, int in_group_size, void* packed,
                          size_t packed_bytes, aqlm_hip_packed_desc* desc, void* stream);
int aqlm_hip_prepack_1x16_ex(const void* codes_i16, int out_features, int in_features, int in_group_size, void* packed,
                             size_t packed_bytes, aqlm_hip_packed_desc* desc, int flags, void* stream);
int aqlm_hip_packed_set_codebook(aqlm_hip_packed_desc* desc, void* packed, const void* codebook, void* stream);
int aqlm_hip_packed_desc_read(const void* header_host, size_t header_bytes, aqlm_hip_packed_desc* desc);
int aqlm_hip_unpack_1x16(const aqlm_hip_packed_desc* desc, const void* packed, void* codes_i16, void* stream);
int aqlm_hip_dequant_1x16_packed(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                 const void* scales /* nullable */, void* W, int dtype, void* stream);
/* Host-side planning steps (no GPU work).  relabel: usage counts of the 65536 entries -> new_of_old[65536] (returns 1 and
 * fills it when the entries should be re-dealt, 0 when the slices are already even within 2 %).  geometry: lane-steps
 * (units of 4 entries) of every slice -> slice_groups[1 << slices_log2] (returns 1 when the result is not uniform). */
int aqlm_hip_packed_plan_relabel(const uint32_t* usage, int slices_log2, uint16_t* new_of_old);
/* The same deal with `force` != 0: also when the slices' total masses are already within 2 % of even -- what the repack calls
 * whenever the 16 x 16 layout is not balanced (label use correlated with the row leaves every global histogram flat; round 6). */
int aqlm_hip_packed_plan_relabel_ex(const uint32_t* usage, int slices_log2, int force, uint16_t* new_of_old);
int aqlm_hip_packed_plan_geometry(const uint64_t* slice_steps, int slices_log2, int out_features, int in_features,
                                  uint8_t* slice_groups);

/*
 * 1x16 g8 matvec for 1..AQLM_HIP_MAX_GEMV_BATCH input rows on prepacked codes: every CU keeps one 64 KiB slice of the
 * codebook in LDS and walks only the codes of that slice; the rows of x share the codes and the gathered codebook
 * vectors.  Same result contract as aqlm_hip_gemv_1x16 (which it replaces for large layers; same reference lines:
 * cuda_kernel.cu:7-95, cuda_kernel.cpp:148-182 incl. the per-row relaunch loop :165-175).  x / y row strides in elements.
 * Finalize: with desc->codebook_absmax > 0 the 16 slice workgroups of an output row add their sums as fixed-point
 * integers into one 64-bit cell INSIDE the packed buffer (order-independent, hence deterministic; the cells are zero at rest
 * and every call leaves them zero), and the last one to arrive writes y -- one kernel, no workspace (`workspace` may be
 * NULL).  The packed buffer is therefore WRITTEN by the call: do not run the same packed buffer on two streams at once.
 * With codebook_absmax == 0 the call falls back to two kernels and needs
 * workspace: aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMV_1X16_PACKED, batch, out, in) bytes of fp32 partials.
 */
int aqlm_hip_gemv_1x16_packed(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                              const void* scales, const void* bias, const void* x, void* y, int batch,
                              long x_row_stride, long y_row_stride, int dtype, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * The LDS image of the launch that aqlm_hip_gemv_1x16_packed / _cells makes for `rows` input rows of this layer under the current
 * tuning (no launch, no device needed): *lds_bytes = its dynamic LDS (of one launch: more rows than fit one image go out in
 * several), *x_window = the bytes reserved for x in front of the codebook slice -- 8208 (the compact window: one row, inputs of
 * <= 4096 features, tuning key packed_compact_window at 0), 65520 (the full window) or 0 (slice first: two and more rows, tall
 * layers).  A compact image leaves room on the CU for a workgroup of another layer, which is what lets captured launches
 * (capture overlap, below) run side by side.  With `blocks_per_cu` the runtime is asked as well (this needs a device):
 * hipOccupancyMaxActiveBlocksPerMultiprocessor for the kernel instance that launch would run, at its block size (desc->waves x 64)
 * and at `probe_lds_bytes` of dynamic LDS (0: the launch's own *lds_bytes) -- how many such workgroups the runtime lets share a CU.
 * Every output pointer may be NULL.  0, AQLM_HIP_E_INVALID / _UNSUPPORTED, or the HIP error.
 */
int aqlm_hip_gemv_1x16_packed_image(const aqlm_hip_packed_desc* desc, int rows, int dtype, size_t probe_lds_bytes, size_t* lds_bytes,
                                    uint32_t* x_window, int* blocks_per_cu);

/*
 * Re-entrant form of the single-kernel finalize: the accumulator cells are the CALLER's -- `cells` = at least
 * batch * out_features * 8 bytes, 8-B aligned, zero-filled once; every call leaves them zero.  The packed buffer is only
 * read, so the same layer may run on several streams / from several host threads at once, like the reference's stateless
 * launcher (cuda_kernel.cu:505-509); give every stream its own cells (launches on one stream are ordered, so all layers
 * of a stream can share one set).  Requires desc->codebook_absmax > 0.  Same results, bit for bit, as
 * aqlm_hip_gemv_1x16_packed.
 */
int aqlm_hip_gemv_1x16_packed_cells(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                    const void* scales, const void* bias, const void* x, void* y, int batch,
                                    long x_row_stride, long y_row_stride, int dtype, void* cells, size_t cells_bytes,
                                    void* stream);

/*
 * aqlm_hip_gemv_1x16_packed that also names the prepacked layer which runs NEXT on the same stream (chain prefetch; no
 * reference counterpart -- the reference launches each layer cold, cuda_kernel.cpp:148-182): a few extra waves of every
 * workgroup request the next layer's entry stream and codebook so that they sit in the GPU's L2 / Infinity Cache when the
 * next launch starts (a batch-1 matvec is bound by the latency of its cold start, not by HBM bandwidth, and HBM idles
 * most of the kernel).  A hint: results are identical to aqlm_hip_gemv_1x16_packed; next_* may be NULL (then it IS that
 * call).  The next layer's buffers are only read, and only inside [next_packed, next_packed + next_desc->used_bytes) and the
 * 65536 vectors of next_codebook.  The prefetch waves read the next layer's entry stream in whole KiB per workgroup; where that
 * would run past used_bytes -- a buffer of 3-byte entries that is not relabelled, whose stream of waves x steps x 776 bytes per
 * workgroup is no whole number of KiB and ends the buffer -- the hint is dropped and the call is the plain one.  So it is for a
 * variable-geometry next layer (aqlm_amd/csrc/chain_hint.h has the rule).  An invalid next_desc or a next_packed /
 * next_codebook that is not 16-byte aligned: AQLM_HIP_E_INVALID, nothing is launched.
 */
int aqlm_hip_gemv_1x16_packed_chain(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                    const void* scales, const void* bias, const void* x, void* y, int batch,
                                    long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                    size_t workspace_bytes, const aqlm_hip_packed_desc* next_desc,
                                    const void* next_packed, const void* next_codebook, void* stream);

/*
 * What aqlm_hip_gemv_1x16_packed_chain would do with its hint for `rows` input rows of this layer and this next layer under the
 * current tuning (no launch, no device needed; the entry and this report read one and the same rule): *hint_kept = 1 when the
 * next layer's entry stream is handed to the prefetch waves (0: dropped -- variable geometry, requests that would leave the
 * buffer, or the two-kernel finalize, which never prefetches), *prefetch_waves = the extra waves of every workgroup of the launch
 * that carries the hint (the last one when the rows go out in several; tuning key packed_prefetch_waves, at most 16 - desc->waves,
 * 0 when the LDS image with their landing zones would not fit the CU), *lds_bytes = the dynamic LDS of that launch.  Every output
 * pointer may be NULL.  0, or AQLM_HIP_E_INVALID / _UNSUPPORTED as the chain entry would answer for these descriptors.
 */
int aqlm_hip_gemv_1x16_packed_chain_plan(const aqlm_hip_packed_desc* desc, int rows, int dtype, const aqlm_hip_packed_desc* next_desc,
                                         int* hint_kept, int* prefetch_waves, size_t* lds_bytes);

/*
 * aqlm_hip_gemv_1x16_packed for up to AQLM_HIP_MAX_SEGMENTS prepacked layers that share x, in one launch (+ one
 * finalize; none when every descriptor carries codebook_absmax: the fused finalize of aqlm_hip_gemv_1x16_packed, which
 * writes into the packed buffers); segment.codes is the prepacked buffer, descs[s] its descriptor.  workspace (two-kernel
 * fallback only): the sum over segments of
 * aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMV_1X16_PACKED, batch, out_features_s, in_features), 16-B aligned.  Results
 * are bit-identical to separate aqlm_hip_gemv_1x16_packed calls.
 */
int aqlm_hip_gemv_1x16_packed_multi(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                    int num_segments, const void* x, int in_features, int batch, long x_row_stride,
                                    int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* aqlm_hip_gemv_1x16_packed_multi with caller-owned accumulator cells (see aqlm_hip_gemv_1x16_packed_cells): `cells` holds
 * the segments' cells back to back, batch * out_features_s * 8 bytes each, zero-filled once and left zero. */
int aqlm_hip_gemv_1x16_packed_multi_cells(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                          int num_segments, const void* x, int in_features, int batch, long x_row_stride,
                                          int dtype, void* cells, size_t cells_bytes, void* stream);

/*
 * aqlm_hip_gemv_1x16_routed on PREPACKED experts (Mixtral decode on the packed matvec): every (token, expert) pair of one or two
 * projections in one launch of 256 x num_segments x num_experts workgroups, each pair as its own batch-1 pass of
 * aqlm_hip_gemv_1x16_packed on its expert's packed buffer.  `table` is a DEVICE array of num_experts * num_segments
 * aqlm_hip_routed_packed_entry, entry [e * num_segments + s]; an entry is filled ON THE HOST by
 * aqlm_hip_routed_packed_entry_fill from the layer's descriptor, packed buffer (device address), codebook, scales and bias, so
 * that callers never derive offsets inside a packed buffer (a relabelled buffer's entry points at the codebook image inside the
 * buffer: aqlm_hip_packed_set_codebook first, and fill again whenever the codebook or its range changes -- the entry bakes
 * codebook_absmax in).  aqlm_hip_gemv_1x16_routed_packed_geometry checks the descriptors of one table (all of one shape, g8 or
 * g16) and returns the launch-wide values -- the largest wave count, the LDS image -- as a HOST struct the launch takes;
 * ..._supported is the same check as a yes / no.  AQLM_HIP_E_UNSUPPORTED (the caller keeps aqlm_hip_gemv_1x16_routed for the whole
 * block) for 3-byte entries, variable-geometry buffers (AQLM_HIP_PACKED_VARGEOM), descriptors without a codebook range, and
 * shapes the packed format refuses.
 *
 * expert_ids, x, x_row_stride, x_per_pair, top_k and y as for aqlm_hip_gemv_1x16_routed:
 *     y[(p * num_segments + s) * out_features + o] = (W[e_p, s] x_row(p))[o] * scales[o] + bias[o]
 * bit-identical to aqlm_hip_gemv_1x16_packed (batch 1) of that expert on that row, whatever the other pairs are and however
 * many there are.  Ids are only ever compared for equality with an expert index: a pair whose id lies outside
 * [0, num_experts) gets a zero row; duplicates, one expert for every pair and garbage are safe.  The grid depends on the shapes
 * only: a captured launch stays valid when the routing changes; a workgroup whose expert has no pair exits at once, an expert
 * with several pairs takes them one after the other.  `cells`: caller-owned accumulator cells [num_pairs][num_segments]
 * [out_features] u64, 8-byte aligned, ZERO at rest and zero again after the launch whatever the routing was (one set per stream).
 * x rows 16-byte aligned (x_row_stride % 8 == 0).  num_pairs <= AQLM_HIP_MAX_ROUTED_PAIRS.  Stream-ordered, no allocation, no
 * synchronisation.  aqlm_hip_gemv_1x16_routed_packed_lds_bytes: the dynamic LDS of a launch on that shape (0: shape refused).
 */
typedef struct aqlm_hip_routed_packed_entry {
  const void* entries;    /* entry stream of the packed buffer */
  const void* wave_info;
  const void* row_starts;
  const void* codebook;   /* [65536][in_group_size], or the permuted image inside a relabelled buffer */
  const void* scales;     /* [out_features] */
  const void* bias;       /* [out_features] or NULL */
  int32_t out_features, rows_per_group, waves, steps, x_copies;
  uint32_t entry_stream_bytes;
  float codebook_absmax;
  int32_t reserved;
} aqlm_hip_routed_packed_entry;

typedef struct aqlm_hip_routed_packed_geometry {
  int32_t out_features, in_features, in_group_size;
  int32_t rows_per_group; /* of every entry (uniform geometry) */
  int32_t max_waves;      /* workgroup size of the launch / 64 */
  int32_t slice_first;    /* LDS map of the launch: 1 = slice in front (row tables that do not fit behind the x window) */
  uint32_t lds_bytes;
  int32_t reserved;
} aqlm_hip_routed_packed_geometry;

size_t aqlm_hip_gemv_1x16_routed_packed_lds_bytes(int out_features, int in_features, int in_group_size);
int aqlm_hip_routed_packed_entry_fill(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                      const void* scales, const void* bias, aqlm_hip_routed_packed_entry* entry);
int aqlm_hip_gemv_1x16_routed_packed_geometry(const aqlm_hip_packed_desc* const* descs, int n,
                                              aqlm_hip_routed_packed_geometry* geom);
int aqlm_hip_gemv_1x16_routed_packed_supported(const aqlm_hip_packed_desc* const* descs, int n);
int aqlm_hip_gemv_1x16_routed_packed(const aqlm_hip_routed_packed_entry* table, const aqlm_hip_routed_packed_geometry* geom,
                                     int num_experts, int num_segments, const void* expert_ids, int ids_int64, int num_pairs,
                                     int top_k, const void* x, long x_row_stride, int x_per_pair, void* y, int dtype,
                                     void* cells, size_t cells_bytes, void* stream);

/*
 * LoRA adapters on top of a quantized layer, a different adapter for every row of a decode batch if need be (batched adapter
 * matvec; no reference counterpart -- the reference leaves adapters to PEFT's x @ A^T @ B^T * scaling + add, four generic launches
 * per layer).  An adapter cannot be merged into an AQLM base (the weights exist as codes + codebooks only), so it runs at every
 * token.  `table` is a DEVICE array of num_adapters aqlm_hip_lora_entry (8-byte aligned): A_a [rank][in_features] and B_a
 * [out_features][rank], row-major, 16-byte aligned, in the storage type of x and y; rank a multiple of 8 in 8..max_rank (an entry
 * with any other rank counts as "no adapter"); max_rank a multiple of 8 in 8..128.  ids: DEVICE [rows] int64 (ids_int64 != 0) or
 * int32, or NULL = adapter 0 for every row.  For every row b < rows with a = ids[b]:
 *     t[b, r] = sum_k A_a[r, k] * x[b, k]                                      r < rank_a   (fp32)
 *     y[b, i] = round(float(y[b, i]) + scaling_a * sum_r B_a[i, r] * t[b, r])
 * Products of storage-type operands are exact, all sums are fp32 in a fixed order, t is NEVER rounded to the storage type (PEFT
 * rounds it), y is rounded exactly once more.  An id is range-checked before it indexes the table: a row whose id lies outside
 * [0, num_adapters) is left bit for bit as it was and nothing is loaded through its table slot.  Two launches -- shrink (t into
 * `workspace`, fp32 [rows][max_rank]: aqlm_hip_lora_workspace_bytes, 16-byte aligned) and expand + add (read-modify-write of y) --
 * whose grids depend on rows, max_rank and out_features only; adapters of different rank share them.  No atomics, no
 * inter-workgroup communication: a row's bits depend on its own x row, its own y row and its adapter, never on the other rows,
 * their number or their order.  Stream-ordered, no allocation, no synchronisation (hipGraph-capturable; ids may be rewritten in
 * place between replays).  x / y row strides in elements; y 2-byte aligned with y_row_stride >= out_features (columns past
 * out_features are not touched); y must not overlap x.
 * AQLM_HIP_E_UNSUPPORTED (the caller runs the adapters as generic ops): max_rank not a multiple of 8 in 8..128, in_features % 8
 * != 0, rows > AQLM_HIP_MAX_LORA_ROWS, x rows not 16-byte aligned, dtype other than fp16 / bf16; aqlm_hip_lora_bgmv_supported
 * answers for the four sizes beforehand.  AQLM_HIP_E_INVALID: null / misaligned table, ids, y or workspace, non-positive sizes,
 * strides shorter than the rows, y overlapping x, a workspace smaller than aqlm_hip_lora_workspace_bytes.
 */
typedef struct aqlm_hip_lora_entry {
  const void* a;  /* [rank][in_features] */
  const void* b;  /* [out_features][rank] */
  int32_t rank;
  float scaling;
} aqlm_hip_lora_entry; /* 24 bytes */

#define AQLM_HIP_MAX_LORA_ROWS 256

size_t aqlm_hip_lora_workspace_bytes(int rows, int max_rank); /* rows * max_rank * 4; 0 when unsupported */
int aqlm_hip_lora_bgmv_supported(int out_features, int in_features, int max_rank, int rows);
int aqlm_hip_lora_bgmv(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const void* x, long x_row_stride, void* y, long y_row_stride, int out_features, int in_features, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same adapters on the ROUTED experts of a mixture-of-experts block: aqlm_hip_lora_bgmv with a row per (token, expert) pair
 * and projection, on top of the output of aqlm_hip_gemv_1x16_routed / ..._routed_packed / aqlm_hip_gemm_1x16_grouped (no reference
 * counterpart).  `table` is a DEVICE array of num_adapters x num_experts x num_segments aqlm_hip_lora_entry: entry
 * [(a * num_experts + e) * num_segments + s] is adapter a on projection s of expert e (num_segments 2: w1, w3 of the gate / up
 * launch; 1: w2).  A combination the adapter does not cover is an entry of rank 0 with null pointers: "no adapter", and nothing is
 * loaded through it.  adapter_ids: DEVICE, one id per TOKEN (num_pairs / top_k of them), int64 or int32, or NULL = adapter 0.
 * expert_ids: DEVICE [num_pairs] (= [tokens][top_k] row-major), int64 or int32, as for aqlm_hip_gemv_1x16_routed.  For every pair
 * p with a = adapter_ids[p / top_k] and e = expert_ids[p] -- both range-checked BEFORE either forms an address -- and every
 * segment s, with x_row(p) = x + (x_per_pair ? p : p / top_k) * x_row_stride and yrow = y + (p * num_segments + s) * out_features
 * (y is contiguous, the routed entries' output layout):
 *     t[r]    = sum_k A[r, k] * x_row(p)[k]                                    r < rank   (fp32, never rounded)
 *     yrow[i] = round(float(yrow[i]) + scaling * sum_r B[i, r] * t[r])
 * A pair whose adapter id or expert id is out of range keeps its y rows bit for bit, and so does a pair whose entry has a rank
 * that is no multiple of 8 in 8..max_rank.  The arithmetic is aqlm_hip_lora_bgmv's, operation for operation and in the same
 * order: a pair's y row is BIT-IDENTICAL to aqlm_hip_lora_bgmv called on that one row with that entry as a one-slot table, so it
 * does not depend on the other pairs, their number or their order.  Two launches (shrink into `workspace`, fp32 [num_pairs]
 * [num_segments][max_rank], 16-byte aligned; expand + add) on grids of max_rank / 2 x num_pairs x num_segments and
 * ceil(out_features / 256) x num_pairs x num_segments workgroups: the shapes only.  No atomics, no inter-workgroup
 * communication; stream-ordered, no allocation, no synchronisation (hipGraph-capturable; both id arrays may be rewritten in place
 * between replays).
 * Argument checks as aqlm_hip_lora_bgmv, in the same order (num_pairs in the place of rows), after: null expert_ids, misaligned
 * expert_ids, and non-positive num_experts / num_segments / top_k / num_pairs or num_pairs % top_k != 0 (AQLM_HIP_E_INVALID).
 * AQLM_HIP_E_UNSUPPORTED in addition for num_pairs > AQLM_HIP_MAX_LORA_ROWS, num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS and
 * num_segments > 2; aqlm_hip_lora_bgmv_routed_supported answers for the six sizes beforehand.
 */
size_t aqlm_hip_lora_bgmv_routed_workspace_bytes(int num_pairs, int num_segments, int max_rank); /* 0 when unsupported */
int aqlm_hip_lora_bgmv_routed_supported(int out_features, int in_features, int max_rank, int num_pairs, int num_experts,
                                        int num_segments);
int aqlm_hip_lora_bgmv_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments, int max_rank,
                              const void* adapter_ids, int adapter_ids_int64, const void* expert_ids, int expert_ids_int64,
                              int num_pairs, int top_k, const void* x, long x_row_stride, int x_per_pair, void* y,
                              int out_features, int in_features, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same adapters at any row count (prefill, large batches): the segmented counterpart of aqlm_hip_lora_bgmv on the matrix
 * unit, same table, same ids, same two launches.  For every row b < rows with a = ids[b] (NULL: adapter 0), a in
 * [0, num_adapters) and the entry's rank a multiple of 8 in 8..max_rank, with T the storage type of x and y:
 *     t[b, r] = sum_k A_a[r, k] * x[b, k]                                      r < rank_a   (fp32)
 *     hi = round_T(t),  lo = round_T(t - float(hi))
 *     y[b, i] = round_T(float(y[b, i]) + scaling_a * sum_r B_a[i, r] * (hi[b, r] + lo[b, r]))
 * t enters the second product as a PAIR of storage-type values (two matrix instructions per step of a sum that is only rank
 * long), which keeps the adapter term at roughly fp32 accuracy; in fp16 a |t| above 65504 has no such pair and makes the row NaN.
 * Every other row -- id out of range, or an entry whose rank is no multiple of 8 in 8..max_rank -- is left bit for bit as it was,
 * and nothing is loaded through its table slot (the id is range-checked before it forms an address).  Rows are cut into tiles of
 * 16; a tile is served in one pass per DISTINCT valid adapter among its 16 ids, and a row is written exactly once per launch:
 * per-sequence ids at prefill cost one pass per tile and two at a seam, 16 different adapters in one tile cost 16.  Both grids
 * depend on rows, max_rank, in_features and out_features only; the sum over in_features is cut by a function of in_features alone
 * and added in a fixed order, so a row's bits depend on its own x row, its own y row and its adapter, never on the other rows,
 * their number or their order.  No atomics, stream-ordered, no allocation, no synchronisation (hipGraph-capturable; ids may be
 * rewritten in place between replays).  Results are NOT bit-equal to aqlm_hip_lora_bgmv -- the sums run in another order -- but
 * both sit within the same bound of the fp64 value.  `workspace`: fp32, aqlm_hip_lora_sgmv_workspace_bytes(rows, max_rank,
 * in_features) bytes (at least rows * max_rank * 4), 16-byte aligned.  Columns of y past out_features are not touched.
 * Argument checks as aqlm_hip_lora_bgmv, in the same order, with rows up to AQLM_HIP_MAX_LORA_SGMV_ROWS; in addition
 * AQLM_HIP_E_UNSUPPORTED when y is not 8-byte aligned or, at more than one row, y_row_stride % 4 != 0 (y is written in groups of
 * 4 outputs).  aqlm_hip_lora_sgmv_supported answers for the four sizes beforehand.
 */
#define AQLM_HIP_MAX_LORA_SGMV_ROWS 65536

size_t aqlm_hip_lora_sgmv_workspace_bytes(int rows, int max_rank, int in_features); /* 0 when unsupported */
int aqlm_hip_lora_sgmv_supported(int out_features, int in_features, int max_rank, int rows);
int aqlm_hip_lora_sgmv(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids, int ids_int64, int rows,
                       const void* x, long x_row_stride, void* y, long y_row_stride, int out_features, int in_features, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * The segmented adapter GEMM on the ROUTED experts of a mixture-of-experts block (prefill, large batches): aqlm_hip_lora_sgmv
 * on row tiles gathered through the expert bucket of the grouped launches, the counterpart of aqlm_hip_lora_bgmv_routed above
 * AQLM_HIP_MAX_LORA_ROWS pairs (no reference counterpart).  `table`, adapter_ids, expert_ids, x, x_per_pair, y and top_k are
 * aqlm_hip_lora_bgmv_routed's.  `bucket`: DEVICE, 16-byte aligned, written by aqlm_hip_moe_bucket from the SAME expert_ids with
 * the same num_pairs and num_experts and tile_pairs 16.  For every pair p of a tile of the bucket, with a = adapter_ids[p / top_k]
 * (NULL: adapter 0) and e the tile's expert, and every segment s, with the entry [(a * num_experts + e) * num_segments + s],
 * x_row(p) = x + (x_per_pair ? p : p / top_k) * x_row_stride and yrow = y + (p * num_segments + s) * out_features, T the storage
 * type:
 *     t[r]    = sum_k A[r, k] * x_row(p)[k]                                    r < rank   (fp32)
 *     hi = round_T(t),  lo = round_T(t - float(hi))
 *     yrow[i] = round_T(float(yrow[i]) + scaling * sum_r B[i, r] * (hi[r] + lo[r]))
 * A pair keeps its y rows bit for bit, and nothing is loaded through its table slot, when its adapter id is out of range, its
 * expert id is out of range (such pairs sit in the bucket's tail and belong to no tile), its entry has rank 0 or its entry's rank
 * is no multiple of 8 in 8..max_rank.  One workgroup row tile is one slot of the bucket: up to 16 pairs of one expert, read through
 * the pair list, served in one pass per DISTINCT valid adapter among them, every row written exactly once; pairs stay in ascending
 * order inside an expert, so per-sequence adapter ids cost one pass per tile and two at a seam.  Both grids have
 * ceil(num_pairs / 16) + min(num_experts, num_pairs) row tiles x num_segments -- the sizes only, never the routing --, and a slot
 * at or past the bucket's tile count exits after reading that one word.  A tile record is dropped before it forms an address when
 * its expert lies outside [0, num_experts), its count outside [1, 16], its first outside [0, num_pairs - count] or an entry of its
 * list outside [0, num_pairs) (a foreign bucket, or one with larger tiles); a listed pair whose expert id is not the tile's
 * expert (a bucket of other ids) counts as a pair without an adapter.  The sum over in_features is cut as aqlm_hip_lora_sgmv
 * cuts it, by a function of in_features alone, and every sum runs in aqlm_hip_lora_sgmv's order: a pair's y row is BIT-IDENTICAL
 * to aqlm_hip_lora_sgmv called on that one row with that entry as a one-slot table, so it does not depend on the other pairs,
 * their number or their order.  `workspace`: fp32 [num_pairs][num_segments][splits][max_rank],
 * aqlm_hip_lora_sgmv_routed_workspace_bytes bytes, 16-byte aligned.  No atomics, no inter-workgroup communication;
 * stream-ordered, no allocation, no synchronisation (hipGraph-capturable; both id arrays may be rewritten in place between
 * replays when the aqlm_hip_moe_bucket launch is part of the captured step).
 * Argument checks as aqlm_hip_lora_bgmv_routed, in the same order, with num_pairs up to AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS;
 * then a null or misaligned bucket (AQLM_HIP_E_INVALID); AQLM_HIP_E_UNSUPPORTED in addition for num_experts >
 * AQLM_HIP_MAX_ROUTED_EXPERTS, num_segments > 2, and out_features % 4 != 0 or y not 8-byte aligned (y rows are written in 8-byte
 * groups at a stride of out_features); last the workspace size.  aqlm_hip_lora_sgmv_routed_supported answers for the six sizes
 * beforehand.
 */
#define AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS 65536

size_t aqlm_hip_lora_sgmv_routed_workspace_bytes(int num_pairs, int num_segments, int max_rank, int in_features); /* 0 when unsupported */
int aqlm_hip_lora_sgmv_routed_supported(int out_features, int in_features, int max_rank, int num_pairs, int num_experts,
                                        int num_segments);
int aqlm_hip_lora_sgmv_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments, int max_rank,
                              const void* adapter_ids, int adapter_ids_int64, const void* expert_ids, int expert_ids_int64,
                              const void* bucket, int num_pairs, int top_k, const void* x, long x_row_stride, int x_per_pair, void* y,
                              int out_features, int in_features, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The BACKWARD of the adapters on the routed experts (training; no reference counterpart).  With grad_y the gradient arriving
 * for y [num_pairs][num_segments][out_features], t = A x_row(p) the forward's workspace and u[p, s] = B^T grad_y[p, s] (fp32):
 *     grad_x_row(p) += scaling * A^T u[p, s]
 *     grad_A[a, e, s] = scaling * sum over the pairs p of (a, e) of  u[p, s] (x) x_row(p)          [rank][in_features]
 *     grad_B[a, e, s] = scaling * sum over the pairs p of (a, e) of  grad_y[p, s] (x) t[p, s]      [out_features][rank]
 *
 * grad_x is aqlm_hip_lora_sgmv_routed itself on a TRANSPOSED table: num_segments one-segment tables laid out
 * [num_segments][num_adapters][num_experts], the entry of (s, a, e) = {a: B^T [rank][out_features], b: A^T [in_features][rank],
 * rank, scaling} (a zero entry where the forward entry is none or has a rank that is no multiple of 8), called per segment with
 * x := grad_y[:, s, :] (pair rows, row stride num_segments * out_features), a zeroed y [num_pairs][1][in_features], in_features
 * := out_features and out_features := in_features (so both must be multiples of 8); its workspace then holds u[:, s] in
 * sgmv slices of out_features.  aqlm_hip_lora_transpose_routed fills the storage-type `buffer` that the transposed entries point
 * into: ONE launch over all entries of the forward `table`, which copies A and B of every entry whose rank is a multiple of 8 in
 * 8..max_rank and equals the rank of its transposed entry, and whose two copies lie inside [buffer, buffer + buffer_bytes) --
 * checked on the device before an address is formed; every other entry leaves the buffer as it is.  Stream-ordered, no
 * allocation, no synchronisation.  aqlm_hip_lora_transpose_routed_bytes: the buffer size when every entry has max_rank,
 * num_adapters * num_experts * num_segments * max_rank * (out_features + in_features) * 2; 0 when unsupported.
 * Checks, in order: null table / transposed / buffer, then table or transposed not 8-byte or buffer not 16-byte aligned, then a
 * size below 1 (AQLM_HIP_E_INVALID); then AQLM_HIP_E_UNSUPPORTED for max_rank no multiple of 8 in 8..128, in_features or
 * out_features no multiple of 8, num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS, num_segments > 2 or more than 65535 entries.
 *
 * aqlm_hip_lora_grad_routed is the reduction over pairs that both weight gradients are: for ONE adapter index `adapter` (adapter_ids
 * NULL: every pair has adapter 0) and every expert e and segment s, with scaling that of the entry [(adapter * E + e) * S + s],
 *     g[e][s][r][i] = scaling * sum over the pairs p of expert e whose adapter id is `adapter`, in bucket order (ascending p), of
 *                     w[p, s][r] * V[p, s][i]                                  r < max_rank, i < dim      (fp32, fused multiply-add)
 * V[p, s] = v + (v_per_pair ? p : p / top_k) * v_row_stride + s * v_seg_stride: storage-type rows of `dim` elements (elements;
 * 16-byte aligned rows).  w[p, s][r] = sum over k < w_splits, in ascending k, of
 * w[p * w_pair_stride + s * w_seg_stride + k * w_split_stride + r]: fp32, the workspace of a shrink launch.  grad_A: V = x,
 * v_seg_stride 0, w = u; grad_B^T: V = grad_y, w = the forward's workspace.  An entry that is live (rank a multiple of 8 in
 * 8..max_rank) has ALL its max_rank x dim elements written -- zeros when no pair has it, and for r >= rank --, so nothing needs
 * a memset; an entry that is not live is not touched.  `bucket`, the ids and their checks are aqlm_hip_lora_sgmv_routed's: tile
 * records, list entries and both ids are range-checked before they form an address, and a pair with an id out of range, or listed
 * under another expert than its own, contributes nothing.  No atomics, no inter-workgroup communication: the result is a function
 * of the inputs alone, bit for bit.  Stream-ordered, no allocation, no synchronisation (hipGraph-capturable).
 * Checks, in order: a null pointer (adapter_ids may be NULL), misalignment (table 8, ids their size, bucket and g 16, w 4 bytes),
 * a size below 1 / num_pairs no multiple of top_k / adapter outside [0, num_adapters), strides shorter than the rows or negative
 * (AQLM_HIP_E_INVALID); the dtype, then max_rank no multiple of 8 in 8..128, dim no multiple of 8, num_pairs >
 * AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS, num_experts > AQLM_HIP_MAX_ROUTED_EXPERTS, num_segments > 2, w_splits > 8, v not 16-byte
 * aligned or a V stride no multiple of 8 (AQLM_HIP_E_UNSUPPORTED); last g_bytes < num_experts * num_segments * max_rank * dim * 4
 * (AQLM_HIP_E_INVALID).  aqlm_hip_lora_grad_routed_supported answers for the five sizes beforehand.
 */
size_t aqlm_hip_lora_transpose_routed_bytes(int num_adapters, int num_experts, int num_segments, int max_rank, int out_features,
                                            int in_features); /* 0 when unsupported */
int aqlm_hip_lora_transpose_routed_supported(int out_features, int in_features, int max_rank, int num_experts, int num_segments);
int aqlm_hip_lora_transpose_routed(const aqlm_hip_lora_entry* table, const aqlm_hip_lora_entry* transposed, int num_adapters,
                                   int num_experts, int num_segments, int max_rank, int out_features, int in_features, void* buffer,
                                   size_t buffer_bytes, void* stream);
int aqlm_hip_lora_grad_routed_supported(int dim, int max_rank, int num_pairs, int num_experts, int num_segments);
int aqlm_hip_lora_grad_routed(const aqlm_hip_lora_entry* table, int num_adapters, int num_experts, int num_segments, int max_rank,
                              int adapter, const void* adapter_ids, int adapter_ids_int64, const void* expert_ids,
                              int expert_ids_int64, const void* bucket, int num_pairs, int top_k, const void* v, long v_row_stride,
                              long v_seg_stride, int v_per_pair, int dim, const float* w, long w_pair_stride, long w_seg_stride,
                              int w_splits, long w_split_stride, float* g, size_t g_bytes, int dtype, void* stream);

/*
 * Gradients of the continuous parameters of a 1x16 layer (one codebook of 65536 entries, out_group_size 1, in_group_size g = 8
 * or 16) from dW = grad_y^T @ x, [out_features][in_features] with a row stride in elements, fp16 / bf16 / fp32 (dw_dtype; 16-byte
 * aligned rows).  The reference gets them from autograd through its dequantisation (an embedding_bag backward: sort or atomics);
 * here the codes, which do not change while codebooks and scales train, are turned round once per layer into an inverted index:
 *     order        int32 [n_codes]     positions o * (in_features / g) + j, sorted stably by code value (codes % 65536), so that
 *                                      every entry's list is in ascending position order          (n_codes = out * in / g)
 *     starts       int32 [65537]       entry c owns order[starts[c] .. starts[c + 1])
 *     chunks       int32 [max_chunks][3]  (entry, begin, end): every list cut into pieces of at most
 *                                      AQLM_HIP_CODEBOOK_GRAD_CHUNK positions, in entry order then list order, unused entries absent;
 *                                      rows past the last chunk hold entry -1.  max_chunks = min(n_codes, 65536) + n_codes / CHUNK
 *                                      (aqlm_hip_codebook_grad_1x16_max_chunks; 0: shape refused) bounds the count for any codes
 *     chunk_starts int32 [65537]       entry c owns the chunk rows chunk_starts[c] .. chunk_starts[c + 1]
 * aqlm_hip_codebook_grad_1x16:  out[c][t] = sum over the positions (o, j) of entry c of s[o] * dW[o, j * g + t], s = scales
 * [out_features] in `dtype` (fp16 / bf16) or NULL for 1; out [65536][g] in out_dtype (fp16 / bf16 / fp32), 16-byte aligned.
 * Summation, a function of the index and of CHUNK alone: a chunk is summed in fp32 by 16 lanes -- lane l adds the chunk's
 * positions l, l + 16, ... in that order (fused multiply-add by s), then a fixed butterfly adds the lanes --; an entry of one
 * chunk writes that sum, an entry of several has its partials (`workspace`, fp32 [max_chunks][g], 16-byte aligned,
 * aqlm_hip_codebook_grad_1x16_workspace_bytes) added in chunk order by a second launch; one rounding to out_dtype.  EVERY one of
 * the 65536 x g outputs is written by every call (+0 for an entry without positions): no memset, no dependence on what out or
 * workspace held.  No atomics.  Index values are range-checked before they form an address: a chunk row with an entry outside
 * [0, 65536), a range outside [0, n_codes] or longer than CHUNK is skipped, a position outside [0, n_codes) contributes nothing.
 * aqlm_hip_scales_grad_1x16:  out[o] = sum over j, t of dW[o, j * g + t] * C[code(o, j)][t] with the canonical codes
 * [out][in / g] int16 and the UNSCALED codebook [65536][g] in `dtype`; one wave per row -- lane l adds the products of the
 * groups l, l + 64, ... in order (fp32, fused multiply-add), a fixed tree adds the lanes --, one rounding to out_dtype.
 * Both: stream-ordered, no allocation, no synchronisation (hipGraph-capturable), no scratch.  Checks, in order: a null pointer
 * (scales may be NULL), misalignment (dw / out of the codebook gradient / workspace / codebook 16 bytes, the index arrays and the
 * output of the scales gradient 4, scales and codes 2), non-positive sizes or in_features % g != 0, a row stride below in_features
 * or a workspace that is too small (AQLM_HIP_E_INVALID); then dw_dtype / out_dtype outside fp16 / bf16 / fp32, dtype outside
 * fp16 / bf16, g outside {8, 16}, more than AQLM_HIP_CODEBOOK_GRAD_MAX_CODES codes or dW rows not 16-byte aligned
 * (AQLM_HIP_E_UNSUPPORTED).  Nothing is launched on bad arguments.  The ..._supported queries answer for the three sizes.
 */
#define AQLM_HIP_CODEBOOK_GRAD_CHUNK 256
#define AQLM_HIP_CODEBOOK_GRAD_MAX_CODES (1 << 30)
int aqlm_hip_codebook_grad_chunk(void); /* AQLM_HIP_CODEBOOK_GRAD_CHUNK of the loaded library */
int aqlm_hip_codebook_grad_1x16_supported(int out_features, int in_features, int in_group_size);
int aqlm_hip_codebook_grad_1x16_max_chunks(int out_features, int in_features, int in_group_size);
size_t aqlm_hip_codebook_grad_1x16_workspace_bytes(int out_features, int in_features, int in_group_size);
int aqlm_hip_codebook_grad_1x16(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int dtype, const void* starts,
                                const void* order, const void* chunks, const void* chunk_starts, int out_features, int in_features,
                                int in_group_size, void* out, int out_dtype, void* workspace, size_t workspace_bytes, void* stream);
int aqlm_hip_scales_grad_1x16_supported(int out_features, int in_features, int in_group_size);
int aqlm_hip_scales_grad_1x16(const void* dw, long dw_row_stride, int dw_dtype, const void* codes, const void* codebook, int dtype,
                              int out_features, int in_features, int in_group_size, void* out, int out_dtype, void* stream);

/*
 * The same two gradients for the K x 8 schemes: K = num_codebooks in 1..8 codebooks of 256 entries, out_group_size 1, g in
 * {8, 16, 32}; canonical codes [out][in / g][K] int8 (the entry is the byte & 0xff), dW as above.  No index: the K * 256 * g sums
 * of the codebook gradient live in LDS while a workgroup streams its rows of dW once.
 * aqlm_hip_codebook_grad_kx8:  out [K][256][g] in out_dtype, 16-byte aligned.  The sums are taken as FIXED-POINT INTEGERS, so the
 * result is a function of the arguments alone -- integer adds commute, no schedule changes a bit -- and the sum of the quantised
 * terms is exact:
 *     P      = out_features * (in_features / g)      positions; every accumulator receives at most P terms
 *     shift  = 62 - bit_length(P)                    a function of the shape alone; |sum| <= P * 2^shift < 2^62
 *     bound  = (double)max|s| * (double)max|dW|      maxima over the layer; s = 1 when scales is NULL
 *     (m, E) = frexp(bound)                          bound = m * 2^E, m in [0.5, 1): every |s * dW| < 2^E
 *     q(o, col) = llrint((double)s[o] * (double)dW[o, col] * 2^(shift - E))
 *                 the product is exact in double, the scaling exact, round to nearest even
 *     S[c][v][t] = sum of q(o, j * g + t) over the positions (o, j) with (codes[o][j][c] & 0xff) == v        (int64, exact)
 *     out[c][v][t] = round_to_out_dtype(ldexpf((float)S, E - shift))
 *                 (float)S is the round-to-nearest-even int64 -> fp32 conversion, then the fp32 -> out_dtype rounding of the
 *                 1x16 entries
 * so |out - exact| <= n * u / 2 + (2^-24 + u_out) * (|exact| + n * u / 2) for an entry of n positions, u = 2^(E - shift), plus the
 * output's subnormal spacing.  bound == 0: every output is +0.  ANY non-finite element of dW or scales (told by the exponent
 * bits): EVERY output element is NaN -- a gradient scaler skips such a step.  Every one of the K * 256 * g outputs is written by
 * every call (+0 for an unused entry): no memset, no dependence on what out or workspace held.  Three launches: the maxima per
 * row block; the accumulation, one workgroup per (row block, pass of 64 / g codebooks) with an int64 image of at most 128 KiB in
 * LDS (64-bit integer LDS atomics; no float atomics, no global atomics); the finish, which adds the row blocks' int64 partials.
 * Row blocks:  B = min(out_features, max(1, 256 / passes)), passes = ceil(K / (64 / g)); block b owns the rows
 * [b * out / B, (b + 1) * out / B).  The result does not depend on B.  `workspace` (16-byte aligned; nothing is kept in it):
 * aqlm_hip_codebook_grad_kx8_workspace_bytes = B * K * 256 * g * 8 bytes of partials + 8192 bytes of maxima (<= 33.6 MB; the maxima
 * launch has up to 1024 row blocks of its own, two words each).
 * aqlm_hip_scales_grad_kx8:  out[o] = sum over j, t of dW[o, j * g + t] * w_j[t], w_j[t] = ((C_0[v_0][t] + C_1[v_1][t]) + ...) in
 * fp32 in codebook order, the UNSCALED codebooks [K][256][g] in `dtype` (staged in LDS); one wave per row -- lane l adds the
 * products of the groups l, l + 64, ... in order (fp32, fused multiply-add over t ascending), a fixed tree adds the lanes --, one
 * rounding to out_dtype.  Ordinary IEEE propagation: a NaN poisons its own row only.
 * Both: stream-ordered, no allocation, no synchronisation (hipGraph-capturable), no scratch.  Checks, in order: a null pointer
 * (scales may be NULL), misalignment (dw / out of the codebook gradient / workspace / codebooks 16 bytes, the output of the scales
 * gradient 4, scales 2), non-positive sizes or in_features % g != 0, a row stride below in_features or a workspace that is too
 * small (AQLM_HIP_E_INVALID); then dw_dtype / out_dtype outside fp16 / bf16 / fp32, dtype outside fp16 / bf16, K outside 1..8, g
 * outside {8, 16, 32}, 2^30 or more positions or dW rows not 16-byte aligned (AQLM_HIP_E_UNSUPPORTED).  Nothing is launched on bad
 * arguments.  The ..._supported queries answer for the four sizes.
 */
#define AQLM_HIP_CODEBOOK_GRAD_KX8_MAX_CODEBOOKS 8
#define AQLM_HIP_CODEBOOK_GRAD_KX8_MAX_ROW_BLOCKS 256
#define AQLM_HIP_CODEBOOK_GRAD_KX8_MAXIMA_BLOCKS 1024
int aqlm_hip_codebook_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size);
size_t aqlm_hip_codebook_grad_kx8_workspace_bytes(int out_features, int in_features, int num_codebooks, int in_group_size);
int aqlm_hip_codebook_grad_kx8(const void* dw, long dw_row_stride, int dw_dtype, const void* scales, int dtype, const void* codes,
                               int out_features, int in_features, int num_codebooks, int in_group_size, void* out, int out_dtype,
                               void* workspace, size_t workspace_bytes, void* stream);
int aqlm_hip_scales_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size);
int aqlm_hip_scales_grad_kx8(const void* dw, long dw_row_stride, int dw_dtype, const void* codes, const void* codebooks, int dtype,
                             int out_features, int in_features, int num_codebooks, int in_group_size, void* out, int out_dtype,
                             void* stream);

/*
 * One step of the CALIBRATED training of codebooks and scales (the reference's AQEngine._compute_mse, aq_engine.py:108-131, and its
 * backward) on fp32 master parameters.  With D = W_q - W_ref [out][in], XTX symmetric and G = D XTX (a library GEMM of the caller,
 * between the first entry and the others):
 *     loss = sum_o rowloss[o] / out,    d loss / d scales[o] = 2 / out * ds_raw[o],    d loss / d codebooks = 2 / out * dC
 * No entry applies the factor 2 / out.  All parameters are fp32: codebooks [K][S][g] (16-byte aligned), scales [out]; the codes are
 * canonical: nbits_per_codebook 16: K = 1, int16 [out][in / g], g in {8, 16}; nbits_per_codebook 8: K in 1..8, int8 [out][in / g][K]
 * (the entry is the byte & 0xff), g in {8, 16, 32}; out_group_size 1.  Row strides are in elements.
 * aqlm_hip_calib_delta:  d[o][j * g + t] = scales[o] * w_j[t] - w_ref[o][j * g + t], w_j[t] = ((C_0[v_0][t] + C_1[v_1][t]) + ...) in
 * codebook order; every operation is ONE fp32 operation (a multiply, then a subtract: no fused multiply-add), which is torch's fp32
 * `_dequantize_weight(codes, codebooks, scales) - w_ref` bit for bit.  w_ref in w_ref_dtype (fp32 / fp16 / bf16, aligned to its
 * element, any row stride >= in_features); d fp32, 16-byte aligned, d_row_stride a multiple of 4.  Codebooks of up to 64 KiB are
 * staged in LDS, larger ones (8x8 g32: 256 KiB; 1x16: 2 / 4 MiB) are gathered from L2.  One launch.
 * aqlm_hip_calib_rows:  ds_raw[o] = sum over j, t of g[o][j * g + t] * w_j[t];  rowloss[o] = sum over j, t of g[o][j * g + t] *
 * d[o][j * g + t] -- the STORED d, so nothing cancels.  g and d fp32, 16-byte aligned, row strides multiples of 4.  One wave per
 * row: lane l adds the products of the groups l, l + 64, ... in order (fp32, fused multiply-add over t ascending), a fixed tree
 * adds the lanes (the order of aqlm_hip_scales_grad_1x16).  Ordinary IEEE propagation: a NaN poisons its own row only.  One launch.
 * aqlm_hip_calib_codebook_grad_1x16:  out[c][t] (fp32 [65536][g]) = the sum of scales[o] * g[o][j * g + t] over the positions of
 * entry c -- aqlm_hip_codebook_grad_1x16 (same index, chunk size, lane order, butterfly, finish launch, workspace size) with the
 * scales read as fp32 and dW = g in fp32.  Every output is written by every call.
 * aqlm_hip_calib_codebook_grad_kx8:  the same sums by the fixed-point scheme of aqlm_hip_codebook_grad_kx8 (maxima launch, int64
 * LDS sums per pass of 64 / g codebooks, finish; same workspace size) with the scales read as fp32 -- the product s * g is then
 * exact in double as well (24 x 24 significant bits).  A non-finite element of g or scales makes EVERY output NaN.
 * All: stream-ordered, no allocation, no synchronisation (hipGraph-capturable), no scratch, no global atomics.  Checks, in the
 * order of the sibling entries: a null pointer, misalignment, non-positive sizes or in_features % g != 0, a row stride below
 * in_features or a workspace that is too small (AQLM_HIP_E_INVALID); then w_ref_dtype outside fp16 / bf16 / fp32, a scheme, K or g
 * outside the above, too many positions or fp32 rows that are not 16-byte aligned (AQLM_HIP_E_UNSUPPORTED).  Nothing is launched on
 * bad arguments.
 */
int aqlm_hip_calib_delta_supported(int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size);
int aqlm_hip_calib_delta(const void* codes, const void* codebooks, const void* scales, const void* w_ref, int w_ref_dtype,
                         long w_ref_row_stride, int out_features, int in_features, int num_codebooks, int nbits_per_codebook,
                         int in_group_size, void* d, long d_row_stride, void* stream);
int aqlm_hip_calib_rows_supported(int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size);
int aqlm_hip_calib_rows(const void* g, long g_row_stride, const void* d, long d_row_stride, const void* codes, const void* codebooks,
                        int out_features, int in_features, int num_codebooks, int nbits_per_codebook, int in_group_size, void* ds_raw,
                        void* rowloss, void* stream);
int aqlm_hip_calib_codebook_grad_1x16_supported(int out_features, int in_features, int in_group_size);
size_t aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(int out_features, int in_features, int in_group_size);
int aqlm_hip_calib_codebook_grad_1x16(const void* g, long g_row_stride, const void* scales, const void* starts, const void* order,
                                      const void* chunks, const void* chunk_starts, int out_features, int in_features,
                                      int in_group_size, void* out, void* workspace, size_t workspace_bytes, void* stream);
int aqlm_hip_calib_codebook_grad_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size);
size_t aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(int out_features, int in_features, int num_codebooks, int in_group_size);
int aqlm_hip_calib_codebook_grad_kx8(const void* g, long g_row_stride, const void* scales, const void* codes, int out_features,
                                     int in_features, int num_codebooks, int in_group_size, void* out, void* workspace,
                                     size_t workspace_bytes, void* stream);

/*
 * The V step of PV-tuning for the 1x16 schemes (one codebook of 65536 entries, out_group_size 1, g = 8 / 16): the nearest codeword
 * of every group of g weights -- the reference's `_greedy_find_best_codes` (src/beam_search_l2.py) without its 65536 x groups score
 * matrix.  For group n = o * (in_features / g) + j:
 *     r_n     = reference[o, j * g : (j + 1) * g] / scales[o]     widened to fp32 first, IEEE division; scales NULL: r_n = reference
 *     S(n, c) = |C_c|^2 - 2 <r_n, C_c>
 *     codes_out = the code with the smallest S THE KERNEL COMPUTED; equal computed scores resolve to the smallest index.  Stored as
 *     the checkpoint stores it: the 16 bits in an int16 (32768 ... 65535 are negative).
 * Accuracy: the computed score is within E(n) = eps * (|r_n|^2 + max_c |C_c|^2) of the exact one, eps =
 * AQLM_HIP_CODE_SEARCH_EPS = 2^-17, so the chosen code's exact score is at most min + 2 E(n), and the chosen code EQUALS the exact
 * argmin whenever the exact margin between the best and the second best exceeds 2 E(n).  eps follows from the arithmetic (DESIGN.md
 * 4.8m), it is not fitted: r is scaled by an exact power of two to max|r| in [2^10, 2^11) and split into two operands of the
 * codebook dtype, hi = round(r'), lo = round(r' - hi) (relative error of the pair <= 2^-21 fp16 incl. a flushed tail, 2^-18 bf16);
 * products of two 16-bit operands are exact in fp32; the matrix unit adds 2 g <= 32 of them in fp32 (<= 2^-19 of |r||C| summed);
 * |C_c|^2 is g fp32 fused multiply-adds (<= 2^-20); one fused multiply-add forms S (2^-23).  Valid while 2^-100 <= max|r_n| < 2^100
 * or r_n = 0 (above it 2 |r||C| can leave fp32: scores become infinite and tie; below it the factor of the scaling is clamped).  A
 * group with an Inf or NaN element of r_n, or beyond that range, still yields SOME value in 0 ... 65535 (non-finite: the search
 * runs with r = 0); aqlm.tuning keeps the previous code of a group that is non-finite or has max|r_n| >= 2^100.
 * group_ids NULL: every group, num_groups == out * in / g, entry i of codes_out is group i.  Else flat ids (int32, or int64 when
 * group_ids_int64) in any order, repeats allowed: entry i is the code of group group_ids[i]; an id outside [0, out * in / g) writes
 * NOTHING to its slot and forms no address.  `workspace` (16-byte aligned, nothing is kept in it):
 * aqlm_hip_code_search_1x16_workspace_bytes = 65536 * 4 bytes (|C_c|^2 in fp32, filled by a first launch of every call) for
 * 1 <= num_groups <= AQLM_HIP_CODE_SEARCH_MAX_GROUPS and g 8 / 16, else 0.  Two launches, stream-ordered, no allocation, no
 * synchronisation, no atomics, no scratch: the output is a function of the arguments alone.
 * Checks, in order: a null pointer (scales and group_ids may be NULL); misalignment (codebook / workspace 16 bytes, the others
 * their element); non-positive sizes or in_features % g != 0, a row stride below in_features, num_groups < 1 or != out * in / g
 * without group_ids (AQLM_HIP_E_INVALID); reference_dtype outside fp16 / bf16 / fp32, dtype outside fp16 / bf16, g outside {8, 16},
 * more than AQLM_HIP_CODE_SEARCH_MAX_GROUPS groups in the layer or the call (AQLM_HIP_E_UNSUPPORTED); a workspace that is too small
 * (AQLM_HIP_E_INVALID).  Nothing is launched on bad arguments.
 */
#define AQLM_HIP_CODE_SEARCH_MAX_GROUPS 2147483647L
#define AQLM_HIP_CODE_SEARCH_EPS 7.62939453125e-06 /* 2^-17 */
int aqlm_hip_code_search_1x16_supported(int out_features, int in_features, int in_group_size);
size_t aqlm_hip_code_search_1x16_workspace_bytes(long num_groups, int in_group_size);
int aqlm_hip_code_search_1x16(const void* reference, int reference_dtype, long reference_row_stride, const void* scales,
                              const void* codebook, int dtype, int out_features, int in_features, int in_group_size,
                              const void* group_ids, int group_ids_int64, long num_groups, void* codes_out, void* workspace,
                              size_t workspace_bytes, void* stream);

/*
 * Residual k-means initialisation (the reference's init_aq_kmeans, src/aq.py:288-356): one Lloyd iteration as two entries.
 *
 * aqlm_hip_kmeans_assign replaces the chunked `addmm(bmm norms, data, C^T, beta=-0.5).argmax(1)` of fit_kmeans and
 * find_nearest_cluster (src/kmeans.py:64-72, 105-112, 175-182) and, when sums_out / counts_out are given, the scatter half of
 * `index_reduce_(..., "mean", include_self=False)` (src/kmeans.py:76-80).  data [n, d] and centroids [k, d] are contiguous fp32:
 *     S(n, c)      = |C_c|^2 - 2 <x_n, C_c>
 *     codes_out[n] = the int32 index of the smallest S THE KERNEL COMPUTED; equal computed scores resolve to the smallest index.
 * Accuracy, in the form of aqlm_hip_code_search_1x16: the computed score is within E(n) = eps * (|x_n|^2 + max_c |C_c|^2) of the
 * exact one, eps = AQLM_HIP_KMEANS_EPS = 2^-17, so the chosen index EQUALS the exact argmin whenever the exact margin exceeds 2 E(n).
 * eps follows from the arithmetic: both operands are scaled by an exact power of two (a point by its own, max|x_n|
 * into [2^10, 2^11); the centroids by one for the table, max_ct |C_ct| into [2^10, 2^11)) and split into fp16 pairs hi = round(v'),
 * lo = round(v' - hi); the matrix unit sums hi.hi + lo.hi + hi.lo (d = 8: + lo.lo) of exact products in fp32; |C_c|^2 is d fp32
 * fused multiply-adds over t ascending; one fused multiply-add forms S.  Valid while every max|x_n| and max|C_ct| is 0 or in
 * [2^-50, 2^50).  A point with an Inf or NaN element searches with x = 0; a centroid with one never wins; every index is in range.
 * sums_out ([k, d] int64) and counts_out ([k] int32), both or neither: ZEROED by the entry, then point n adds q_t = rint(x_nt * 2^s)
 * (ties to even) to sums_out[codes_out[n]][t] and 1 to counts_out[codes_out[n]], s = min(40, 62 - ceil_log2(n)) - E with
 * data_absmax = m * 2^E, 1 <= m < 2 (zero and subnormal data_absmax: E = -126): integer adds, so the result does not depend on
 * their order and cannot overflow.  A point with a non-finite element or an element above data_absmax adds nothing.
 * `workspace` (16-byte aligned, nothing is kept in it): aqlm_hip_kmeans_workspace_bytes = 256 + k * 4 + k * d * 4 bytes (a header,
 * |C_c|^2, the two fp16 images of the centroids) for a supported shape, else 0.  Supported (aqlm_hip_kmeans_supported): d in {8, 16},
 * k a multiple of 128 in 128 ... AQLM_HIP_KMEANS_MAX_CENTROIDS, 1 <= n <= AQLM_HIP_KMEANS_MAX_POINTS.  Memsets and three launches,
 * stream-ordered, no allocation, no synchronisation, no scratch.
 * Checks, in order: a null pointer (sums_out and counts_out may be NULL together); misalignment (data / centroids / workspace 16
 * bytes, sums_out 8, the others 4); n, k or d below 1, or a data_absmax that is negative or not finite (AQLM_HIP_E_INVALID); a
 * shape that is not supported (AQLM_HIP_E_UNSUPPORTED); a workspace that is too small (AQLM_HIP_E_INVALID).  Nothing is launched
 * on bad arguments.
 *
 * aqlm_hip_kmeans_update replaces the mean of that index_reduce_ (src/kmeans.py:76-80): with the n and data_absmax the sums were
 * made with, centroids_inout[c][t] = (float)((double)sums[c][t] * 2^-s / (double)counts[c]) where counts[c] > 0; an empty
 * cluster keeps its centroid bit for bit (include_self=False on a clone).  One launch.  Checks: null pointer; misalignment; sizes
 * and data_absmax as above; the shape.
 */
#define AQLM_HIP_KMEANS_MAX_POINTS 2147483647L
#define AQLM_HIP_KMEANS_MAX_CENTROIDS 65536
#define AQLM_HIP_KMEANS_EPS 7.62939453125e-06 /* 2^-17 */
int aqlm_hip_kmeans_supported(long n, int k, int d);
size_t aqlm_hip_kmeans_workspace_bytes(long n, int k, int d);
int aqlm_hip_kmeans_assign(const void* data, long n, const void* centroids, int k, int d, float data_absmax, void* codes_out,
                           void* sums_out, void* counts_out, void* workspace, size_t workspace_bytes, void* stream);
int aqlm_hip_kmeans_update(const void* sums, const void* counts, long n, int k, int d, float data_absmax, void* centroids_inout,
                           void* stream);

/*
 * The V step of PV-tuning for the K x 8 schemes (1 <= K <= 8 codebooks of 256 entries, out_group_size 1, g = 8 / 16 / 32: 2x8 g8,
 * 1x8 g8, 4x8 g16, 8x8 g32 ...): the reference's `_beam_search_update_codes_groupwise` (src/beam_search_l2.py) for every group of
 * one layer, without its [groups, beams, 256] score tensor.  The entry is held to ITS OWN ARITHMETIC bit for bit, not to an error
 * bound (a beam step must get the whole order of its best beam_size + 1 scores right, and at depth a share of the groups has two
 * of them closer than any bound a kernel could promise: DESIGN.md 4.8n); tests/kx8_search_model.py restates it in numpy.  Every
 * operation below is ONE IEEE fp32 operation, rounded to nearest; there are no fused multiply-adds.  For group
 * n = o * (in_features / g) + j, with the codebooks C_c [256][d = g] widened exactly from fp16 / bf16 to fp32:
 *     r        = float(reference[o, j * g : (j + 1) * g]) / float(scales[o])        a true division; scales NULL: r = reference
 *     dot(a,b) : acc = a_0 * b_0, then acc = acc + a_j * b_j for j = 1 .. d - 1     (the product is rounded, then the sum)
 *     cn[c][s] = dot(C_c[s], C_c[s])
 *     kept     = C_0[p_0], then kept = kept + C_c[p_c] for c = 1 .. K - 1           p: prev_codes of the group, the int8 mod 256
 *     res[0]   = r - kept                                                           one position, whose beam is p
 *     for each step c of dim_order (a permutation of 0 .. K - 1; NULL: 0, 1 .. K - 1):
 *         res[b]  = res[b] + C_c[beam[b][c]]                                        for each position b
 *         rn[b]   = dot(res[b], res[b])
 *         S(b, s) = (rn[b] - 2 * dot(res[b], C_c[s])) + cn[c][s]                    (the doubling is exact; the same formula at
 *                                                                                    beam_size 1, where the reference drops rn)
 *         keep the best 1 hypothesis on the last step, else min(beam_size, positions * 256), ordered by (S, b * 256 + s)
 *         ascending: equal scores compare as floats (-0 equals +0) and go to the smaller flat index; rank i takes the codes of
 *         its source position b with code c replaced by s;
 *         not the last step: res[i] = res_old[i] - C_c[chosen_i], POSITION BY POSITION as the reference does it -- the residue of
 *         old position i stays at position i even when the hypothesis now at i came from another position; after the first step
 *         every new position starts from old position 0
 *     codes_out = the codes of rank 0 (int8 [num_groups, K], the 8 bits as the checkpoint stores them: 128 .. 255 are negative);
 *     scores_out (fp32 [num_groups], may be NULL) = its S on the last step.
 * The contract holds while every element of r and of the codebooks is finite and below 2^60 in magnitude.  Outside that range the
 * kernel still writes SOME code in 0 .. 255 per codebook: no address and no source position is derived from a score, so NaNs can
 * neither index out of range nor stall a loop; aqlm.tuning keeps the previous codes of such a group.
 * reference: fp32 / fp16 / bf16, any row stride >= in_features (elements).  codebooks [K, 256, g] fp16 / bf16, 16-byte aligned;
 * scales [out] in the same dtype, or NULL.  prev_codes int8 [out * in / g, K] for the WHOLE layer, read at the group's id.
 * group_ids as in aqlm_hip_code_search_1x16: NULL = every group (num_groups == out * in / g, entry i is group i), else flat ids
 * (int32, or int64 when group_ids_int64) in any order, repeats allowed; an id outside [0, out * in / g) writes NOTHING to its slot
 * of codes_out / scores_out and forms no address.  aqlm_hip_code_search_kx8_workspace_bytes is 0: `workspace` may be NULL (|C|^2 is
 * formed from the registers that hold the candidates).  One launch, stream-ordered, no allocation, no synchronisation, no global
 * atomics, no scratch: the output is a function of the arguments alone.
 * Supported (aqlm_hip_code_search_kx8_supported): 1 <= K <= 8, g in {8, 16, 32}, 1 <= beam_size <=
 * AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM, in_features % g == 0, at most AQLM_HIP_CODE_SEARCH_MAX_GROUPS groups.
 * Checks, in the order of aqlm_hip_code_search_1x16: a null pointer (scales, dim_order, group_ids, scores_out and workspace may be
 * NULL); misalignment (codebooks 16 bytes, the others their element); non-positive out / in / g or in_features % g != 0, a row
 * stride below in_features, num_groups < 1 or != out * in / g without group_ids (AQLM_HIP_E_INVALID); reference_dtype outside fp16 /
 * bf16 / fp32, dtype outside fp16 / bf16, K, g or beam_size outside the supported set, too many groups (AQLM_HIP_E_UNSUPPORTED); a
 * dim_order (host memory) that is no permutation (AQLM_HIP_E_INVALID).  Nothing is launched on bad arguments.
 */
#define AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM 16
int aqlm_hip_code_search_kx8_supported(int out_features, int in_features, int num_codebooks, int in_group_size, int beam_size);
size_t aqlm_hip_code_search_kx8_workspace_bytes(long num_groups, int num_codebooks, int in_group_size, int beam_size); /* may be 0 */
int aqlm_hip_code_search_kx8(const void* reference, int reference_dtype, long reference_row_stride, const void* scales,
                             const void* codebooks, int dtype, const void* prev_codes, int out_features, int in_features,
                             int num_codebooks, int in_group_size, int beam_size, const int* dim_order /* host, NULL = natural */,
                             const void* group_ids, int group_ids_int64, long num_groups, void* codes_out, void* scores_out /* NULL ok */,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * The CALIBRATED code search of the K x 8 schemes: one input group of the reference's src/beam_search_xtx.py, the beam search that
 * minimises ||X W_ref^T - X W_q^T||^2 through XTX = X^T X, for every output row o of one layer; all K codebook steps of the group run
 * in the launch.  With E_b = W_ref[o] - W_b[o] the error of beam position b and T_b = E_b XTX, the group's steps
 * need only the slice t[b] = T_b[group] (g numbers), H = XTX[group, group] and q[c][s] = C_c[s] H C_c[s]^T (unscaled; the caller
 * forms it).  Like aqlm_hip_code_search_kx8 the entry is held to ITS OWN ARITHMETIC bit for bit (tests/kx8_xtx_model.py restates it
 * in numpy): every operation below is ONE IEEE fp32 operation rounded to nearest, no fused multiply-adds, sums over f ascending
 * (acc = a_0 * b_0, then acc = acc + a_f * b_f).  For row o with scale s = float(scales[o]) (scales NULL: s = 1), 2s = 2 * s (exact),
 * ss = s * s, the codebooks widened exactly to fp32, and P positions (positions_in at entry), position b holding loss L[b], slice
 * t[b], the group's codes beam[b] (codes_in, the int8 mod 256), entry position src[b] = b and weight change d[b] = 0:
 *     for each step c of dim_order (a permutation of 0 .. K - 1; NULL: 0, 1 .. K - 1), p = beam[b][c]:
 *         w[b][f]  = s * C_c[p][f]
 *         u[b][f'] = t[b][f'] + sum_f w[b][f] * H[f][f']
 *         base[b]  = (L[b] + 2s * sum_f C_c[p][f] * u[b][f]) - ss * q[c][p]
 *         S(b, s') = (base[b] - 2s * sum_f C_c[s'][f] * u[b][f]) + ss * q[c][s']          a result of -0 is replaced by +0
 *         keep the best min(beam_size, P * 256) = beam_size hypotheses -- on EVERY step, the last one too: the reference returns
 *         position 0 only at the end of its call -- ordered by (S, b * 256 + s') ascending: equal scores go to the smaller flat
 *         index.  Rank i, from source position b with code s':
 *             beam[i] = beam[b] with code c replaced by s';  src[i] = src[b];  L[i] = S(b, s')
 *             dw[f]    = s * C_c[s'][f] - s * C_c[p][f]
 *             d[i][f]  = d[b][f] + dw[f]
 *             t[i][f'] = t[b][f'] - sum_f dw[f] * H[f][f']
 *         (state follows the hypothesis: the reference re-dequantises every survivor)
 *     loss_out [beam_size][out] fp32 = L;  codes_out [beam_size][out][K] int8 (128 .. 255 negative);  source [beam_size][out] uint8 = src,
 *     the position AT ENTRY a hypothesis descends from;  delta [beam_size][out][g] fp32 = d, the group's new weights minus those of the
 *     source position at entry, scaled (the caller owes T_b[other columns] -= delta XTX[group, other columns]);  t_out
 *     [beam_size][out][g] fp32 (may be NULL) = t.  Rank 0 is the best.
 * t: fp32 [positions_in][out][g] with element strides per position and per row (a view into a wider buffer works), g contiguous;
 * loss fp32 [positions_in][out]; codes_in int8 [positions_in][out][K]; H fp32 [g][g] (not assumed symmetric); q fp32 [K][256];
 * codebooks [K][256][g] fp16 / bf16, 16-byte aligned; scales [out] in the same dtype or NULL; dim_order in host memory or NULL.
 * No address, LDS slot or source position is formed from a score: NaN / Inf in t, loss, H or q still give codes in 0 .. 255 and
 * sources below positions_in, and cannot stall a loop.  One launch, stream-ordered, no allocation, no synchronisation, no global
 * atomics, no scratch; aqlm_hip_code_search_kx8_xtx_workspace_bytes is 0 and `workspace` may be NULL: the output is a function of
 * the arguments alone.
 * Supported (aqlm_hip_code_search_kx8_xtx_supported): out >= 1, 1 <= K <= 8, g in {8, 16, 32}, 1 <= beam_size, positions_in <=
 * AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM.
 * Checks, in the order of aqlm_hip_code_search_kx8: a null pointer (scales, dim_order, t_out and workspace may be NULL); misalignment
 * (codebooks 16 bytes, the others their element); out or g below 1, a row stride of t below g, or a position stride below g with
 * several positions (AQLM_HIP_E_INVALID); dtype outside fp16 / bf16, K, g, beam_size or positions_in outside the supported set
 * (AQLM_HIP_E_UNSUPPORTED); a dim_order that is no permutation (AQLM_HIP_E_INVALID).  Nothing is launched on bad arguments.
 */
int aqlm_hip_code_search_kx8_xtx_supported(int out_features, int num_codebooks, int in_group_size, int beam_size, int positions_in);
size_t aqlm_hip_code_search_kx8_xtx_workspace_bytes(int out_features, int num_codebooks, int in_group_size, int beam_size); /* 0 */
int aqlm_hip_code_search_kx8_xtx(const void* t, long t_position_stride, long t_row_stride, const void* loss, const void* codes_in,
                                 const void* h, const void* q, const void* codebooks, int dtype, const void* scales, int out_features,
                                 int num_codebooks, int in_group_size, int beam_size, int positions_in,
                                 const int* dim_order /* host, NULL = natural */, void* loss_out, void* codes_out, void* source_out,
                                 void* delta_out, void* t_out /* NULL ok */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The CALIBRATED code search of the 1x16 schemes (one codebook of 65536 entries, out_group_size 1, g = 8 / 16): one input group of
 * the same search for every output row o of one layer.  It is aqlm_hip_code_search_kx8_xtx with K = 1 and 65536
 * candidates per position, and it is held to the same arithmetic bit for bit (tests/x16_xtx_model.py restates it in numpy): every
 * operation below is ONE IEEE fp32 operation rounded to nearest, no fused multiply-adds, sums over f ascending from the first
 * product.  For row o with scale s = float(scales[o]) (scales NULL: s = 1), 2s = 2 * s, ss = s * s, and position b of positions_in
 * holding loss L[b], slice t[b] and code p = codes_in[b] (the int16 mod 65536):
 *     w[f]     = s * C[p][f]
 *     u[b][f'] = t[b][f'] + sum_f w[f] * H[f][f']
 *     base[b]  = (L[b] + 2s * sum_f C[p][f] * u[b][f]) - ss * q[p]
 *     S(b, s') = (base[b] - 2s * sum_f C[s'][f] * u[b][f]) + ss * q[s']                  a result of -0 is replaced by +0
 *     keep the best beam_size of the positions_in * 65536 hypotheses, ordered by (S, b * 65536 + s') ascending: equal scores go to
 *     the smaller flat index; NaN scores come last, in the order of their flat indices.  Rank i, from (b, s'):
 *         codes_out[i] = s';  source[i] = b;  loss_out[i] = S(b, s')
 *         dw[f] = s * C[s'][f] - s * C[p][f];  delta[i][f] = dw[f];  t_out[i][f'] = t[b][f'] - sum_f dw[f] * H[f][f']
 * The 65536 scores of a position are never all formed in this arithmetic: the matrix unit scans approximate scores, and a candidate
 * is re-scored exactly unless its approximate score exceeds the largest of the beam_size best exact scores met so far by more than
 * a bound E on the approximation's error, derived from the arithmetic.  The result is the definition's whatever
 * the order of the scan.  A rank that only a NaN score could take gets position 0 and the smallest code not yet among the ranks
 * before it, with loss NaN (the definition's answer when the scores of position 0 are NaN).
 * t: fp32 [positions_in][out][g] with element strides per position and per row, g contiguous; loss fp32 [positions_in][out];
 * codes_in / codes_out int16 [positions][out] (32768 .. 65535 negative); H fp32 [g][g] (not assumed symmetric); q fp32 [65536],
 * q[s] = C[s] H C[s]^T unscaled, 16-byte aligned; codebook [65536][g] fp16 / bf16, 16-byte aligned; scales [out] in the same dtype or
 * NULL; loss_out fp32 [beam_size][out]; source uint8 [beam_size][out]; delta and t_out (may be NULL) fp32 [beam_size][out][g].
 * No address, LDS slot or loop bound is formed from a score: NaN / Inf in t, loss, H or q still give codes in 0 .. 65535 and
 * sources below positions_in, and cannot stall a loop (a column whose bound is not finite refines every candidate).  Three
 * stream-ordered launches through `workspace` (aqlm_hip_code_search_1x16_xtx_workspace_bytes, 16-byte aligned): the maxima of |C|
 * and |q|, the scan over column blocks x codebook splits, the merge of a row's lists.  No allocation, no synchronisation, no global
 * atomics, no scratch: the output is a function of the arguments alone.
 * Supported (aqlm_hip_code_search_1x16_xtx_supported): out >= 1, g in {8, 16}, 1 <= beam_size, positions_in <=
 * AQLM_HIP_CODE_SEARCH_1X16_XTX_MAX_BEAM.
 * Checks, in the order of aqlm_hip_code_search_kx8_xtx: a null pointer (scales and t_out may be NULL); misalignment; out or g below 1,
 * a row stride of t below g, or a position stride below g with several positions (AQLM_HIP_E_INVALID); dtype outside fp16 / bf16, g,
 * beam_size or positions_in outside the supported set (AQLM_HIP_E_UNSUPPORTED); a workspace below the size the query returns
 * (AQLM_HIP_E_INVALID).  Nothing is launched on bad arguments.
 */
#define AQLM_HIP_CODE_SEARCH_1X16_XTX_MAX_BEAM 8
int aqlm_hip_code_search_1x16_xtx_supported(int out_features, int in_group_size, int beam_size, int positions_in);
size_t aqlm_hip_code_search_1x16_xtx_workspace_bytes(int out_features, int in_group_size, int beam_size, int positions_in);
int aqlm_hip_code_search_1x16_xtx(const void* t, long t_position_stride, long t_row_stride, const void* loss, const void* codes_in,
                                  const void* h, const void* q, const void* codebook, int dtype, const void* scales, int out_features,
                                  int in_group_size, int beam_size, int positions_in, void* loss_out, void* codes_out, void* source_out,
                                  void* delta_out, void* t_out /* NULL ok */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Row-parallel ("in"-split) layers over several MI355X: the finalize of the prepacked matvec fused with a ONE-SHOT
 * all-reduce over xGMI (no reference counterpart -- the reference has no tensor parallelism; BASELINE.json north star:
 * the 70B layer 8192 -> 28672 split over 8 GPUs).  Every rank runs aqlm_hip_gemv_1x16_packed_partials on its shard (the
 * main kernel only: fp32 slice partials [16][batch][out] in `workspace`), then aqlm_hip_xgmi_finalize: it publishes the
 * slice-summed vector in a buffer the peers have mapped (IPC), raises a flag, waits (bounded) for the peers' flags, reads
 * their vectors over xGMI and adds them in rank order, then scale + bias + one rounding -- y is bit-identical on every rank.
 * State per rank: one device allocation of aqlm_hip_xgmi_state_bytes(max_elems) bytes, zero-filled except epoch = 1, laid
 * out as  [pub: 2 x max_elems fp32][flag: 2 x u32 at byte 8 * max_elems][epoch, 2 tickets: 3 x u32 at +64][arrival counters of
 * aqlm_hip_gemv_1x16_packed_publish: 9 x u32 at +80][status: u32 at +128];
 * `peer_pub[r]` / `peer_flag[r]` are DEVICE arrays (world entries) of the peers' pub / flag addresses as mapped into this
 * process (own entries included).  Collective semantics: every rank calls it the same number of times.  On a time-out
 * (spin_limit polls, 0 = default ~seconds) status becomes 1 and y is NaN.  Graph-capturable (the epoch lives in device memory).
 */
typedef struct aqlm_hip_xgmi {
  const void* const* peer_pub;   /* device array [world] of float* */
  const void* const* peer_flag;  /* device array [world] of uint32_t* */
  void* epoch;                   /* this rank's epoch / ticket words (device) */
  void* status;                  /* this rank's status word (device) */
  int rank, world, max_elems;
  uint32_t spin_limit;
} aqlm_hip_xgmi;

size_t aqlm_hip_xgmi_state_bytes(int max_elems);
int aqlm_hip_gemv_1x16_packed_partials(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook, const void* x,
                                       int batch, long x_row_stride, int dtype, void* workspace, size_t workspace_bytes,
                                       void* stream);
int aqlm_hip_xgmi_finalize(const aqlm_hip_xgmi* xg, const void* partials, const void* scales, const void* bias, void* y,
                           int out_features, int batch, long y_row_stride, int dtype, void* stream);
/*
 * Two launches instead of three: aqlm_hip_gemv_1x16_packed_publish is the shard's matvec with the single-kernel finalize
 * (descriptor with codebook_absmax > 0) whose last-arrival branch writes the row's fp32 total into this rank's pub buffer
 * (`pub_own` / `flag_own` = the rank's own pub and flag addresses, i.e. peer_pub[rank] / peer_flag[rank]) and whose last
 * workgroup raises the flag; then aqlm_hip_xgmi_finalize with partials == NULL runs the reduce only (poll the peers' flags,
 * add the vectors in rank order, scale + bias + one rounding).  AQLM_HIP_E_UNSUPPORTED when the rows do not fit one launch
 * or the codebook range is unknown: use the partials form above.  State words used: epoch + 4 .. + 12 (arrival counters).
 */
int aqlm_hip_gemv_1x16_packed_publish(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook, const void* x,
                                      int batch, long x_row_stride, int dtype, const aqlm_hip_xgmi* xg, void* pub_own,
                                      void* flag_own, void* stream);

/*
 * Batch-1 matvec for 8 x 8-bit schemes (e.g. the 2-bit 8x8 g32 models; in_group_size 8, 16 or 32) through per-token
 * look-up tables in LDS:  lut[j,c,v] = <codebooks[c,v], x_j>,  y[i] = sum lut[j,c,codes[i,j,c]]  -- the formulation of
 * the reference's CPU kernel (numba_kernel.py:37-48) mapped onto LDS slabs.  Same result contract as aqlm_hip_gemv_kx8
 * (which it replaces for num_codebooks == 8; reference route: triton_kernel.py).  workspace:
 * aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMV_8X8_LUT, in_group_size, out, in) bytes  [note: the `batch` slot carries
 * in_group_size for this op].
 */
int aqlm_hip_gemv_8x8_lut(const void* codes_i8, const void* codebooks, const void* scales, const void* bias,
                          const void* x, void* y, int out_features, int in_features, int in_group_size, int dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * aqlm_hip_gemv_8x8_lut for up to AQLM_HIP_MAX_SEGMENTS 8-codebook layers that share x (batch 1) in one launch
 * (+ one finalize).  workspace: the sum over segments of
 * aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMV_8X8_LUT, in_group_size, out_features_s, in_features).  A row's value does
 * not depend on how the rows are dealt to workgroups, so results equal separate aqlm_hip_gemv_8x8_lut calls bit for bit.
 */
int aqlm_hip_gemv_8x8_lut_multi(const aqlm_hip_segment* segments, int num_segments, const void* x, int in_features,
                                int in_group_size, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same two operations in ONE kernel each (no finalize launch): the slab sums of an output row are added as fixed-point
 * integers into one 64-bit cell (one returning atomic per slab and row; integer adds commute, so the result does not
 * depend on the arrival order: deterministic), and the workgroup that finds all other slabs arrived applies scale and
 * bias, rounds once, writes y and puts the cell back to zero.  The fixed-point unit is derived inside the kernel from
 * max|codebook| and max|x| (both read by every workgroup): no overflow whatever the data; non-finite inputs give NaN.
 * `cells`: out_features (multi: the sum over the segments, in segment order) x 8 bytes, 8-B aligned, ZERO-FILLED by the
 * caller once after allocation; every call leaves them zero.  A set of cells serves one launch at a time (stream order);
 * keep one per layer, or one per stream.
 */
int aqlm_hip_gemv_8x8_lut_fused(const void* codes_i8, const void* codebooks, const void* scales, const void* bias,
                                const void* x, void* y, int out_features, int in_features, int in_group_size, int dtype,
                                void* cells, size_t cells_bytes, void* stream);
int aqlm_hip_gemv_8x8_lut_multi_fused(const aqlm_hip_segment* segments, int num_segments, const void* x, int in_features,
                                      int in_group_size, int dtype, void* cells, size_t cells_bytes, void* stream);

/*
 * Planar layout of 8 x 8-bit codes (ABI 5): [8 codebooks][out_features][jp] bytes, jp = in_features / in_group_size rounded up
 * to 4 (padding bytes zero) -- the checkpoint's [out][in_groups][8] transposed, same size, lossless.  With it a workgroup of the
 * look-up-table matvec serves ONE codebook x 128 input groups: it fetches 16 KiB of codebook (g = 32) instead of all 128 KiB
 * and reads its codes as 128 contiguous bytes per row.  Load-time re-layout, the counterpart of the reference's code
 * permutation for its CPU look-up kernel (inference.py:78-83).  aqlm_hip_8x8_planar_bytes returns 0 for impossible sizes;
 * buffers 8-byte aligned; pack / unpack are plain kernels on `stream` (no sync, capturable).
 */
size_t aqlm_hip_8x8_planar_bytes(int out_features, int in_features, int in_group_size);
int aqlm_hip_8x8_planar_pack(const void* codes_i8, int out_features, int in_features, int in_group_size, void* planar,
                             size_t planar_bytes, void* stream);
int aqlm_hip_8x8_planar_unpack(const void* planar, int out_features, int in_features, int in_group_size, void* codes_i8,
                               void* stream);

/*
 * aqlm_hip_gemv_8x8_lut[_fused] / _multi[_fused] on planar codes (replaces the same reference route, triton_kernel.py:30-125,
 * reached through kernel_selector.py:91-94).  `fused` != 0: `workspace` = zero-at-rest cells as for the _fused entries, and
 * `codebook_absmax` (> 0, a bound of max |codebook entry| over ALL 8 codebooks, e.g. taken at load time) replaces the in-kernel
 * maximum -- a workgroup sees one codebook only, and every workgroup of a row must derive the same fixed-point unit; a bound
 * that is too large only costs resolution, one that is too small gives NaN rows, never a wrong number.  `fused` == 0:
 * `workspace` = aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMV_8X8_LUT, ...) bytes of fp32 partials, `codebook_absmax` ignored.
 * _multi: segments[k].codes = the segment's planar buffer, codebook_absmax[k] its bound.  Results equal the canonical-layout
 * entries up to fp32 summation order (other slab shape), and _multi equals the single-layer entry bit for bit.
 */
int aqlm_hip_gemv_8x8_lut_planar(const void* planar, const void* codebooks, const void* scales, const void* bias, const void* x,
                                 void* y, int out_features, int in_features, int in_group_size, int dtype, float codebook_absmax,
                                 void* workspace, size_t workspace_bytes, int fused, void* stream);

/*
 * The look-up-table matvec for 1..AQLM_HIP_MAX_GEMV_BATCH input rows in ONE launch (round 5; single-kernel form): row b of x
 * runs as its own set of workgroups (tables are functions of x; what the rows share is the launch and the codes in L2) with its
 * own zero-at-rest cells -- `cells` = batch * out_features * 8 bytes -- and its own output row.  `planar` != 0: `codes` is the
 * planar buffer of aqlm_hip_8x8_planar_pack and codebook_absmax must be > 0; else canonical codes (codebook_absmax ignored).
 * A row's bits equal those of the same row launched alone through the batch-1 entries.
 * Replaces: the per-row loop around the reference's generic gemv for 8x8 (triton_kernel.py:161-182).
 */
int aqlm_hip_gemv_8x8_lut_batch(const void* codes, const void* codebooks, const void* scales, const void* bias, const void* x,
                                void* y, int out_features, int in_features, int in_group_size, int batch, long x_row_stride,
                                long y_row_stride, int dtype, int planar, float codebook_absmax, void* cells, size_t cells_bytes,
                                void* stream);
int aqlm_hip_gemv_8x8_lut_planar_multi(const aqlm_hip_segment* segments, const float* codebook_absmax, int num_segments,
                                       const void* x, int in_features, int in_group_size, int dtype, void* workspace,
                                       size_t workspace_bytes, int fused, void* stream);

/*
 * Large-batch path of the 8-bit schemes (ABI 6): Y[B][out] = (X[B][in] @ W^T) * scales + bias for 1 or 2 codebooks of 256 x 8
 * (1x8 g8, 2x8 g8), W never materialised: the codebooks live in LDS, a block owns 16 output rows over all of K, every lane
 * takes its lanes of the 16 x 32 MFMA fragments straight from the codebook entries its code bytes name (one MFMA per codebook:
 * exact products, fp32 sums -- W is never rounded), X streams through LDS.  No workspace, one launch per 128 batch rows.
 * At <= 32 rows (<= 16: ABI 7) X is RESIDENT in LDS instead: a workgroup loads the X image once (in phases when batch x in_features x 2
 * bytes exceed the LDS, and for 17 .. 32 rows: ABI 8) and walks 16-row tiles with nothing to synchronise inside a tile; a row's bits then depend neither on
 * the other rows of the call nor on their number.
 * Replaces: code2x8_matmat_dequant / code1x8_matmat_dequant = Code2x8Dequant / CodeKx8Dequant + F::linear(cuBLAS) + epilogue
 * (cuda_kernel.cpp:450-484, 615-649; kernels cuda_kernel.cu:235-294, 392-468).
 * AQLM_HIP_E_UNSUPPORTED (the caller dequantises + calls its GEMM, like the reference): other schemes, in_features not a
 * multiple of 128 or < 384, X rows not 16-B aligned.
 */
int aqlm_hip_gemm_kx8_mfma(const void* codes_i8, const void* codebooks, const void* scales, const void* bias, const void* X,
                           void* Y, int batch, int out_features, int in_features, int num_codebooks, int in_group_size,
                           long x_row_stride, long y_row_stride, int dtype, void* stream);

/*
 * 8 codebooks of 256 x 32 (8x8 g32, 2 bits per weight) at 2 .. many batch rows (ABI 8): Y[B][out] = (X[B][in] @ W^T) * scales + bias,
 * W never materialised.  The eight codebooks (128 KiB) live in LDS as 16-byte piece planes; a workgroup owns 16-row output tiles over
 * all of K, a group of 32 features is one k-step of v_mfma_f32_16x16x32 whose A fragment lanes gather their piece of the entry
 * the lane's code byte names -- one MFMA per codebook, so the eight terms of a weight meet in the fp32 accumulator (exact
 * products, fp32 sums; W is never rounded).  Codes in the CHECKPOINT layout [out][in_groups][8] (not the planar copy).  No
 * workspace, one launch per 64 batch rows; a row's bits do not depend on the other rows of the call nor on their number.
 * Replaces: the reference's Triton kernel looped over the rows (triton_kernel.py:161-182) and, above the gemv rule's 6 rows,
 * dequantize_gemm = _dequantize_weight + F.linear (dequantization.py:9-21, utils.py:43-70) for this scheme.
 * AQLM_HIP_E_UNSUPPORTED (the caller takes its other routes): group sizes other than 32, in_features not a multiple of 256 or
 * < 2048, codes / codebooks / X rows not 16-B aligned.
 */
int aqlm_hip_gemm_8x8_mfma(const void* codes_i8, const void* codebooks, const void* scales, const void* bias, const void* X, void* Y,
                           int batch, int out_features, int in_features, int in_group_size, long x_row_stride, long y_row_stride,
                           int dtype, void* stream);

/*
 * aqlm_hip_gemm_kx8_mfma with a workspace (ABI 8): at 49+ batch rows every 16-row block of the no-workspace form pulls all of X
 * (batch x in_features x 2 bytes: 1 MiB at 128 rows of a 4096-wide layer) through its CU's L1; given `workspace` (16-B aligned,
 * aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMM_KX8_MFMA, batch, out_features, in_features) bytes) the entry takes two row tiles per
 * block and deals the K range to 2 or 4 blocks -- half / a quarter of the X bytes per CU -- whose fp32 tiles a second small kernel
 * sums in slice order before scale, bias and the one rounding (deterministic; results differ from the no-workspace form only in
 * the order of the fp32 sums).  workspace == NULL or too small: exactly aqlm_hip_gemm_kx8_mfma.
 */
int aqlm_hip_gemm_kx8_mfma_ws(const void* codes_i8, const void* codebooks, const void* scales, const void* bias, const void* X,
                              void* Y, int batch, int out_features, int in_features, int num_codebooks, int in_group_size,
                              long x_row_stride, long y_row_stride, int dtype, void* workspace, size_t workspace_bytes, void* stream);

#define AQLM_HIP_OP_GEMM_1X16_MFMA 1
#define AQLM_HIP_OP_GEMM_KX8_MFMA 6
#define AQLM_HIP_OP_GEMV_1X16_PACKED 3
#define AQLM_HIP_OP_GEMV_8X8_LUT 4
#define AQLM_HIP_OP_GEMV_1X16_G16_PACKED 5 /* prepacked codes of 16-element vectors: 32 slices */
size_t aqlm_hip_workspace_bytes(int op, int batch, int out_features, int in_features);

/*
 * 128-bit position-sensitive checksum of a device buffer: out[0] = sum of its 32-bit words, out[1] = sum of word_i * (odd
 * multiplier of i), both mod 2^64 (trailing 1-3 bytes count as one zero-padded word).  `out_u64x2` is 16 bytes of DEVICE memory,
 * overwritten; stream-ordered, no synchronisation (the caller reads it back).
 * What it is for: everything this library DERIVES from the parameters at load time (prepacked / planar codes, the codebook image
 * and range, a dense copy of W) goes stale when a caller overwrites a parameter through a path that leaves no trace on the host
 * (`tensor.data.copy_()` does not bump the version counter).  The reference has no such state -- its launcher reads the live
 * tensors on every call (cuda_kernel.cpp:148-182) -- so the host side re-checks this checksum every few hundred calls
 * (aqlm_amd/inference.py, DERIVED_CHECK_EVERY) and rebuilds what no longer matches.
 */
int aqlm_hip_checksum(const void* data, size_t bytes, void* out_u64x2, void* stream);

/*
 * Capture overlap -- the ordering contract of aqlm_hip_gemv_1x16_packed, _cells, _chain, _multi and _multi_cells.
 * Outside a stream capture nothing differs from every other entry: stream-ordered.  On a stream that is being captured
 * (hipStreamBeginCapture / torch.cuda.graph) the first kernel of such a call is ordered after everything captured before it
 * EXCEPT earlier calls of these same entries in an unbroken run whose argument footprints it does not touch; everything
 * captured after it, by this library or by anyone else, is ordered after all of them.
 *   - footprint of a call, from its arguments and descriptor: the rows of x it uses, the packed buffer(s), codebook, scales,
 *     bias (read); the rows of y, the accumulator cells (those inside the packed buffer, or the caller's) and the workspace
 *     when used (written).  Two calls touch when two of their ranges overlap and at least one is written.  Memory a call
 *     reaches in no other way than through these arguments is all it may assume about: a caller that aliases buffers the
 *     arguments do not show (none of the entries allows that) gets no ordering for them.
 *   - a run is broken by any other node or wait on the capturing stream between two calls: another entry of this library, a
 *     kernel of the framework, a memcpy, an event wait, a change of the dependency set by the caller.
 *   - at most `packed_capture_window` (tuning key, 1..8, default 2) calls of a run are left unordered among themselves; the
 *     next one waits for the oldest.  1 = every call after the previous one, exactly the graph that stream order gives.
 *     Every branch of the replayed graph wants a hardware queue of its own out of the 4 a process opens by default; with 3 or
 *     4 branches two of them can land on one queue, depending on the streams the process created before, and most of the
 *     gain is lost.  Two branches were the fastest in every placement measured.
 *   - a run leaves nothing unordered until it holds `packed_capture_min_run` calls (tuning key, default 8; 1 = from the second
 *     call on).  A graph with branches is replayed at about 2 us of host time per node, for every node of the graph; that pays
 *     where these calls are most of the graph (a stack of linears) and not in a decoder's graph of thousands of short framework
 *     kernels, whose runs of these calls (q/k/v, gate/up) are short.  Below the threshold the graph is the one stream order gives.
 *   - results are the same bits either way.  A graph captured this way has parallel branches: replay it with at least the
 *     default number of hardware queues.
 *   - should the runtime refuse the capture calls (hipStreamGetCaptureInfo_v2, hipStreamUpdateCaptureDependencies), the
 *     launch goes out stream-ordered, the feature switches itself off for the process and aqlm_hip_last_error() says so;
 *     the call fails only if a launch that was already moved can no longer be joined to the stream.
 * aqlm_hip_capture_overlap_stats: out[0..5] = calls seen on a capturing stream, relaxed (no edge to any call of the run), kept
 * for a conflict, kept for the window, runs started or broken, capture-call failures; process-wide, since the last reset.
 * NULL resets the counters.  Returns 0.
 *
 * Grouped launches (tuning key `packed_capture_merge`, 1..8, default 4; 1 = off).  Every node of a replayed graph pays a launch
 * boundary and waits for the last workgroup of the node before it; within one launch the hardware puts the next workgroup
 * on a CU the moment one leaves.  With the key at n > 1, a one-row call of aqlm_hip_gemv_1x16_packed / _cells / _chain whose
 * layer runs on the compact-window kernels (<= 4096 input features, 4-byte entries, codebook range in the descriptor) and
 * that would have waited for the oldest call of a full window JOINS the node of an earlier such call of the same kernel
 * instance, block size and LDS image instead (same shape, in practice), up to n calls per node: the node is rewritten
 * (hipGraphKernelNodeSetParams) to a grouped kernel that runs the layers as segments of one grid, each with its own x,
 * codebook, cells and y.  A joined call has been checked against the footprint of every call it can run beside, the ones
 * it shares the node with included; ordering towards everything captured later is as above.  Same bits.  Nothing changes
 * outside a capture, in runs shorter than `packed_capture_min_run`, or for any other launch.  Should the runtime refuse the
 * rewrite, the call is captured as a node of its own, as with the key at 1, and the refusal is counted.
 * Folded nodes (tuning key `packed_group_fold`: 0 = default, which is 4; 1 = off; 2; 4).  A node of n >= F calls of ordinary
 * geometry whose layers have at most one row of a row group per thread of the block runs as n * 256 / F workgroups instead of
 * n * 256: a workgroup fills its 64 KiB codebook slice and x once and walks F row groups of its (layer, slice) in turn, where
 * the unfolded grid fills them once per row group.  Chosen again at every join, so a node below F calls, a variable-geometry
 * node and every launch outside a grouped node run the kernels they ran before.  Same LDS image, same block size, same bits.
 * The head of a run (tuning key `packed_capture_head`: 1 = on, the default; 0 = off).  The first `packed_capture_min_run` calls
 * of a run are captured as a chain of single launches, because only the last of them shows that the run is long.  At that call
 * they are regrouped in place: calls of one kernel instance, block size and LDS image share grouped / folded nodes of up to
 * `packed_capture_merge` calls, exactly the nodes later calls get; the head stays one chain in stream order, its first nodes are
 * rewritten (hipGraphKernelNodeSetParams) and the nodes left over are destroyed from the end of the chain
 * (hipStreamUpdateCaptureDependencies, hipGraphDestroyNode), each a node nothing depends on.  Only a head whose calls are
 * pairwise free of hazards is regrouped; a call of a kernel with no grouped form keeps a node to itself.  Same bits; out[0..8]
 * count what they counted before, at the time each call was planned.  Runs shorter than `packed_capture_min_run` are not touched.
 * Should the runtime refuse a step, the graph is correct as it stands (a call may then run twice, one copy after the other, writing
 * the same bits), the capture goes on, the refusal is counted and no head is regrouped again in this process.
 * aqlm_hip_capture_overlap_stats_ex: the first `count` (0..13) of out[0..5] as above, then out[6] = calls that joined a node
 * (they are also counted in out[3]), out[7] = rewrites the runtime refused, out[8] = calls that added a node of their own
 * (out[0] - out[6]), out[9] = nodes that run the folded kernel (the head's included), out[10] = runs whose head was regrouped,
 * out[11] = head calls that gave up a node of their own (the nodes destroyed), out[12] = head regroupings that stopped early.
 * NULL resets all counters.  Returns 0, or AQLM_HIP_E_INVALID for a count outside 0..13.  (A caller that asks for 9 or 10 gets
 * what it got before.)
 */
int aqlm_hip_capture_overlap_stats(uint64_t out[6]);
int aqlm_hip_capture_overlap_stats_ex(uint64_t* out, int count);

/*
 * Tuning / experiment knobs (process-wide, not part of the reference surface; defaults are the shipped
 * configuration).  Unknown keys return AQLM_HIP_E_INVALID.  Keys: struct Tuning in aqlm_amd/csrc/aqlm_common.h.
 */
int aqlm_hip_set_tuning(const char* key, int value);
int aqlm_hip_get_tuning(const char* key, int* value);

#ifdef __cplusplus
}
#endif
#endif /* AQLM_HIP_H_ */

// 1x16 g8 matvec (1..8 input rows) on slice-bucketed ("prepacked") codes, gfx950.  Packed format v7.
//
// Why a load-time repack: on MI355X a random 16-B codebook gather that hits L2 costs a whole 128-B line of the CU's
// L1-fill path (0.43 lane-gathers/clk/CU measured, profiles/r01_call1_mb_l2gather.log), which pins the direct kernel
// (gemv.hip) at ~5.5 % of the HBM roofline.  LDS gathers are >10x cheaper but only 160 KiB fit per CU, so the codebook is
// cut into S = 16 slices of 4096 entries (64 KiB), one slice per workgroup -- and every workgroup must find "its" codes.
// Bucketing the codes by slice ONCE, when the layer is loaded, removes that search.  (The reference also re-lays codes
// out at load time for its CPU kernel, inference.py:78-83.)
//
// Format v7 = format v6 + balancing at pack time (round 5; the reference's kernels are data-oblivious -- one warp per
// output row, cuda_kernel.cu:16-27 -- while a slice-bucketed kernel is only as fast as its fullest slice):
//   * relabelling: the 65536 codebook entries are dealt to the slices by how often the layer uses them (LPT greedy), so the
//     slices carry equal numbers of codes whatever the checkpoint's labelling; the permutation (unpack stays bit-exact) and a
//     permuted image of the codebook (what the kernels read) live behind the entries.  Evenly used codebooks keep their labels.
//   * variable geometry (16-B vectors): an entry used by more than 1/16 of the codes cannot be balanced by labels; the 256
//     workgroups are then dealt to the slices in proportion to their work: slice s gets n_s row groups of M / n_s rows
//     (stream index = slice-major; block -> stream keeps an XCD on 32 consecutive streams, i.e. on 2-3 slices).
// Format v6 (built by aqlm_hip_prepack_1x16; specification + simulation: tests/packed_model.py):
//   rows -> NG = 16 row-groups of RG rows; codes -> S = 16 slices by (code >> 12); workgroup (g, s) owns stream (g, s).
//   In a stream every row's codes of the slice are rounded up to whole LANE-STEPS of 4 entries (>= 1; null entries pad)
//   and the lane-steps of rows 0, 1, 2, ... are laid end to end.  The sequence is cut into NW wave ranges of 64*T
//   lane-steps, a wave range into 64 lane COLUMNS of T lane-steps: lane l of wave w walks lane-steps
//   [(w*64 + l)*T, +T).  Entry (w, t, l, k) is stored at (((st*NW + w)*T + t)*64 + l)*4 + k, so step t of a wave is ONE
//   contiguous KiB at an address that depends on nothing but (st, w, t): no bucket table, no dependent round trip
//   before the first code arrives (format v4 needed rowoff -> entries).
//   entry = (j << 4 | fhi) << 16 | (code & 0xfff) << 4 | flo: `half & 0xfff0` IS the LDS byte offset of x[j] resp. of
//   the codebook vector (one v_and_b32_sdwa each).  The spare nibbles carry the bookkeeping: bit 0 of a lane-step's
//   first entry = "a row ends with this lane-step"; the first lane-step of every column carries the column's starting
//   slot (15 bits over the remaining spare bits of entries 0 and 1).  null entry: j = in_groups (a zero vector in LDS).
//   winfo[st][w] = {first row that STARTS in wave w, wave starts inside a row, steps with content, start row of lane 0}
//   (read by the 3-byte-entry kernel and the unpacker; the 4-byte kernel runs all T steps of every wave range -- the
//   tail is null entries -- and finds the start rows in the entries).  rowstart[st][RG + 1] = first lane-step of every
//   row of the stream (epilogue).  Optional 3-byte entries (entry_bytes = 3, T <= 32): a wave range = T 8-byte row-end
//   flag words, then T steps of 64 x 12 B holding 4 x (slot:12 | code:12); 3.5 instead of 4.5 B per code, same speed.
//   4 bytes per code + 6 bytes of padding per (row, slice) on average + < 1 step per wave of tail: 4.5 B per code for
//   4096-wide layers, 4.2 for 8192-wide ones (canonical: 2 B per code).
//
// Kernel: grid = 256 workgroups = 16 groups x 16 slices (slice = block % 16 -> the two slices block % 8 and
// block % 8 + 8 live in one XCD's L2).  Slice, x and the stream's row-start table go to LDS by LDS-DMA
// (global_load_lds: no VGPR staging, no ds_write pass); the entry stream runs PD steps ahead in a register ring from
// fixed addresses, so it is in flight before the LDS fill completes.  A lane accumulates its column in fp32; at the
// lane-step that ends a row it STORES the sum to rowval[row] (exactly one lane-step per row does: unique writer, no
// atomics), at the end of its column it stores what it gathered after its last row end to colend[column].  Epilogue:
// row r = rowval[r] + the colend of the columns the row crosses before its last one, in column order (from the
// row-start table) -> the summation order inside a workgroup is fixed.  The 16 slice sums of a row then meet in one 64-bit
// cell of the packed buffer: fixed-point integers added with ONE returning atomic each (order-independent, hence
// deterministic); the workgroup that finds 15 earlier arrivals applies scale + bias, rounds once, writes y and zeroes
// the cell.  The fixed-point unit comes from max|x| (taken from the x image in LDS) and the layer's codebook range
// (descriptor): no overflow whatever the data.  Without a codebook range the kernel leaves fp32 partials
// [slice][batch][row] in a workspace and a second kernel finalizes.  Per entry: 2 v_and_sdwa + 2 ds_read_b128 + 4 v_dot2c (x B for B
// input rows: one codebook read, B x reads).  The kernels take their leading parameters as scalar arguments: the
// command processor preloads them into SGPRs (-amdgpu-kernarg-preload-count), so no kernel-argument fetch precedes the
// first load.
#include <algorithm>
#include <vector>

#include "aqlm_common.h"
#include "chain_hint.h"  // when aqlm_hip_gemv_1x16_packed_chain passes the next layer on to its prefetch waves (host only)

// The file is compiled twice: as it is for 8-element codebook vectors (16 B; 16 slices of 4096 entries x 16 row groups), and
// through gemv_packed_g16.hip for 16-element vectors (AQLM_PK_G 16, AQLM_PK_S_LOG 5, AQLM_PK_NG_LOG 3: 32 B per entry, 32 slices
// of 2048 entries = 64 KiB, 8 row groups; two ds_read_b128 per side and entry).  The second build lives in its own namespace
// and exports its entry points under aqlm_hip_g16_*; the public entries of the first build forward to them (in_group_size 16 /
// a descriptor with slices_log2 == 5).  Matches the reference kernel's template on g in {8, 16} (cuda_kernel.cu:476-521).
#ifndef AQLM_PK_G
#define AQLM_PK_G 8
#endif
#ifndef AQLM_PK_S_LOG
#define AQLM_PK_S_LOG 4  // 16 slices of 64 KiB; 5 = 32 slices of 32 KiB (experiment builds: tools/microbench)
#endif
#ifndef AQLM_PK_NG_LOG
#define AQLM_PK_NG_LOG (8 - AQLM_PK_S_LOG)  // row groups: by default PK_S * PK_NG == 256 workgroups == CUs
#endif
#ifndef AQLM_PK_XFIRST
#define AQLM_PK_XFIRST 1  // batch-1 LDS map: 1 = x first (a 64 KiB window, x copies possible), 0 = slice first (LDS = slice + x: several workgroups per CU)
#endif

// The entry points that exist in both builds, without their aqlm_hip_ prefix.  Every one of them is declared in
// include/aqlm_hip.h; its twin aqlm_hip_g16_<name> gets the SAME type from that declaration (hidden: reached through the public
// entries only).  A definition names itself PK_ENTRY(<name>): the 8-element build defines the public symbol, the 16-element
// build the twin, so each is compiled against a declaration taken from the header -- extern "C" does not overload, a parameter
// that drifts is "conflicting types" in whichever build it happens.
#define PK_TWIN_ENTRIES(X)                                                                                                     \
  X(prepack_1x16_bytes) X(prepack_1x16) X(prepack_1x16_ex) X(packed_set_codebook) X(packed_plan_relabel)                       \
  X(packed_plan_relabel_ex) X(packed_plan_geometry) X(packed_desc_read) X(unpack_1x16) X(dequant_1x16_packed)                  \
  X(gemv_1x16_packed_cells) X(gemv_1x16_packed) X(gemv_1x16_packed_chain) X(gemv_1x16_packed_partials)                         \
  X(gemv_1x16_packed_publish) X(gemv_1x16_packed_multi) X(gemv_1x16_packed_multi_cells) X(gemv_1x16_routed_packed_lds_bytes)   \
  X(routed_packed_entry_fill) X(gemv_1x16_routed_packed_geometry) X(gemv_1x16_routed_packed_supported)                         \
  X(gemv_1x16_routed_packed) X(gemv_1x16_packed_image) X(gemv_1x16_packed_chain_plan)
#define PK_TWIN_DECLARE(name) extern "C" __attribute__((visibility("hidden"))) decltype(aqlm_hip_##name) aqlm_hip_g16_##name;
PK_TWIN_ENTRIES(PK_TWIN_DECLARE)
#undef PK_TWIN_DECLARE

// Per build: the namespace (PK_NS), the name a definition gives itself (PK_ENTRY) and its visibility (PK_API), and
// PK_G16_FORWARD(descriptor, name, args...) / PK_G16_FORWARD_IF(condition, name, args...), the first statement of a public entry
// of the 8-element build: hand the call to the twin when it is for the 32-slice format.  Nothing in the 16-element build.
#if AQLM_PK_G == 16
#define PK_NS pk_g16
#define PK_ENTRY(name) aqlm_hip_g16_##name
#define PK_API __attribute__((visibility("hidden")))  // internal to libaqlm_hip.so: reached through the public entries only
#define PK_G16_FORWARD(desc_expr, name, ...)
#define PK_G16_FORWARD_IF(cond, name, ...)
#else
#define PK_NS pk_g8
#define PK_ENTRY(name) aqlm_hip_##name
#define PK_API
// a descriptor of the twin's format (32 slices)
static inline bool pk_is_g16(const aqlm_hip_packed_desc* d) { return d && d->slices_log2 == 5; }
#define PK_G16_FORWARD_IF(cond, name, ...) \
  if (cond) return aqlm_hip_g16_##name(__VA_ARGS__)
#define PK_G16_FORWARD(desc_expr, name, ...) PK_G16_FORWARD_IF(pk_is_g16(desc_expr), name, __VA_ARGS__)
#endif

// The rest of this file is its eight sections, kept in files of their own.  They are not headers: no include guards and no
// #include of their own (each is read once per build, i.e. twice per library), and the order of the #include lines below, with
// the order of the kernels inside each part, is the order of the kernels in the code object.
namespace aqlm {
namespace PK_NS {
#include "packed_format.h"          // constants, stream geometry, buffer layout, wave-count choice
#include "packed_repack_kernels.h"  // load-time kernels: histogram, count, arrange, compress, unpack, dequantise
#include "packed_gemv_kernels.h"    // matvec: params, LDS maps, body, kernel wrappers, finalize kernels
#include "packed_pipe_kernel.h"     // pipelined shared-input kernel (q/k/v in one launch) and its eligibility rule
#include "packed_launch.h"          // host launch helpers: kernel dispatch, LDS budget
}  // namespace PK_NS
}  // namespace aqlm

using namespace aqlm;
using namespace aqlm::PK_NS;

#include "packed_repack_entries.h"  // repack planning and the C entries of prepack, codebook image, unpack, dequantise
#include "packed_gemv_entries.h"    // matvec launch code and the C entries of the single-layer and shared-input matvec
#include "gemv_packed_routed.h"     // expert-routed launch (MoE decode): its kernel, then its C entries

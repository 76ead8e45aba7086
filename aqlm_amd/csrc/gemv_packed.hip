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
  X(gemv_1x16_routed_packed)
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

// packed_format.h, packed_gemv_kernels.h, packed_launch.h and gemv_packed_routed.h are sections of this file kept in files of
// their own, not headers: no include guards (each is read once per build, i.e. twice per library), and the order of the kernels
// here and in them is their order in the code object.
namespace aqlm {
namespace PK_NS {

#include "packed_format.h"  // constants, stream geometry, buffer layout, wave-count choice

// ------------------------------------------------------------------------------------------------ prepack
// K0: how often every codebook entry is used (the relabelling plan is made from it on the host).
__global__ __launch_bounds__(256) void pk_hist_kernel(const uint16_t* codes, size_t n, uint32_t* hist) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) atomicAdd(&hist[codes[i]], 1u);
}

// K1: lane-steps per (slice, row) -> ls[s][row] (u16), and their totals per slice.  One wave per row.  `relabel` (nullable):
// new label of every checkpoint label.
__global__ __launch_bounds__(256) void pk_count_kernel(const uint16_t* codes, const uint16_t* relabel, uint16_t* ls, uint32_t* slice_steps,
                                                       int M, int in_groups) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  uint32_t cnt[PK_S];
#pragma unroll
  for (int s = 0; s < PK_S; ++s) cnt[s] = 0;
  for (int j = lane; j < in_groups; j += 64) {
    uint32_t code = codes[(size_t)row * in_groups + j];
    if (relabel) code = relabel[code];
    const uint32_t sl = code >> PK_CODE_BITS;
#pragma unroll
    for (int s = 0; s < PK_S; ++s) cnt[s] += (sl == (uint32_t)s);
  }
#pragma unroll
  for (int s = 0; s < PK_S; ++s) {
    uint32_t v = cnt[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    if (lane == 0) {
      const uint32_t steps = v == 0 ? 1u : (v + 3u) >> 2;
      ls[(size_t)s * M + row] = (uint16_t)steps;
      atomicAdd(&slice_steps[s], steps);
    }
  }
}

// K2: per stream, exclusive prefix sum of its rows' lane-steps -> a[st][0..RG] (entries past the stream's rows = its total);
// maxL = longest stream.
__global__ __launch_bounds__(256) void pk_scan_kernel(const uint16_t* ls, uint32_t* a, uint32_t* maxL, const PkGeom G) {
  __shared__ uint32_t sums[256];
  const int st = blockIdx.x;
  int sl, row0, nrows;
  pk_stream_rows(G, st, sl, row0, nrows);
  const uint16_t* src = ls + (size_t)sl * G.M + row0;
  uint32_t* row = a + (size_t)st * (G.RG + 1);
  const int t = threadIdx.x;
  const int n = G.RG + 1;
  const int chunk = (n + 255) / 256;
  const int lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += i < nrows ? (uint32_t)src[i] : 0u;
  sums[t] = s;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const uint32_t v = sums[i];
      sums[i] = run;
      run += v;
    }
    atomicMax(maxL, run);
  }
  __syncthreads();
  uint32_t run = sums[t];
  for (int i = lo; i < hi; ++i) {
    row[i] = run;
    run += i < nrows ? (uint32_t)src[i] : 0u;
  }
}

__global__ __launch_bounds__(256) void pk_fill_kernel(uint32_t* p, size_t n, uint32_t v) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

__device__ __forceinline__ size_t pk_entry_index(uint32_t q, int k, size_t st, int NW, int T) {
  const uint32_t w = q / (64u * T), rem = q - w * 64u * T;
  const uint32_t l = rem / T, t = rem - l * T;
  return ((((size_t)st * NW + w) * T + t) * 64 + l) * 4 + k;
}

// K3: scatter the entries, ascending j inside every (row, slice).  One wave per row.
__global__ __launch_bounds__(256) void pk_scatter_kernel(const uint16_t* codes, const uint16_t* relabel, const uint32_t* a, uint32_t* ent,
                                                         const PkGeom G, int in_groups, int NW, int T) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= G.M) return;
  uint32_t cnt[PK_S];  // entries of this row already placed, per slice
#pragma unroll
  for (int s = 0; s < PK_S; ++s) cnt[s] = 0;
  for (int j0 = 0; j0 < in_groups; j0 += 64) {
    const int j = j0 + lane;
    const bool ok = j < in_groups;
    uint32_t code = ok ? codes[(size_t)row * in_groups + j] : 0u;
    if (relabel) code = relabel[code];
    const uint32_t sl = ok ? (code >> PK_CODE_BITS) : 0xffffffffu;
#pragma unroll
    for (int s = 0; s < PK_S; ++s) {
      const bool mine = sl == (uint32_t)s;
      const unsigned long long m = __ballot(mine);
      if (mine) {
        int st, r;
        pk_row_stream(G, s, row, st, r);
        const uint32_t i = cnt[s] + __popcll(m & ((1ull << lane) - 1ull));
        const uint32_t q = a[(size_t)st * (G.RG + 1) + r] + (i >> 2);
        ent[pk_entry_index(q, i & 3, (size_t)st, NW, T)] = ((uint32_t)j << (16 + PK_VSH)) | ((code & (PK_SLICE_ENTRIES - 1)) << PK_VSH);
      }
      cnt[s] += __popcll(m);
    }
  }
}

// K3c (32-byte vectors): stamp the lane parity into every entry (see PK_PARITY_BITS); entry (.., t, lane, k) sits at
// word ((..) * 64 + lane) * 4 + k.
__global__ __launch_bounds__(256) void pk_parity_kernel(uint32_t* ent, size_t n) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    ent[i] = (ent[i] & ~PK_PARITY_BITS) | (((i >> 2) & 1u) ? PK_PARITY_BITS : 0u);
}

// K3b: bank-aware order of the entries.  In the gemv kernel the 64 lanes of a wave execute entry slot (t, k) together:
// one ds_read_b128 for the codebook vectors, one for the x vectors.  The LDS services such a read in four groups of 16
// lanes (MI355X_MICROARCH.md: {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) and needs one extra cycle for every lane whose
// 16-B slot falls into a bank group (slot % 16) another lane of its group already uses: random slots cost ~3 cycles per
// group instead of 1 for both reads, and the loop is LDS-bound.  Two freedoms are used against that:
//   * a row's entries may be summed in any order: inside a wave range the entries of a row form a POOL that is re-dealt
//     over the row's slots (greedy, slot by slot; within a slot the lanes of a service group choose one after the other
//     with rotating priority; a lane takes from its row's pool the first entry whose codebook bank group AND x bank group
//     are still free in its service group, else a null entry -- all nulls read the same two addresses, which the LDS
//     broadcasts --, else one that is free in one of the two);
//   * x is small: the batch-1 kernel keeps XC copies of it in LDS, copy c rotated by 4 c bank groups, and an entry names
//     the copy it reads -- so the x side almost always finds a free bank group and the pool choice serves the codebook.
// The order of choices is fixed -> the layout is deterministic.  One wave per (stream, wave range): the 64 lanes scan
// the pool in parallel, the picks themselves are sequential.  Wave ranges of more than 32 steps keep ascending-j order.
constexpr int PK_ARR_MAX_T = 32;

__device__ __forceinline__ int pk_group_lane(int grp, int pos) {  // inverse of (service group, position) -> lane
  const int half = grp >> 1, g1 = grp & 1;
  int h;
  if (!g1) h = pos < 4 ? pos : (pos < 8 ? pos + 8 : pos + 12);          // G0: 0-3, 12-15, 20-27
  else h = pos < 8 ? pos + 4 : (pos < 12 ? pos + 8 : pos + 16);          // G1: 4-11, 16-19, 28-31
  return half * 32 + h;
}

__global__ __launch_bounds__(64) void pk_arrange_kernel(const uint32_t* a, uint32_t* ent, const PkGeom G, int in_groups, int NW,
                                                        int T, int XC) {
  extern __shared__ uint32_t arr_sm[];
  uint32_t* pool = arr_sm;                                                   // [64 * T * 4] entries in (lane, t, k) order
  uint16_t* rowa = reinterpret_cast<uint16_t*>(pool + (size_t)T * 256);    // [64 * T] first lane-step (in the wave range) of the slot's row
  uint16_t* rem = rowa + (size_t)T * 64;                                    // [64 * T] entries left in the pool of the row starting at that lane-step
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int sl_, row0_, nrows;
  pk_stream_rows(G, (int)st, sl_, row0_, nrows);
  const uint32_t* starts = a + st * (G.RG + 1);
  const uint32_t total = starts[nrows];
  uint32_t* wave_ent = ent + (((size_t)st * NW + w) * T) * 256;             // + (t * 64 + lane) * 4 + k
  const uint32_t w0 = (uint32_t)w * 64u * (uint32_t)T;
  const uint32_t q0 = w0 + (uint32_t)l * (uint32_t)T;
  for (int t = 0; t < T; ++t) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(wave_ent + ((size_t)t * 64 + l) * 4);
    *reinterpret_cast<u32x4*>(pool + ((size_t)l * T + t) * 4) = v;
  }
  {  // row range of every lane-step of this column, clipped to the wave range
    int r = nrows;
    if (q0 < total) {  // last r with starts[r] <= q0
      int lo = 0, hi = nrows;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= q0) lo = mid; else hi = mid;
      }
      r = lo;
    }
    for (int t = 0; t < T; ++t) {
      const uint32_t q = q0 + (uint32_t)t;
      uint32_t ra = q - w0, rb = ra + 1;  // trailing null lane-steps: pools of one step
      if (q < total) {
        while (starts[r + 1] <= q) ++r;
        const uint32_t rs = starts[r], re = starts[r + 1];
        ra = rs > w0 ? rs - w0 : 0u;
        rb = re < w0 + 64u * (uint32_t)T ? re - w0 : 64u * (uint32_t)T;
      }
      rowa[l * T + t] = (uint16_t)ra;
      if (q - w0 == ra) rem[ra] = (uint16_t)((rb - ra) * 4u);
    }
  }
  __syncthreads();
  const uint32_t null_j = (uint32_t)in_groups;
  const uint32_t xstride = (uint32_t)pk_x_stride(in_groups);
  for (int s = 0; s < 4 * T; ++s) {
    const int t = s >> 2, k = s & 3;
    for (int grp = 0; grp < 4; ++grp) {
      uint32_t ux = 0u, uc = 0u;  // bank groups taken in this (slot, service group); wave-uniform
      bool null_placed = false;   // the null entry's two addresses are already being read (further nulls are free)
      for (int r = 0; r < 16; ++r) {
        const int tl = pk_group_lane(grp, (r - s) & 15);  // the lane whose turn it is
        const uint32_t par = PK_G == 16 ? (uint32_t)(tl & 1) : 0u;  // 32-byte vectors: odd lanes read the upper half first
        const uint32_t null_x = 1u << (((null_j << (PK_VSH - 4)) & 15u) ^ par), null_c = 1u << par;
        const uint32_t ra = rowa[tl * T + t];
        const uint32_t n = rem[ra];
        const uint32_t base = ra * 4u;
        uint32_t key = 0u;  // (score + 1) << 20 | copy << 16 | (0xffff - index): the maximum is the best, lowest-index candidate
        for (uint32_t i = (uint32_t)l; i < n; i += 64u) {
          const uint32_t v = pool[base + i];
          const uint32_t j = v >> (16 + PK_VSH);
          uint32_t score, copy = 0u;
          if (j == null_j) score = (null_placed || (!(ux & null_x) && !(uc & null_c))) ? 3u : 0u;
          else {
            const bool cf = !((uc >> (((v >> 4) & 15u) ^ par)) & 1u);
            bool xf = false;
            for (uint32_t c = 0; c < (uint32_t)XC; ++c)
              if (!((ux >> ((((j << (PK_VSH - 4)) + 4u * c) & 15u) ^ par)) & 1u)) { xf = true; copy = c; break; }
            score = xf && cf ? 4u : (xf ? 2u : (cf ? 1u : 0u));
          }
          const uint32_t kk = ((score + 1u) << 20) | (copy << 16) | (0xffffu - i);
          key = kk > key ? kk : key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t other = (uint32_t)__shfl_xor((int)key, o, WAVE);
          key = other > key ? other : key;
        }
        if (key == 0u) __builtin_trap();  // every slot of a row has an entry left in the row's pool
        const uint32_t idx = 0xffffu - (key & 0xffffu), copy = (key >> 16) & 3u;
        const uint32_t v = pool[base + idx];           // same address in every lane: broadcast
        const uint32_t j = v >> (16 + PK_VSH);
        if (j != null_j) {
          ux |= 1u << ((((j << (PK_VSH - 4)) + 4u * copy) & 15u) ^ par);
          uc |= 1u << (((v >> 4) & 15u) ^ par);
        } else {
          ux |= null_x;
          uc |= null_c;
          null_placed = true;
        }
        __syncthreads();  // everybody has read pool[base + idx] and rem[ra]
        if (l == 0) {
          const uint32_t out = j == null_j ? v : ((v & ((1u << (16 + PK_VSH)) - 1u)) | ((j + copy * xstride) << (16 + PK_VSH)) | (copy << 16));
          wave_ent[((size_t)t * 64 + tl) * 4 + k] = out;
          pool[base + idx] = pool[base + n - 1u];      // swap-remove
          rem[ra] = (uint16_t)(n - 1u);
        }
        __syncthreads();
      }
    }
  }
}

// K3c: local search on the greedy deal.  The greedy order is good in a wave range's early slots and poor in its last ones
// (the pools run dry: whatever is left must be taken).  This pass walks the slots again; an entry that shares its codebook
// or x bank group with another lane of its service group looks at every other position of its row's pool and swaps with
// the one that lowers
//     cost(slot, service group) = 8 * (max_b count_c[b] + max_b count_x[b]) + sum_b count_c[b]^2 + sum_b count_x[b]^2
// (the max terms are the LDS cycles of the two reads, the squares break ties towards flatter histograms) the most, summed
// over the two (slot, service group) cells the swap touches; swaps that leave the cost unchanged are taken too (they walk
// plateaus), PK_IMPROVE_SWEEPS passes (3 for long wave ranges).  tools/arrangement_bound.py: LDS cycles per service group and read 2.18 + 1.70 ->
// 1.6 + 1.5 (lower bound of any order 1.27 + 1.26, simulated annealing 1.57 + 1.43).  Same launch shape and the same fixed
// order of decisions as K3b -> deterministic.  Entries are still plain here (parity, flags and row numbers are stamped
// later), null entries of a cell read one address (two with 32-byte vectors: one per lane parity) and count once.
constexpr int PK_IMPROVE_SWEEPS = 6;       // most of the gain comes in the first three (3.88 -> 3.34 / 3.23 / 3.16 ... 3.07 cycles)
constexpr long PK_IMPROVE_MAX_CODES = 8L << 20;  // packed_arrange = 1 (default): layers above this keep the greedy deal alone
constexpr int PK_IMPROVE_SWEEPS_LONG = 3;  // wave ranges of more than 12 steps: the 70B layers, bound by their entry stream anyway

struct PkHist {
  uint32_t w[4];  // 16 counts of 8 bits
  __device__ __forceinline__ void add(uint32_t bank, uint32_t delta) {  // delta = +1 or -1 (as uint32_t)
    const uint32_t v = delta << ((bank & 3u) * 8u);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) w[i] += (bank >> 2) == i ? v : 0u;
  }
  __device__ __forceinline__ uint32_t count(uint32_t bank) const {
    uint32_t v = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) v = (bank >> 2) == i ? w[i] : v;
    return (v >> ((bank & 3u) * 8u)) & 255u;
  }
  __device__ __forceinline__ int cost() const {
    int mx = 0, sq = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = (int)((w[i >> 2] >> ((i & 3) * 8)) & 255u);
      mx = c > mx ? c : mx;
      sq += c * c;
    }
    return 8 * mx + sq;
  }
};

__device__ __forceinline__ int pk_lane_group(int lane) {  // LDS service group of a lane (inverse of pk_group_lane)
  const int h = lane & 31;
  const int g1 = (h >= 4 && h < 12) || (h >= 16 && h < 20) || h >= 28;
  return (lane >> 5) * 2 + g1;
}

__global__ __launch_bounds__(64) void pk_improve_kernel(const uint32_t* a, uint32_t* ent, const PkGeom G, int in_groups, int NW,
                                                        int T) {
  extern __shared__ uint32_t arr_sm[];
  uint32_t* e = arr_sm;                                                       // [64 * T * 4] entries in (lane, t, k) order: a row's pool is contiguous
  PkHist* hc = reinterpret_cast<PkHist*>(e + (size_t)T * 256);               // [4 T slots][4 service groups]
  PkHist* hx = hc + (size_t)T * 16;
  uint16_t* rowa = reinterpret_cast<uint16_t*>(hx + (size_t)T * 16);         // [64 * T] the pool of the lane-step's row: lane-steps [rowa, rowb)
  uint16_t* rowb = rowa + (size_t)T * 64;
  uint8_t* nulls = reinterpret_cast<uint8_t*>(rowb + (size_t)T * 64);        // [4 T][4][2] null entries per cell and lane parity
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int sl_, row0_, nrows;
  pk_stream_rows(G, (int)st, sl_, row0_, nrows);
  const uint32_t* starts = a + st * (G.RG + 1);
  const uint32_t total = starts[nrows];
  uint32_t* wave_ent = ent + (((size_t)st * NW + w) * T) * 256;
  const uint32_t w0 = (uint32_t)w * 64u * (uint32_t)T;
  if (w0 >= total) return;  // nothing but null entries
  const uint32_t q0 = w0 + (uint32_t)l * (uint32_t)T;
  for (int t = 0; t < T; ++t)
    *reinterpret_cast<u32x4*>(e + ((size_t)l * T + t) * 4) = *reinterpret_cast<const u32x4*>(wave_ent + ((size_t)t * 64 + l) * 4);
  for (int i = l; i < T * 16 * 2 * 4; i += 64) reinterpret_cast<uint32_t*>(hc)[i] = 0u;  // hc and hx
  for (int i = l; i < T * 32; i += 64) nulls[i] = 0;
  {
    int r = nrows;
    if (q0 < total) {
      int lo = 0, hi = nrows;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= q0) lo = mid; else hi = mid;
      }
      r = lo;
    }
    for (int t = 0; t < T; ++t) {
      const uint32_t q = q0 + (uint32_t)t;
      uint32_t ra = q - w0, rb = ra + 1;
      if (q < total) {
        while (starts[r + 1] <= q) ++r;
        const uint32_t rs = starts[r], re = starts[r + 1];
        ra = rs > w0 ? rs - w0 : 0u;
        rb = re < w0 + 64u * (uint32_t)T ? re - w0 : 64u * (uint32_t)T;
      }
      rowa[l * T + t] = (uint16_t)ra;
      rowb[l * T + t] = (uint16_t)rb;
    }
  }
  __syncthreads();
  const uint32_t null_j = (uint32_t)in_groups;
  // bank groups of an entry read by a lane of parity `par`; null entries: the zero vector's slot and x slot `in_groups`
  auto bank_c = [&](uint32_t v, uint32_t par) { return (v >> (16 + PK_VSH)) == null_j ? par : (((v >> 4) & 15u) ^ par); };
  auto bank_x = [&](uint32_t v, uint32_t par) { return (((v >> (16 + PK_VSH)) << (PK_VSH - 4)) & 15u) ^ par; };
  auto lane_par = [](int lane) { return PK_G == 16 ? (uint32_t)(lane & 1) : 0u; };
  // the cell's histograms after `v` joined (sign = +1) or left (-1) at lane parity `par`; `nz` = the cell's null count there
  auto apply = [&](PkHist& c, PkHist& x, uint32_t v, uint32_t par, uint32_t sign, uint32_t& nz) {
    if ((v >> (16 + PK_VSH)) == null_j) {
      const bool counts = sign == 1u ? nz == 0u : nz == 1u;  // the first null in, the last null out
      nz += sign;
      if (!counts) return;
    }
    c.add(bank_c(v, par), sign);
    x.add(bank_x(v, par), sign);
  };
  if (l == 0) {  // histograms of the greedy deal (sequential: pack time, 256 T entries)
    for (int lane = 0; lane < 64; ++lane)
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < 4; ++k) {
          const int cell = (t * 4 + k) * 4 + pk_lane_group(lane);
          const uint32_t par = lane_par(lane);
          uint32_t nz = nulls[cell * 2 + par];
          apply(hc[cell], hx[cell], e[(lane * T + t) * 4 + k], par, 1u, nz);
          nulls[cell * 2 + par] = (uint8_t)nz;
        }
  }
  __syncthreads();
  const int sweeps = T <= 12 ? PK_IMPROVE_SWEEPS : PK_IMPROVE_SWEEPS_LONG;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    for (int s = 0; s < 4 * T; ++s) {
      const int t = s >> 2, k = s & 3;
      for (int lane = 0; lane < 64; ++lane) {  // wave-uniform: the entry under repair
        const int p = (lane * T + t) * 4 + k;
        const uint32_t v = e[p];
        if ((v >> (16 + PK_VSH)) == null_j) continue;
        const uint32_t par = lane_par(lane);
        const int cell = s * 4 + pk_lane_group(lane);
        const PkHist c0 = hc[cell], x0 = hx[cell];
        if (c0.count(bank_c(v, par)) <= 1u && x0.count(bank_x(v, par)) <= 1u) continue;  // alone in both bank groups
        const int cost0 = c0.cost() + x0.cost();
        const uint32_t nz0 = nulls[cell * 2 + par];
        const int base = (int)rowa[lane * T + t] * 4, n = ((int)rowb[lane * T + t] - (int)rowa[lane * T + t]) * 4;
        uint32_t key = ~0u;  // (cost change + 2^14) << 16 | pool index: the minimum is the best, lowest-index partner
        for (int i = l; i < n; i += 64) {
          const int p2 = base + i, q2 = p2 >> 2, k2 = p2 & 3, lane2 = q2 / T, t2 = q2 - lane2 * T;
          const int cell2 = (t2 * 4 + k2) * 4 + pk_lane_group(lane2);
          if (cell2 == cell) continue;
          const uint32_t v2 = e[p2], par2 = lane_par(lane2);
          PkHist c1 = c0, x1 = x0, c2 = hc[cell2], x2 = hx[cell2];
          const int cost2 = c2.cost() + x2.cost();
          uint32_t nz1 = nz0, nz2 = nulls[cell2 * 2 + par2];
          apply(c1, x1, v, par, ~0u, nz1);
          apply(c1, x1, v2, par, 1u, nz1);
          apply(c2, x2, v2, par2, ~0u, nz2);
          apply(c2, x2, v, par2, 1u, nz2);
          int cost_a = c1.cost() + x1.cost(), cost_b = c2.cost() + x2.cost();
          // hipcc 7.2 / gfx950 -O3 miscompiles the four-cost difference when it may fold it (every change came out positive: no
          // swap was ever taken; found with tools/microbench/arr_dbg.hip): keep the new costs as opaque values
          asm volatile("" : "+v"(cost_a), "+v"(cost_b));
          const int d = cost_a + cost_b - cost0 - cost2;
          const uint32_t kk = ((uint32_t)(d + (1 << 14)) << 16) | (uint32_t)i;
          key = kk < key ? kk : key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t other = (uint32_t)__shfl_xor((int)key, o, WAVE);
          key = other < key ? other : key;
        }
        if ((key >> 16) > (1u << 14)) continue;  // every partner makes it worse (or there is none)
        __syncthreads();  // everybody has read the cells
        if (l == 0) {
          const int p2 = base + (int)(key & 0xffffu), q2 = p2 >> 2, k2 = p2 & 3, lane2 = q2 / T, t2 = q2 - lane2 * T;
          const int cell2 = (t2 * 4 + k2) * 4 + pk_lane_group(lane2);
          const uint32_t v2 = e[p2], par2 = lane_par(lane2);
          PkHist c1 = hc[cell], x1 = hx[cell], c2 = hc[cell2], x2 = hx[cell2];
          uint32_t nz1 = nulls[cell * 2 + par], nz2 = nulls[cell2 * 2 + par2];
          apply(c1, x1, v, par, ~0u, nz1);
          apply(c1, x1, v2, par, 1u, nz1);
          apply(c2, x2, v2, par2, ~0u, nz2);
          apply(c2, x2, v, par2, 1u, nz2);
          hc[cell] = c1; hx[cell] = x1; hc[cell2] = c2; hx[cell2] = x2;
          nulls[cell * 2 + par] = (uint8_t)nz1;
          nulls[cell2 * 2 + par2] = (uint8_t)nz2;
          e[p] = v2;
          e[p2] = v;
        }
        __syncthreads();
      }
    }
  }
  for (int t = 0; t < T; ++t)
    *reinterpret_cast<u32x4*>(wave_ent + ((size_t)t * 64 + l) * 4) = *reinterpret_cast<const u32x4*>(e + ((size_t)l * T + t) * 4);
}

// K4: bookkeeping bits.  Thread (st, r): flag on the row's last lane-step.
__global__ __launch_bounds__(256) void pk_flag_kernel(const uint32_t* a, uint32_t* ent, const PkGeom G, int NW, int T) {
  const size_t st = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  int sl_, row0_, nrows;
  pk_stream_rows(G, (int)st, sl_, row0_, nrows);
  if (r >= nrows) return;
  const uint32_t ql = a[st * (G.RG + 1) + r + 1] - 1;
  atomicOr(&ent[pk_entry_index(ql, 0, st, NW, T)], 1u);
}

// K5: per lane column its starting row (in the spare bits of the column's first lane-step), per wave winfo.
__global__ __launch_bounds__(64) void pk_column_kernel(const uint32_t* a, uint32_t* ent, uint32_t* winfo, const PkGeom G,
                                                       int NW, int T) {
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int sl_, row0_, nrows;
  pk_stream_rows(G, (int)st, sl_, row0_, nrows);
  const uint32_t* starts = a + st * (G.RG + 1);  // starts[r], r < nrows; starts[nrows] == total (rows past the stream's have 0 steps)
  const uint32_t total = starts[nrows];
  const uint32_t w0 = (uint32_t)w * 64u * T;
  if (l == 0) {
    // wfr = first r in [0, nrows] with starts[r] >= w0  (informational: first row that starts in this wave range)
    int lo = 0, hi = nrows;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (starts[mid] >= w0) hi = mid; else lo = mid + 1;
    }
    uint32_t* wi = winfo + (st * NW + w) * 4;
    wi[0] = (uint32_t)lo;
    wi[1] = (w0 < total && starts[lo] > w0) ? 1u : 0u;
    wi[2] = w0 >= total ? 0u : (total - w0 >= (uint32_t)T ? (uint32_t)T : total - w0);
    wi[3] = 0u;
  }
  const uint32_t q = w0 + (uint32_t)l * T;
  int r0;
  if (q >= total) {
    r0 = nrows;
  } else {  // last r with starts[r] <= q
    int a0 = 0, b0 = nrows;  // invariant: starts[a0] <= q, answer in [a0, b0)
    while (b0 - a0 > 1) {
      const int mid = (a0 + b0) >> 1;
      if (starts[mid] <= q) a0 = mid; else b0 = mid;
    }
    r0 = a0;
  }
  const uint32_t f = (uint32_t)r0;
  uint32_t* e = ent + ((((size_t)st * NW + w) * T + 0) * 64 + l) * 4;
  e[0] |= (f & 7u) << 1;
  e[1] |= (f >> 3) & 15u;
  e[2] |= (f >> 7) & 15u;
  e[3] |= (f >> 11) & 15u;
}

// K6 (3-byte entries): the repack works on the 4-byte layout; this pass squeezes it.  A wave range becomes
// [T flag words of 8 B: bit l = lane l's lane-step t ends a row][T steps of 64 x 12 B]; an entry is slot << 12 | code
// (24 bits), four of them in three dwords.  The start row of a column is no longer stored: the kernel derives it from
// winfo[3] (start row of the wave range's first column) and the flag words.
__device__ __forceinline__ void pk_pack3(const u32x4& v, uint32_t& w0, uint32_t& w1, uint32_t& w2) {
  auto e24 = [](uint32_t x) { return ((x >> 20) << 12) | ((x >> 4) & 0xfffu); };
  const uint32_t e0 = e24(v.x), e1 = e24(v.y), e2 = e24(v.z), e3 = e24(v.w);
  w0 = e0 | (e1 << 24);
  w1 = (e1 >> 8) | (e2 << 16);
  w2 = (e2 >> 16) | (e3 << 8);
}
__device__ __forceinline__ void pk_unpack3(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t (&e)[4]) {
  e[0] = w0 & 0xffffffu;
  e[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
  e[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
  e[3] = w2 >> 8;
}

__global__ __launch_bounds__(64) void pk_compress_kernel(const uint32_t* ent4, uint8_t* ent3, uint32_t* winfo, const PkGeom G,
                                                         int NW, int T) {
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int sl_, row0_, nrows;
  pk_stream_rows(G, (int)st, sl_, row0_, nrows);
  const uint32_t* src = ent4 + (((size_t)st * NW + w) * T) * 256;
  uint8_t* dst = ent3 + ((size_t)st * NW + w) * T * PK_WREG3;
  uint32_t* wi = winfo + (st * NW + w) * 4;
  for (int t = 0; t < T; ++t) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + ((size_t)t * 64 + l) * 4);
    if (t == 0 && l == 0) wi[3] = wi[2] ? pk_get_start_row(v.x, v.y, v.z, v.w) : (uint32_t)nrows;
    uint32_t w0, w1, w2;
    pk_pack3(v, w0, w1, w2);
    uint32_t* o = reinterpret_cast<uint32_t*>(dst + (size_t)T * 8 + (size_t)t * PK_STEP3 + (size_t)l * 12);
    o[0] = w0; o[1] = w1; o[2] = w2;
    const unsigned long long fl = __ballot((v.x & 1u) != 0u);
    if (l == 0) *reinterpret_cast<unsigned long long*>(dst + (size_t)t * 8) = fl;
  }
}

__global__ __launch_bounds__(64) void pk_unpack3_kernel(const uint8_t* ent3, const uint32_t* winfo, const uint16_t* old_of_new,
                                                        uint16_t* codes, const PkGeom G, int in_groups, int NW, int T) {
  const int xstride = pk_x_stride(in_groups);
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int s, row0, nrows;
  pk_stream_rows(G, (int)st, s, row0, nrows);
  const uint32_t* wi = winfo + (st * NW + w) * 4;
  const int steps = (int)wi[2];
  const uint8_t* base = ent3 + ((size_t)st * NW + w) * T * PK_WREG3;
  // start row of this column: the wave range's start row + the row ends in the columns before it
  int row = (int)wi[3];
  for (int t = 0; t < steps; ++t) {
    const unsigned long long fl = *reinterpret_cast<const unsigned long long*>(base + (size_t)t * 8);
    row += __popcll(fl & ((1ull << l) - 1ull));
  }
  for (int t = 0; t < steps; ++t) {
    const uint32_t* p3 = reinterpret_cast<const uint32_t*>(base + (size_t)T * 8 + (size_t)t * PK_STEP3 + (size_t)l * 12);
    uint32_t e[4];
    pk_unpack3(p3[0], p3[1], p3[2], e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int slot = (int)(e[k] >> 12);
      const int j = slot % xstride;
      if (j < in_groups && row < nrows) {
        const uint32_t c = ((uint32_t)s << PK_CODE_BITS) | (e[k] & 0xfffu);
        codes[(size_t)(row0 + row) * in_groups + j] = old_of_new ? old_of_new[c] : (uint16_t)c;
      }
    }
    const unsigned long long fl = *reinterpret_cast<const unsigned long long*>(base + (size_t)t * 8);
    row += (int)((fl >> l) & 1ull);
  }
}

// inverse of the repack: canonical codes [M][in_groups] from a packed buffer (lossless; used to drop / restore the
// canonical codes of inference-only models and by the tests).  One wave per (stream, wave range).
__global__ __launch_bounds__(64) void pk_unpack_kernel(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ winfo,
                                                       const uint16_t* __restrict__ old_of_new, uint16_t* __restrict__ codes, const PkGeom G,
                                                       int in_groups, int NW, int T) {
  const int xstride = pk_x_stride(in_groups);
  const size_t st = blockIdx.x;
  const int w = blockIdx.y, l = threadIdx.x;
  int s, row0, nrows;
  pk_stream_rows(G, (int)st, s, row0, nrows);
  const uint32_t* wi = winfo + (st * NW + w) * 4;
  const int steps = (int)wi[2];
  const u32x4* col = reinterpret_cast<const u32x4*>(ent + (((size_t)st * NW + w) * T * 64 + l) * 4);
  int local = 0;
  // A column's lane-steps are independent loads; only the row counter is sequential.  UB of them are requested before the first is
  // decoded (round 6: the first cut loaded, decoded and stored one lane-step at a time -- with ~10 steps per column and 14 waves per
  // CU the kernel was a chain of HBM round trips: 32 us for the 10 MB of a 4096 x 4096 layer, bench.py detail.unpack_1x16_us).
  constexpr int UB = 8;
  for (int t0 = 0; t0 < steps; t0 += UB) {
    u32x4 ev[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int t = t0 + u < steps ? t0 + u : steps - 1;
      ev[u] = col[(size_t)t * 64];
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if (t0 + u >= steps) break;
      const uint32_t e[4] = {ev[u].x, ev[u].y, ev[u].z, ev[u].w};
      if (t0 + u == 0) local = (int)pk_get_start_row(e[0], e[1], e[2], e[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t v = e[k];
        const int j = (int)(v >> (16 + PK_VSH)) - (int)((v >> 16) & 3u) * xstride;
        if (j < in_groups && local < nrows) {
          const uint32_t c = ((uint32_t)s << PK_CODE_BITS) | ((v >> PK_VSH) & (uint32_t)(PK_SLICE_ENTRIES - 1));
          codes[(size_t)(row0 + local) * in_groups + j] = old_of_new ? old_of_new[c] : (uint16_t)c;
        }
      }
      local += (int)(e[0] & 1u);
    }
  }
}

// W[M][in_features] straight from a packed buffer: the unpack kernels' walk, writing codebook vectors instead of labels (no int16
// codes in between).  One wave per (stream, wave range); per round UB lane-steps of entries are requested before the first is
// decoded, then all their permutation look-ups (relabelled buffers) and row scales, then the codebook vectors DB lane-steps at a
// time -- every dependent level is one batch of independent loads, never a chain per entry.  Only the STORE is predicated (null /
// padding entries: j >= in_groups or a row past the stream's last), so the loads stay unconditional and in flight together; the
// indices they use are in range whatever the entry holds (labels < 65536, the scale of an invalid row is read from row 0).
// The arithmetic is dequant.hip's, operation for operation (0 + entry, times the scale or 1, one rounding): same bits.
// `by_xcd`: the 32 streams of consecutive blocks b, b + 8, ... (one XCD under the round-robin placement) are all slices of ONE
// row group, so the 16-/32-B pieces of a row's lines meet in one L2 (uniform geometry; any bijection is correct).
template <class T_, int EB, bool PERM>
__global__ __launch_bounds__(64) void pk_dequant_kernel(const uint8_t* __restrict__ ent, const uint32_t* __restrict__ winfo,
                                                        const uint16_t* __restrict__ old_of_new, const u32x4* __restrict__ codebook,
                                                        const uint16_t* __restrict__ scales, uint16_t* __restrict__ W, const PkGeom G,
                                                        int in_groups, int NW, int T, int by_xcd) {
  constexpr int P = PK_G / 8;   // 16-B pieces of a codebook vector
  constexpr int UB = 8;         // lane-steps per round
  constexpr int DB = 4 / P;     // lane-steps whose vectors are gathered together: 16 x 16 B or 8 x 32 B per lane
  static_assert(EB == 4 || (EB == 3 && PK_G == 8), "3-byte entries: 16-B vectors only");
  const int xstride = pk_x_stride(in_groups);
  const int l = threadIdx.x;
  const uint32_t b = blockIdx.x;
  int st, w;
  if (by_xcd) {
    const uint32_t x = b & 7u, q = b >> 3, i = q & (uint32_t)(PK_NST / 8 - 1);
    w = (int)(q / (uint32_t)(PK_NST / 8));
    st = (int)(((((i >> PK_S_LOG) * 8u) + x) << PK_S_LOG) | (i & (uint32_t)(PK_S - 1)));
  } else {
    st = (int)(b % (uint32_t)PK_NST);
    w = (int)(b / (uint32_t)PK_NST);
  }
  int s, row0, nrows;
  pk_stream_rows(G, st, s, row0, nrows);
  const uint32_t* wi = winfo + ((size_t)st * NW + w) * 4;
  const int steps = (int)wi[2];
  const uint8_t* base = ent + ((size_t)st * NW + w) * T * (EB == 3 ? (size_t)PK_WREG3 : (size_t)1024);
  int local = 0;
  if constexpr (EB == 3) {  // start row of this column: the wave range's start row + the row ends in the columns before it
    local = (int)wi[3];
    for (int t = 0; t < steps; ++t) {
      const unsigned long long fl = *reinterpret_cast<const unsigned long long*>(base + (size_t)t * 8);
      local += __popcll(fl & ((1ull << l) - 1ull));
    }
  }
  for (int t0 = 0; t0 < steps; t0 += UB) {
    uint32_t e[UB][4], rowend[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int t = t0 + u < steps ? t0 + u : steps - 1;
      if constexpr (EB == 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(base + ((size_t)t * 64 + l) * 16);
        e[u][0] = v.x; e[u][1] = v.y; e[u][2] = v.z; e[u][3] = v.w;
        rowend[u] = 0;
      } else {
        const uint32_t* p3 = reinterpret_cast<const uint32_t*>(base + (size_t)T * 8 + (size_t)t * PK_STEP3 + (size_t)l * 12);
        pk_unpack3(p3[0], p3[1], p3[2], e[u]);
        const unsigned long long fl = *reinterpret_cast<const unsigned long long*>(base + (size_t)t * 8);
        rowend[u] = (uint32_t)((fl >> l) & 1ull);
      }
    }
    // decode: input group and label of every entry, row of every lane-step (the only sequential part)
    int jj[UB][4], rowl[UB];
    uint32_t lab[UB][4];
    bool live[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if constexpr (EB == 4) {
        if (t0 + u == 0) local = (int)pk_get_start_row(e[u][0], e[u][1], e[u][2], e[u][3]);
        rowend[u] = e[u][0] & 1u;
      }
      live[u] = t0 + u < steps && local < nrows;
      rowl[u] = live[u] ? row0 + local : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t v = e[u][k];
        if constexpr (EB == 4) {
          jj[u][k] = (int)(v >> (16 + PK_VSH)) - (int)((v >> 16) & 3u) * xstride;
          lab[u][k] = ((uint32_t)s << PK_CODE_BITS) | ((v >> PK_VSH) & (uint32_t)(PK_SLICE_ENTRIES - 1));
        } else {
          jj[u][k] = (int)(v >> 12) % xstride;
          lab[u][k] = ((uint32_t)s << PK_CODE_BITS) | (v & 0xfffu);
        }
      }
      if (t0 + u < steps) local += (int)rowend[u];
    }
    if constexpr (PERM) {  // back to the checkpoint's labels: the caller's codebook is indexed by them
#pragma unroll
      for (int u = 0; u < UB; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) lab[u][k] = old_of_new[lab[u][k]];
    }
    float sc[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) sc[u] = scales ? T_::to_float(scales[rowl[u]]) : 1.f;
#pragma unroll
    for (int d0 = 0; d0 < UB; d0 += DB) {
      u32x4 vec[DB][4][P];
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int pp = 0; pp < P; ++pp) vec[d][k][pp] = codebook[(size_t)lab[d0 + d][k] * P + pp];
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const int u = d0 + d;
        const float scale = sc[u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!live[u] || jj[u][k] < 0 || jj[u][k] >= in_groups) continue;
          uint16_t* out = W + ((size_t)rowl[u] * in_groups + jj[u][k]) * PK_G;
#pragma unroll
          for (int pp = 0; pp < P; ++pp) {
            const u32x4 c = vec[d][k][pp];
            float f[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) f[q] = 0.f;
            f[0] += T_::lo(c.x); f[1] += T_::hi(c.x);
            f[2] += T_::lo(c.y); f[3] += T_::hi(c.y);
            f[4] += T_::lo(c.z); f[5] += T_::hi(c.z);
            f[6] += T_::lo(c.w); f[7] += T_::hi(c.w);
            u32x4 o;
            o.x = (uint32_t)T_::from_float(f[0] * scale) | ((uint32_t)T_::from_float(f[1] * scale) << 16);
            o.y = (uint32_t)T_::from_float(f[2] * scale) | ((uint32_t)T_::from_float(f[3] * scale) << 16);
            o.z = (uint32_t)T_::from_float(f[4] * scale) | ((uint32_t)T_::from_float(f[5] * scale) << 16);
            o.w = (uint32_t)T_::from_float(f[6] * scale) | ((uint32_t)T_::from_float(f[7] * scale) << 16);
            *reinterpret_cast<u32x4*>(out + pp * 8) = o;
          }
        }
      }
    }
  }
}

#include "packed_gemv_kernels.h"  // matvec: params, LDS maps, body, kernel wrappers, finalize kernels


// ---------------------------------------------------------------------------------------------- pipelined shared-input launch
// q/k/v (gate/up) of a decoder layer in ONE launch of 256 workgroups, each walking its (row group, slice) stream of every
// segment in turn with the codebook slices double-buffered: while the compute waves run the loop of segment k, two DMA
// waves pull the slice of segment k + 1 into the other buffer, so only the first fill of the launch is exposed (the
// plain multi kernel above starts a fresh workgroup per segment: fill and loop of a CU never overlap).  Batch 1, 4-byte
// entries, one x copy, single-kernel finalize; everything else takes the plain multi kernel.
//   LDS: x window | slice buffer 0 | slice buffer 1 | rowstart x 2 | rowval | colend | xmax.  The two slice buffers are
//   65536 bytes apart: an entry's codebook address is (word & 0xfff0) | (k & 1) << 16 -- one v_and_or_b32, as many
//   operations per entry as the single-layer kernel -- plus the constant offset of buffer 0 in the ds_read.
//   Waves: NWC compute waves (max over the segments' wave counts) + 2 DMA waves.  The compute waves' VMEM queue holds ring
//   fetches and the returning atomics only (hipcc counts those); the DMA waves hold LDS-DMA only (waited with vmcnt(0)).
//   Layers packed for 15 / 16 waves (SELF_DMA): no DMA waves; every compute wave requests its share of slice k + 1 when its
//   own steps of segment k are done, and the epilogue reads its row tables through asm (hipcc guards every LDS read it sees
//   with vmcnt(0) while LDS-DMA is in flight).
//   Barriers per segment: M_k (loop k done -> epilogue k may read rowval / colend) and F_k (epilogue k done AND slice
//   k + 1 landed).
//   Hand-shake: segment k's returning atomic is looked at in epilogue k + 1 (settle_pending), i.e. behind loop k + 1 -- its
//   round trip is off the critical path; the last segment settles at once.
constexpr uint32_t PP_XWIN = 16640;        // x window: (in_groups + 1) * vector bytes <= the window (inputs of <= 8192 features) ...
constexpr uint32_t PP_XWIN_SMALL = 8448;   // ... or <= 4096 features: 8 KiB more for the tables (template parameter XW of the kernel)
constexpr int PP_DMA_WAVES = 2;

// Bookkeeping behind the two slice buffers.  Two barriers per segment (M_k, F_k): row starts double-buffered, one set of row
// sums.  ONE barrier (ONEB): the compute waves go from epilogue k straight into loop k + 1, so row sums / column ends are
// double-buffered (loop k + 1 writes the other set) and the row starts triple-buffered (the DMA waves request segment
// k + 2's while epilogue k may still read segment k's).
struct PipeLds {
  uint32_t rs0, rs_bytes, rowval, rowval_bytes, colend, colend_bytes, xmax, total;  // row starts of buffer b at rs0 + b * rs_bytes, ...
};
__host__ __device__ static inline PipeLds pipe_lds(int max_rg, uint32_t xwin, bool oneb) {
  PipeLds l;
  l.rs_bytes = oneb ? (((uint32_t)(max_rg + 1) * 4u + 255u) & ~255u) : (((uint32_t)(max_rg + 1) * 4u + 1023u) & ~1023u);
  l.rs0 = xwin + 2u * PK_SLICE_BYTES;
  l.rowval = l.rs0 + (oneb ? 3u : 2u) * l.rs_bytes;
  l.rowval_bytes = ((uint32_t)(max_rg + 1) * 4u + 15u) & ~15u;
  l.colend = l.rowval + (oneb ? 2u : 1u) * l.rowval_bytes;
  l.colend_bytes = (uint32_t)PK_MAX_NW * 64u * 4u;
  l.xmax = l.colend + (oneb ? 2u : 1u) * l.colend_bytes;
  l.total = l.xmax + (uint32_t)PK_MAX_NW * 4u;
  return l;
}

struct PipeParams {
  const uint16_t* x;
  int in_groups, nseg, max_rg, nwc;  // nwc: compute waves of the workgroup
  int dma_waves;                     // PP_DMA_WAVES, or 0: every compute wave requests its share of the next slice itself
  int defer;                         // DMA-wave mode: look at a segment's atomics one segment later (packed_pipe == 4 switches it off)
  PackedSegment seg[AQLM_HIP_MAX_SEGMENTS];
};

__device__ __forceinline__ uint32_t and_or(uint32_t w, uint32_t mask_vgpr, uint32_t base) {
  uint32_t d;  // one scalar operand per VOP3 instruction (constant bus): the mask travels in a VGPR
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(w), "v"(mask_vgpr), "s"(base));
  return d;
}

template <class T_, bool SELF_DMA, uint32_t XW, bool ONEB>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_pipe_kernel(const PipeParams mp) {
  static_assert(!(SELF_DMA && ONEB), "the single-barrier form needs the DMA waves");
  constexpr uint32_t PP_BUF0 = XW;
#ifndef AQLM_PP_PD
#define AQLM_PP_PD 3
#endif
  constexpr int PD = AQLM_PP_PD;  // entry steps in flight per wave (and requested ahead for the next segment)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_raw != 0u) __builtin_trap();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NWC = mp.nwc;
  // Layers packed for 15 or 16 waves leave no room for DMA waves: then every compute wave requests its share of segment
  // k + 1's slice when its own steps of segment k are done -- the requests land under the epilogue (barrier, row sums,
  // atomic round trip).  Not earlier: loads return in order, so a request in front of ring fetches would stall the loop
  // for the slice's latency, and hipcc guards VGPR loads with vmcnt(0) while LDS-DMA is in flight.
  constexpr bool self_dma = SELF_DMA;  // == (mp.dma_waves == 0)
  const bool dma_wave = wave >= NWC;
  const int dw = wave - NWC;  // 0 / 1 for the DMA waves
  const int block = (int)blockIdx.x;
  const int slice = block & (PK_S - 1), group = block >> PK_S_LOG;
  const PipeLds L = pipe_lds(mp.max_rg, XW, ONEB);
  const int NTC = NWC << 6;  // compute threads

  // scalar select of a segment's parameters (no dynamic indexing of the kernel-argument struct)
  auto segment = [&](int k) -> PackedSegment {
    PackedSegment s = mp.seg[0];
#pragma unroll
    for (int q = 1; q < AQLM_HIP_MAX_SEGMENTS; ++q)
      if (k == q) s = mp.seg[q];
    return s;
  };
  auto dma_slice = [&](const PackedSegment& s, int buf, int first, int stride) {  // pieces first, first + stride, ... of the slice
    const uint8_t* src = s.codebook + (size_t)slice * PK_SLICE_BYTES;
    constexpr int PIECES = (int)(PK_SLICE_BYTES / 1024);
    const int rot = group * (PIECES / PK_NG);
    for (int i0 = first; i0 < PIECES; i0 += stride) {
      const int i = (i0 + rot) & (PIECES - 1);
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)(src + i * 1024 + lane * 16),
                                       (lds_void_ptr)(size_t)(PP_BUF0 + (uint32_t)buf * PK_SLICE_BYTES + (uint32_t)i * 1024u), 16, 0, 0);
    }
  };
  auto rs_buf = [](int k) -> int { return ONEB ? k % 3 : (k & 1); };  // row-start buffer of segment k
  auto dma_rowstart = [&](const PackedSegment& s, int buf, int first, int stride) {
    const int RG1 = s.RG + 1;
    const uint32_t* rs_src = s.rowstart + (size_t)block * RG1;
    for (int i = first; i * 64 < RG1; i += stride) {
      const int idx = i * 64 + lane;
      if (idx < RG1)
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(rs_src + idx), (lds_void_ptr)(size_t)(L.rs0 + (uint32_t)buf * L.rs_bytes + (uint32_t)i * 256u), 4, 0, 0);  // buf: rs_buf(segment)
    }
  };

  // ---- prologue: every wave helps with the first fill (slice 0, x, row starts 0), as in the single-layer kernel ---------
  PackedSegment s0 = segment(0);
  const int NWB = NWC + mp.dma_waves;
  dma_slice(s0, 0, wave, NWB);
  {
    const int x16 = mp.in_groups * (int)(PK_VB / 16);  // 16-byte units of x
    const int nchunk = (x16 + 63) >> 6;
    for (int c = wave; c < nchunk; c += NWB) {
      const int idx = c * 64 + lane;
      if (idx < x16)
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(mp.x + (size_t)idx * 8), (lds_void_ptr)(size_t)((uint32_t)c * 1024u), 16, 0, 0);
    }
  }
  dma_rowstart(s0, rs_buf(0), wave, NWB);
  if (tid < (int)(PK_VB / 16))  // the null entries' x
    *reinterpret_cast<u32x4*>(smem_raw + (uint32_t)mp.in_groups * PK_VB + (uint32_t)tid * 16u) = u32x4{0u, 0u, 0u, 0u};
  if (tid < PK_MAX_NW) *reinterpret_cast<uint32_t*>(smem_raw + L.xmax + (uint32_t)tid * 4u) = 0u;

  uint32_t mask = PK_HMASK;
  asm volatile("" : "+v"(mask));  // SDWA operand in a VGPR

  // Epilogue of segment k by the threads t0, t0 + nt, ... (single-barrier form): row sums -> fixed-point cells -> the last
  // arrival writes y.  Two phases -- the atomics of up to four rows of a thread go out before the first answer is looked at --
  // and asm LDS reads (the DMA waves run it with LDS-DMA in flight; see lds_asm_load_b32).
  auto epilogue_rows = [&](int k, int t0, int nt) {
    const PackedSegment s = segment(k);
    int nrows = s.M - group * s.RG;
    nrows = nrows < 0 ? 0 : (nrows < s.RG ? nrows : s.RG);
    const uint32_t T = (uint32_t)s.T;
    const int row_begin = group * s.RG;
    const uint32_t rs_off = L.rs0 + (uint32_t)rs_buf(k) * L.rs_bytes;
    const uint32_t rowval_k = L.rowval + (ONEB ? (uint32_t)(k & 1) * L.rowval_bytes : 0u);
    const uint32_t colend_k = L.colend + (ONEB ? (uint32_t)(k & 1) * L.colend_bytes : 0u);
    if (t0 >= nrows) return;
    uint32_t xm = 0u;
    {
      u32x4 sl0 = lds_asm_load_b128(L.xmax), sl1 = lds_asm_load_b128(L.xmax + 16u), sl2 = lds_asm_load_b128(L.xmax + 32u),
            sl3 = lds_asm_load_b128(L.xmax + 48u);
      uint32_t dummy0 = 0u, dummy1 = 0u, dummy2 = 0u;
      lds_asm_wait(dummy0, dummy1, dummy2, sl0, sl1, sl2, sl3);
      const u32x4 sl[4] = {sl0, sl1, sl2, sl3};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t a = sl[q].x > sl[q].y ? sl[q].x : sl[q].y, c = sl[q].z > sl[q].w ? sl[q].z : sl[q].w;
        const uint32_t d = a > c ? a : c;
        xm = d > xm ? d : xm;
      }
    }
    const float bound = (float)mp.in_groups * (float)PK_G * s.cb_absmax * T_::to_float((uint16_t)xm);
    int e = 0;
    (void)frexpf(bound, &e);
    const int sh = PK_FIX_BITS - e;
    const uint16_t* bias_src = s.bias ? s.bias : s.scales;
    for (int r0 = t0; r0 < nrows; r0 += 4 * nt) {
      unsigned long long old[4], mine[4];
      uint16_t sc[4], bi[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = r0 + i * nt;
        old[i] = mine[i] = 0ull;
        sc[i] = bi[i] = 0;
        if (r < nrows) {
          uint32_t q0 = lds_asm_load_b32(rs_off + (uint32_t)r * 4u), q1 = lds_asm_load_b32(rs_off + (uint32_t)r * 4u + 4u);
          uint32_t vbits = lds_asm_load_b32(rowval_k + (uint32_t)r * 4u);
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q0), "+v"(q1), "+v"(vbits));
          float v = __uint_as_float(vbits);
          const uint32_t c0 = q0 / T;
          uint32_t c1 = (q1 - 1u) / T;
          c1 = c1 < (uint32_t)(PK_MAX_NW * 64) ? c1 : (uint32_t)(PK_MAX_NW * 64 - 1);
          for (uint32_t c = c0; c < c1; ++c) {
            uint32_t ce = lds_asm_load_b32(colend_k + c * 4u);
            lds_asm_wait(ce);
            v += __uint_as_float(ce);
          }
          const bool finite = bound < __builtin_inff() && fabsf(v) <= 2.f * bound;
          const long long qv = finite ? __float2ll_rn(ldexpf(v, sh)) : 0ll;
          mine[i] = ((unsigned long long)qv << PK_VAL_SHIFT) + (finite ? 1ull : 1ull + (1ull << PK_CNT_BITS));
          const int row = row_begin + r;
          old[i] = __hip_atomic_fetch_add(s.acc + row, mine[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          sc[i] = s.scales[row];
          bi[i] = bias_src[row];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = r0 + i * nt;
        if (r < nrows && (old[i] & PK_CNT_MASK) == (unsigned long long)(PK_S - 1)) {
          const int row = row_begin + r;
          const unsigned long long cell = old[i] + mine[i];
          const long long sum = (long long)cell >> PK_VAL_SHIFT;
          float sv = (float)ldexp((double)sum, -sh);
          if ((cell >> PK_CNT_BITS) & PK_CNT_MASK) sv = __builtin_nanf("");
          s.y[row] = T_::from_float(__builtin_fmaf(sv, T_::to_float(sc[i]), s.bias ? T_::to_float(bi[i]) : 0.f));
          __hip_atomic_store(s.acc + row, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  };

  // Single-barrier form: who runs segment k's epilogue?  The two DMA waves, during loop k + 1, when that costs the compute
  // waves nothing -- at most two rows per DMA thread and a next loop at least as long as this one (measured: with the short
  // k / v loops behind q, or 688-row groups, the DMA waves become the critical path); else the compute waves, right after M_k.
  auto epi_on_dma = [&](int k) -> bool {
    if (!ONEB || k + 1 >= mp.nseg) return false;
    const PackedSegment a = segment(k), b = segment(k + 1);
    int nrows = a.M - group * a.RG;
    nrows = nrows < 0 ? 0 : (nrows < a.RG ? nrows : a.RG);
    return nrows <= 2 * PP_DMA_WAVES * 64 && b.NW * b.T >= a.NW * a.T;
  };

  if (dma_wave) {
    // ============================================ DMA waves ================================================================
    __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (0 << 8));  // vmcnt(0) lgkmcnt(0): my share of the first fill has landed
    __builtin_amdgcn_s_barrier();                          // B0
    for (int k = 0; k < mp.nseg; ++k) {
      if (k + 1 < mp.nseg) {
        const PackedSegment sn = segment(k + 1);
        dma_slice(sn, (k + 1) & 1, dw, PP_DMA_WAVES);
        dma_rowstart(sn, rs_buf(k + 1), dw, PP_DMA_WAVES);
      }
      if constexpr (ONEB) {
        if (k >= 1 && epi_on_dma(k - 1)) epilogue_rows(k - 1, dw * 64 + lane, PP_DMA_WAVES * 64);  // while the compute waves run loop k
        __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (0 << 8));  // slice k + 1 is in LDS when the compute waves leave M_k
        __builtin_amdgcn_s_barrier();                        // M_k
      } else {
        __builtin_amdgcn_s_barrier();                        // M_k
        __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (0 << 8));
        __builtin_amdgcn_s_barrier();                        // F_k: slice k + 1 is in LDS
      }
    }
    return;
  }

  // ============================================== compute waves =============================================================
  __amdgpu_buffer_rsrc_t rs_ent = __builtin_amdgcn_make_buffer_rsrc((void*)s0.ent, 0, s0.ent_bytes, 0x00020000);
  auto fetch_from = [&](const __amdgpu_buffer_rsrc_t& rs, uint32_t wbase, int Tm1, int t) -> u32x4 {
    const uint32_t vo = t <= Tm1 ? (uint32_t)lane * 16u : 0xfffffff0u;  // past the range: zeros, no memory traffic
    return __builtin_amdgcn_raw_buffer_load_b128(rs, vo, wbase + (uint32_t)t * 1024u, AUX_NT);
  };
  u32x4 ring[PD];
  {
    const int wv = wave < s0.NW ? wave : s0.NW - 1;
    const uint32_t wbase = (uint32_t)(((size_t)block * s0.NW + wv) * s0.T) * 1024u;
#pragma unroll
    for (int j = 0; j < PD; ++j) ring[j] = fetch_from(rs_ent, wbase, wave < s0.NW ? s0.T - 1 : -1, j);
  }
  __builtin_amdgcn_s_waitcnt((PD & 15) | (7 << 4) | (0 << 8) | ((PD >> 4) << 14));  // vmcnt(PD): the fill, not the ring
  __builtin_amdgcn_s_barrier();                            // B0
  // the first ring steps: waited for here, by the builtin, so that the segment loop is ENTERED with nothing pending -- hipcc's
  // wait-count pass merges the entry state with the back edge's (a deferred atomic in flight) and would otherwise guard the
  // first use of the ring with vmcnt(0) on every segment (it emitted this wait itself before; now it knows)
  __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));

  // A row's hand-shake (returning atomic) is looked at one segment LATER, behind the next segment's loop, so its round trip
  // to the memory side is off the critical path (the compute waves wait for nothing else between segments; in the
  // self-service mode the wait for the LDS-DMA is counted so that it leaves the atomic in flight).  Only when every thread
  // has at most one row per segment.
  const bool tuning_defer = mp.defer != 0;
  bool defer_k = false;
  bool pend = false;
  unsigned long long pend_old = 0ull, pend_mine = 0ull;
  unsigned long long* pend_cell = nullptr;
  uint16_t* pend_y = nullptr;
  uint16_t pend_scale = 0, pend_bias = 0;
  int pend_sh = 0;
  bool pend_has_bias = false;
  auto settle_pending = [&]() {
    if (pend && (pend_old & PK_CNT_MASK) == (unsigned long long)(PK_S - 1)) {
      const unsigned long long cell = pend_old + pend_mine;
      const long long sum = (long long)cell >> PK_VAL_SHIFT;
      float sv = (float)ldexp((double)sum, -pend_sh);
      if ((cell >> PK_CNT_BITS) & PK_CNT_MASK) sv = __builtin_nanf("");
      *pend_y = T_::from_float(__builtin_fmaf(sv, T_::to_float(pend_scale), pend_has_bias ? T_::to_float(pend_bias) : 0.f));
      __hip_atomic_store(pend_cell, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    pend = false;
  };
  for (int k = 0; k < mp.nseg; ++k) {
    const PackedSegment s = segment(k);
    const int RG1 = s.RG + 1;
    int nrows = s.M - group * s.RG;
    nrows = nrows < 0 ? 0 : (nrows < s.RG ? nrows : s.RG);
    const int steps = wave < s.NW ? s.T : 0;
    const uint32_t bufsel = (uint32_t)(k & 1) << 16;
    const uint32_t rowval_k = L.rowval + (ONEB ? (uint32_t)(k & 1) * L.rowval_bytes : 0u);  // this segment's row sums / column ends
    const uint32_t colend_k = L.colend + (ONEB ? (uint32_t)(k & 1) * L.colend_bytes : 0u);
    const uint32_t wbase = (uint32_t)(((size_t)block * s.NW + (wave < s.NW ? wave : s.NW - 1)) * s.T) * 1024u;
    const int Tm1 = steps > 0 ? s.T - 1 : -1;
    // the first steps of the NEXT segment's entry stream are requested now: by the time the epilogue below waits for its
    // atomics they have long landed (VMEM returns in order), and loop k + 1 starts on data that is already here
    u32x4 ring_next[PD];
    __amdgpu_buffer_rsrc_t rs_next = rs_ent;
    if (k + 1 < mp.nseg) {
      const PackedSegment sn = segment(k + 1);
      rs_next = __builtin_amdgcn_make_buffer_rsrc((void*)sn.ent, 0, sn.ent_bytes, 0x00020000);
      const int wv = wave < sn.NW ? wave : sn.NW - 1;
      const uint32_t wb = (uint32_t)(((size_t)block * sn.NW + wv) * sn.T) * 1024u;
#pragma unroll
      for (int j = 0; j < PD; ++j) ring_next[j] = fetch_from(rs_next, wb, wave < sn.NW ? sn.T - 1 : -1, j);
    } else {
#pragma unroll
      for (int j = 0; j < PD; ++j) ring_next[j] = u32x4{0u, 0u, 0u, 0u};
    }
    float acc = 0.f;
    uint32_t row_addr = 0;
    auto step = [&](const u32x4& e) {
      const uint32_t w[4] = {e.x, e.y, e.z, e.w};
      uint32_t a_cb[4], a_x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a_cb[j] = and_or(w[j], mask, bufsel);
        a_x[j] = half_and<1>(w[j], mask);
      }
      constexpr int NV = (int)(PK_VB / 16);  // 16-byte reads per vector (2: second half at offset ^ 16, see PK_PARITY_BITS)
      u32x4 ev[4][NV], xv[4][NV];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < NV; ++h) {
          ev[j][h] = *(lds_u32x4_ptr)(size_t)((a_cb[j] ^ ((uint32_t)h * 16u)) + PP_BUF0);
          xv[j][h] = *(lds_u32x4_ptr)(size_t)(a_x[j] ^ ((uint32_t)h * 16u));
        }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < NV; ++h) acc = dot8<T_>(ev[j][h], xv[j][h], acc);
      if (e.x & 1u) {  // a row ends here: unique writer
        lds_store_f32(row_addr, acc);
        acc = 0.f;
        row_addr += 4u;
      }
    };
    if (steps > 0) {
      row_addr = rowval_k + pk_get_start_row(ring[0].x, ring[0].y, ring[0].z, ring[0].w) * 4u;
      int t = 0;
      for (; t + PD <= steps; t += PD) {
#pragma unroll
        for (int j = 0; j < PD; ++j) {
          step(ring[j]);
          ring[j] = fetch_from(rs_ent, wbase, Tm1, t + PD + j);
        }
      }
      const int rem = steps - t;
#pragma unroll
      for (int j = 0; j < PD - 1; ++j)
        if (j < rem) step(ring[j]);
    }
    if (k == 0) {  // largest |x| (every segment multiplies the same x): per-wave maxima, once
      typedef unsigned short us2 __attribute__((ext_vector_type(2)));
      us2 m = {0, 0};
      for (int idx = tid; idx < mp.in_groups * (int)(PK_VB / 16); idx += NTC) {
        const u32x4 v = *(lds_u32x4_ptr)(size_t)((uint32_t)idx * 16u);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) m = __builtin_elementwise_max(m, __builtin_bit_cast(us2, w4[j] & 0x7fff7fffu));
      }
      const uint32_t mm = wave_max_u32(m.x > m.y ? (uint32_t)m.x : (uint32_t)m.y);
      if (lane == 0) *reinterpret_cast<uint32_t*>(smem_raw + L.xmax + (uint32_t)wave * 4u) = mm;
    }
    if (wave < s.NW) lds_store_f32(colend_k + (uint32_t)(wave * 64 + lane) * 4u, acc);
    // every entry fetch of this wave has landed (the next segment's first steps were requested a loop ago): said with the
    // builtin on EVERY path, so that hipcc's wait-count pass knows no VGPR load is pending when the epilogue reuses the
    // ring's registers -- otherwise it guards that reuse with vmcnt(0), i.e. waits for the LDS-DMA issued just below
    __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));  // (both modes: the deferred atomic of the DMA-wave mode must be the only thing pending at the loop's back edge)
    if (self_dma && k + 1 < mp.nseg) {  // this wave's share of the next slice and row-start table (buffer (k + 1) & 1 is free: its
      const PackedSegment sn = segment(k + 1);  // last readers passed F_{k-1})
      dma_slice(sn, (k + 1) & 1, wave, NWC);
      dma_rowstart(sn, rs_buf(k + 1), wave, NWC);
    }
    rs_ent = rs_next;
#pragma unroll
    for (int j = 0; j < PD; ++j) ring[j] = ring_next[j];
    asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");  // the asm LDS stores are invisible to the compiler's counters
    __builtin_amdgcn_s_barrier();                          // M_k
    // ---- epilogue of segment k (compute waves): row sums -> fixed-point cell -> last arrival writes y ---------------------
    // (single-barrier form: where epi_on_dma(k) says so the DMA waves do it while this wave is already in loop k + 1)
    if (!epi_on_dma(k)) {
      const uint32_t rs_off = L.rs0 + (uint32_t)rs_buf(k) * L.rs_bytes;
      const uint32_t T = (uint32_t)s.T;
      const int row_begin = group * s.RG;
      settle_pending();  // segment k - 1's rows: their atomics went out one loop ago
      const bool defer = nrows <= NTC && k + 1 < mp.nseg && tuning_defer;
      defer_k = defer;
      for (int r = tid; r < nrows; r += NTC) {
        uint32_t q0, q1;
        float v;
        u32x4 sl[4];
        if constexpr (SELF_DMA) {  // asm reads: segment k + 1's slice is on its way into the other buffer (lds_asm_load_b32)
          q0 = lds_asm_load_b32(rs_off + (uint32_t)r * 4u);
          q1 = lds_asm_load_b32(rs_off + (uint32_t)r * 4u + 4u);
          uint32_t vbits = lds_asm_load_b32(rowval_k + (uint32_t)r * 4u);
#pragma unroll
          for (int q = 0; q < 4; ++q) sl[q] = lds_asm_load_b128(L.xmax + (uint32_t)(q * 4) * 4u);
          lds_asm_wait(q0, q1, vbits, sl[0], sl[1], sl[2], sl[3]);
          v = __uint_as_float(vbits);
          const uint32_t c0 = q0 / T;
          uint32_t c1 = (q1 - 1u) / T;
          c1 = c1 < (uint32_t)(PK_MAX_NW * 64) ? c1 : (uint32_t)(PK_MAX_NW * 64 - 1);  // a column index, whatever was read
          for (uint32_t c = c0; c < c1; ++c) {
            uint32_t ce = lds_asm_load_b32(colend_k + c * 4u);
            lds_asm_wait(ce);
            v += __uint_as_float(ce);
          }
        } else {
          const uint32_t* rs = reinterpret_cast<const uint32_t*>(smem_raw + rs_off);
          const float* rowval = reinterpret_cast<const float*>(smem_raw + rowval_k);
          const float* colend = reinterpret_cast<const float*>(smem_raw + colend_k);
          q0 = rs[r];
          q1 = rs[r + 1];
          const uint32_t c0 = q0 / T, c1 = (q1 - 1u) / T;
          v = rowval[r];
          for (uint32_t c = c0; c < c1; ++c) v += colend[c];
#pragma unroll
          for (int q = 0; q < 4; ++q) sl[q] = *(lds_u32x4_ptr)(size_t)(L.xmax + (uint32_t)(q * 4) * 4u);
        }
        uint32_t xm = 0u;
        {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t a = sl[q].x > sl[q].y ? sl[q].x : sl[q].y, c = sl[q].z > sl[q].w ? sl[q].z : sl[q].w;
            const uint32_t d = a > c ? a : c;
            xm = d > xm ? d : xm;
          }
        }
        const float bound = (float)mp.in_groups * (float)PK_G * s.cb_absmax * T_::to_float((uint16_t)xm);
        int e = 0;
        (void)frexpf(bound, &e);
        const bool finite = bound < __builtin_inff() && fabsf(v) <= 2.f * bound;
        const int sh = PK_FIX_BITS - e;
        const long long qv = finite ? __float2ll_rn(ldexpf(v, sh)) : 0ll;
        const unsigned long long mine = ((unsigned long long)qv << PK_VAL_SHIFT) + (finite ? 1ull : 1ull + (1ull << PK_CNT_BITS));
        const int row = row_begin + r;
        // the hand-shake goes out; it is looked at right away, or (defer, uniform) behind the next segment's loop.  The atomic
        // returns straight into the carried variable: a copy of its result would make hipcc wait for it here.
        pend_mine = mine;
        pend_sh = sh;
        pend_cell = s.acc + row;
        pend_y = s.y + row;
        pend_has_bias = s.bias != nullptr;
        pend_old = __hip_atomic_fetch_add(pend_cell, pend_mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend_scale = s.scales[row];
        pend_bias = (s.bias ? s.bias : s.scales)[row];
        pend = true;
        if (!defer) settle_pending();
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
    if (self_dma) {  // my share of slice k + 1 has landed.  With a deferred hand-shake the wave's atomic and its scale / bias loads
      // are YOUNGER than the LDS-DMA (loads return in order): "at most 3 outstanding" then means the DMA is in, and the atomic
      // may stay in flight through the next loop.  A wave without rows issued none of the three and has to wait for everything.
      if (defer_k && (wave << 6) < nrows) __builtin_amdgcn_s_waitcnt(3 | (7 << 4) | (15 << 8));
      else __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));
    }
    if constexpr (!ONEB) __builtin_amdgcn_s_barrier();    // F_k (single-barrier form: the other table set is written next)
  }
  settle_pending();
}

static bool pipe_eligible(const PackedLayout* Ls, int n, int in_groups, int& max_rg, int& nwc, int& dma_waves, uint32_t& xwin, bool& oneb) {
  max_rg = 0;
  nwc = 0;
  for (int k = 0; k < n; ++k) {
    if (Ls[k].EB != 4 || Ls[k].XC != 1) return false;
    max_rg = std::max(max_rg, Ls[k].RG);
    nwc = std::max(nwc, Ls[k].NW);
  }
  if (PK_SLICE_BYTES != 65536u || PK_NST != 256 || n < 2 || nwc > PK_MAX_NW || (uint32_t)(in_groups + 1) * PK_VB > PP_XWIN) return false;
  dma_waves = nwc + PP_DMA_WAVES <= PK_MAX_NW ? PP_DMA_WAVES : 0;
  if (tuning().packed_pipe == 2) dma_waves = 0;  // experiments: self-service DMA for every shape
  if (tuning().packed_pipe == 3 && dma_waves == 0) return false;  // experiments: round-3 first cut (DMA waves only)
  xwin = (uint32_t)(in_groups + 1) * PK_VB <= PP_XWIN_SMALL ? PP_XWIN_SMALL : PP_XWIN;
  oneb = dma_waves != 0 && tuning().packed_pipe != 5 && pipe_lds(max_rg, xwin, true).total <= 160u * 1024u;  // 5: two barriers always
  return pipe_lds(max_rg, xwin, oneb).total <= 160u * 1024u;
}

#include "packed_launch.h"  // host launch helpers: kernel dispatch, LDS budget

}  // namespace PK_NS
}  // namespace aqlm

using namespace aqlm;
using namespace aqlm::PK_NS;

// ---- planning steps of the repack (host, pure functions) -----------------------------------------------------------------
// Relabelling: deal the 65536 entries to the PK_S slices, heaviest first, each to the lightest slice that still has room
// (longest-processing-time greedy with PK_SLICE_ENTRIES entries per slice): the slices end up with equal code counts unless a
// single entry outweighs a slice's share.  Deterministic (ties: lower label, lower slice).  Within a slice the heaviest entries
// take consecutive slots, i.e. distinct LDS bank groups.  Returns 0 (and leaves new_of_old alone) when the checkpoint's labels
// already load the slices evenly: no permutation, no codebook image, the buffer of format v6.
// `force`: deal even when the slices' TOTAL masses are already even -- label use correlated with the ROW (rows of one block of the
// layer drawing their codes from one slice's labels) leaves every global histogram flat and one stream per row group 14 x the
// mean; the repack asks for it whenever the 16 x 16 layout is not balanced and keeps the result only if the
// longest stream got shorter.  Equal counts fall out round-robin over the slices (stable order, lightest slice first).
static int plan_relabel(const uint32_t* usage, uint16_t* new_of_old, bool force = false) {
  unsigned long long mass0[PK_S] = {}, total = 0;
  for (int c = 0; c < 65536; ++c) mass0[c >> PK_CODE_BITS] += usage[c];
  unsigned long long mx = 0;
  for (int s = 0; s < PK_S; ++s) {
    total += mass0[s];
    mx = std::max(mx, mass0[s]);
  }
  if (total == 0 || (!force && (double)mx * PK_S <= 1.02 * (double)total)) return 0;
  std::vector<uint32_t> order(65536);
  for (uint32_t c = 0; c < 65536; ++c) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return usage[x] > usage[y]; });
  unsigned long long mass[PK_S] = {};
  int cnt[PK_S] = {};
  for (uint32_t i = 0; i < 65536; ++i) {
    const uint32_t c = order[i];
    int best = -1;
    for (int s = 0; s < PK_S; ++s)
      if (cnt[s] < PK_SLICE_ENTRIES && (best < 0 || mass[s] < mass[best])) best = s;
    new_of_old[c] = (uint16_t)(best * PK_SLICE_ENTRIES + cnt[best]);
    ++cnt[best];
    mass[best] += usage[c];
  }
  return 1;
}

// Geometry: deal the PK_NST workgroups to the slices in proportion to their work (lane-steps + a quarter step per row for the
// epilogue's hand-in): start from PK_MIN_GROUPS each, give the next workgroup to the slice whose groups are the longest.
// Uniform unless that shortens the longest stream by more than 6 % (the variable-geometry kernel pays ~0.1 us of scalar
// arithmetic in its prologue and serves single-layer launches only).  Returns 1 when groups[] is not uniform.
static int plan_geometry(const unsigned long long* slice_steps, int M, int in_features, uint8_t* groups) {
  for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)PK_NG;
  if (PK_G != 8 || M < PK_VG_MIN_ROWS || !packed_shape_ok(M, in_features, PK_G)) return 0;
  const int in_groups = in_features / PK_G;
  double w[PK_S], uni = 0.;
  for (int s = 0; s < PK_S; ++s) {
    w[s] = (double)slice_steps[s] + 0.25 * M;
    uni = std::max(uni, w[s] / PK_NG);
  }
  const int mb_uniform = packed_max_batch(in_groups, (M + PK_NG - 1) / PK_NG);
  for (int nmin = PK_MIN_GROUPS; nmin < PK_NG; ++nmin) {
    int n[PK_S], left = PK_NST - nmin * PK_S, mn = PK_NG;
    for (int s = 0; s < PK_S; ++s) n[s] = nmin;
    while (left-- > 0) {
      int best = 0;
      for (int s = 1; s < PK_S; ++s)
        if (w[s] / n[s] > w[best] / n[best]) best = s;
      ++n[best];
    }
    double var = 0.;
    bool uniform = true;
    for (int s = 0; s < PK_S; ++s) {
      var = std::max(var, w[s] / n[s]);
      mn = std::min(mn, n[s]);
      uniform = uniform && n[s] == PK_NG;
      if (n[s] > 255) return 0;
    }
    if (uniform || var > 0.94 * uni) return 0;
    // the bigger row groups of the lightest slices must not cost the layer its multi-row launches (up to 4 rows in one launch; 5
    // and 6 rows may take two): else start from more groups per slice
    if (packed_max_batch(in_groups, (M + mn - 1) / mn) < std::min(mb_uniform, 4)) continue;
    for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)n[s];
    return 1;
  }
  return 0;
}

extern "C" PK_API int PK_ENTRY(packed_plan_relabel)(const uint32_t* usage, int slices_log2, uint16_t* new_of_old) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_relabel, usage, slices_log2, new_of_old);
  if (!usage || !new_of_old || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_relabel: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  return plan_relabel(usage, new_of_old);
}

extern "C" PK_API int PK_ENTRY(packed_plan_relabel_ex)(const uint32_t* usage, int slices_log2, int force, uint16_t* new_of_old) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_relabel_ex, usage, slices_log2, force, new_of_old);
  if (!usage || !new_of_old || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_relabel_ex: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  return plan_relabel(usage, new_of_old, force != 0);
}

extern "C" PK_API int PK_ENTRY(packed_plan_geometry)(const uint64_t* slice_steps, int slices_log2, int out_features, int in_features,
                                                     uint8_t* slice_groups) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_geometry, slice_steps, slices_log2, out_features, in_features, slice_groups);
  if (!slice_steps || !slice_groups || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_geometry: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  unsigned long long st[PK_S];
  for (int s = 0; s < PK_S; ++s) st[s] = slice_steps[s];
  return plan_geometry(st, out_features, in_features, slice_groups);
}

// scratch of the repack, kept in the tail of the caller's capacity: usage counts, the relabelling table, lane-steps per
// (slice, row), lane-steps per slice
struct PkScratch {
  size_t off_hist, off_relabel, off_ls, off_steps, bytes;
};
static PkScratch pk_scratch(int M) {
  PkScratch sc;
  sc.off_hist = 0;
  sc.off_relabel = sc.off_hist + (size_t)65536 * 4;
  sc.off_ls = sc.off_relabel + (size_t)65536 * 2;
  sc.off_steps = align_up(sc.off_ls + (size_t)PK_S * M * 2, 256);
  sc.bytes = align_up(sc.off_steps + PK_S * 4, 1024);
  return sc;
}

extern "C" PK_API size_t PK_ENTRY(prepack_1x16_bytes)(int out_features, int in_features, int in_group_size) {
  PK_G16_FORWARD_IF(in_group_size == 16, prepack_1x16_bytes, out_features, in_features, in_group_size);
  if (!packed_shape_ok(out_features, in_features, in_group_size)) return 0;
  // capacity for streams up to 1.5 x the balanced length (the repack balances the slices; what is left is the difference
  // between the rows of one slice), plus the permutation + codebook image of a relabelled buffer and the repack's scratch;
  // the bytes actually used come back in the descriptor and the buffer may be trimmed to them
  const size_t nst = (size_t)PK_NST;
  const size_t M = (size_t)out_features;
  const size_t RG2 = (M + PK_MIN_GROUPS - 1) / PK_MIN_GROUPS;                 // rows per group at most (variable geometry)
  const size_t in_groups = (size_t)in_features / PK_G;
  const size_t fair = (M * in_groups / 4 + (size_t)PK_S * M) / nst;            // lane-steps per stream when all are equal
  const size_t lane_steps = fair * 3 / 2 + RG2 + 64;                           // per stream
  const size_t ent = nst * (lane_steps * 16 + 16 * 1024);
  const size_t meta = 4096 + nst * PK_MAX_NW * 16 + nst * (RG2 + 1) * 4 + (size_t)AQLM_HIP_MAX_GEMV_BATCH * out_features * 8;
  const size_t image = (size_t)65536 * 2 + (size_t)65536 * PK_VB + 2048;
  // 3-byte entries: the repack builds the 4-byte layout in the tail of the buffer and squeezes it to the front
  return align_up(meta + ent + ent * PK_WREG3 / 1024 + image + pk_scratch(out_features).bytes + 4096, 1024);
}

extern "C" PK_API int PK_ENTRY(prepack_1x16_ex)(const void* codes, int out_features, int in_features, int in_group_size,
                                                void* packed, size_t packed_bytes, aqlm_hip_packed_desc* desc, int flags, void* stream_) {
  PK_G16_FORWARD_IF(in_group_size == 16, prepack_1x16_ex, codes, out_features, in_features, in_group_size, packed, packed_bytes, desc, flags, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  if (!codes || !packed || !desc) {
    set_last_error("aqlm_hip_prepack_1x16: null pointer argument");
    return AQLM_HIP_E_INVALID;
  }
  if (!packed_shape_ok(out_features, in_features, in_group_size)) {
    set_last_error("aqlm_hip_prepack_1x16: unsupported shape (needs g=%d, in/g <= %d; got g=%d in=%d out=%d)", PK_G, PK_MAX_GROUPS,
                   in_group_size, in_features, out_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t cap = PK_ENTRY(prepack_1x16_bytes)(out_features, in_features, in_group_size);
  if (packed_bytes < cap || !aligned16(packed)) {
    set_last_error("aqlm_hip_prepack_1x16: packed buffer needs %zu bytes (16-B aligned), got %zu", cap, packed_bytes);
    return AQLM_HIP_E_INVALID;
  }
  const int M = out_features, in_groups = in_features / PK_G;
  const size_t nst = (size_t)PK_NST;
  uint8_t* base = (uint8_t*)packed;
  const PkScratch sc = pk_scratch(M);
  const size_t work_end = (packed_bytes - sc.bytes) / 1024 * 1024;  // the layout (and the 4-byte working copy of 3-byte entries) stay below
  uint8_t* scratch = base + work_end;
  uint32_t* hist_d = (uint32_t*)(scratch + sc.off_hist);
  uint16_t* relabel_d = (uint16_t*)(scratch + sc.off_relabel);
  uint16_t* ls_d = (uint16_t*)(scratch + sc.off_ls);
  uint32_t* steps_d = (uint32_t*)(scratch + sc.off_steps);
  const int row_blocks = (M + 3) / 4;
  uint32_t* maxL_d = (uint32_t*)(base + 128);
  uint8_t groups[32] = {};
  for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)PK_NG;
  std::vector<uint16_t> new_of_old, old_of_new;
  bool relabel = false;
  uint32_t steps_h[PK_S];
  uint32_t maxL = 0;
  // wave-steps a workgroup runs when its longest stream has L lane-steps (what the balancing can change at all: the kernel
  // runs whole steps of whole waves)
  auto capacity = [](uint32_t L) {
    const int nw = choose_waves(L);
    return (uint64_t)nw * ((L + 64u * nw - 1) / (64u * nw));
  };
  // counts lane-steps per (slice, row) with the given labels, builds the row starts of every stream for `groups` in place (their
  // offset does not depend on the wave count chosen later) and reads back the longest stream
  PackedLayout L0;
  auto count_and_scan = [&](const uint16_t* rl) -> int {
    if (!packed_layout(M, in_features, 1, 1, L0, 1, 4, groups, relabel)) {
      set_last_error("aqlm_hip_prepack_1x16: internal: geometry plan rejected");
      return AQLM_HIP_E_INVALID;
    }
    if (L0.off_ent > work_end) {
      set_last_error("aqlm_hip_prepack_1x16: capacity too small for the row tables");
      return AQLM_HIP_E_INVALID;
    }
    if (int e = check_hip(hipMemsetAsync(base, 0, L0.off_ent, stream), "prepack memset")) return e;
    if (int e = check_hip(hipMemsetAsync(steps_d, 0, PK_S * 4, stream), "prepack memset")) return e;
    hipLaunchKernelGGL(pk_count_kernel, dim3(row_blocks), dim3(256), 0, stream, (const uint16_t*)codes, rl, ls_d, steps_d, M, in_groups);
    hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)nst), dim3(256), 0, stream, ls_d, (uint32_t*)(base + L0.off_rowstart), maxL_d, L0.G);
    if (int e = check_hip(hipMemcpyAsync(steps_h, steps_d, PK_S * 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
    if (int e = check_hip(hipMemcpyAsync(&maxL, maxL_d, 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
    return check_hip(hipStreamSynchronize(stream), "prepack sync");
  };
  // (1) the checkpoint's labels on the 16 x 16 geometry
  if (int e = count_and_scan(nullptr)) return e;
  // Balancing is for the longest stream: when it already runs as few wave-steps as perfectly even streams would (+3.5 %: the
  // noise between the row groups of uniform codes), labels and geometry stay -- no permutation, no codebook image.
  unsigned long long total_steps = 0;
  for (int s = 0; s < PK_S; ++s) total_steps += steps_h[s];
  const uint32_t even = (uint32_t)((total_steps * 1035ull + (unsigned long long)PK_NST * 1000ull - 1ull) / ((unsigned long long)PK_NST * 1000ull));
  const bool balanced = capacity(maxL) <= capacity(even);
  if (!balanced) {
    // (2) usage counts -> relabelling plan -> lane-steps with the new labels
    if (!(flags & AQLM_HIP_PREPACK_NO_RELABEL)) {
      std::vector<uint32_t> usage(65536);
      if (int e = check_hip(hipMemsetAsync(hist_d, 0, (size_t)65536 * 4, stream), "prepack memset")) return e;
      hipLaunchKernelGGL(pk_hist_kernel, dim3(2048), dim3(256), 0, stream, (const uint16_t*)codes, (size_t)M * in_groups, hist_d);
      if (int e = check_hip(hipMemcpyAsync(usage.data(), hist_d, (size_t)65536 * 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
      if (int e = check_hip(hipStreamSynchronize(stream), "prepack sync")) return e;
      new_of_old.resize(65536);
      // forced: the layout is not balanced although the global masses may be (label use correlated with the row); kept only when
      // the longest stream runs fewer wave-steps with the new labels
      const uint32_t maxL_before = maxL;
      relabel = plan_relabel(usage.data(), new_of_old.data(), /*force=*/true) == 1;
      if (relabel) {
        old_of_new.resize(65536);
        for (uint32_t c = 0; c < 65536; ++c) old_of_new[new_of_old[c]] = (uint16_t)c;
        if (int e = check_hip(hipMemcpyAsync(relabel_d, new_of_old.data(), (size_t)65536 * 2, hipMemcpyHostToDevice, stream), "prepack relabel table")) return e;
        if (int e = count_and_scan(relabel_d)) return e;
        if (capacity(maxL) >= capacity(maxL_before)) {  // the deal did not help (e.g. one row that lives in one slice): labels as they are
          relabel = false;
          if (int e = count_and_scan(nullptr)) return e;
        }
      }
    }
    // (3) an entry that outweighs a slice: deal the workgroups to the slices by their work
    if (!(flags & AQLM_HIP_PREPACK_UNIFORM_ONLY)) {
      unsigned long long steps64[PK_S];
      for (int s = 0; s < PK_S; ++s) steps64[s] = steps_h[s];
      if (plan_geometry(steps64, M, in_features, groups))
        if (int e = count_and_scan(relabel ? relabel_d : nullptr)) return e;
    }
  }
  const uint16_t* rl = relabel ? relabel_d : nullptr;
  const PkGeom G = L0.G;
  uint32_t* a = (uint32_t*)(base + L0.off_rowstart);
  const int NW = choose_waves(maxL);
  const int T = (int)((maxL + 64u * NW - 1) / (64u * NW));
  const bool arrange = tuning().packed_arrange && T <= PK_ARR_MAX_T;
  // rotated copies of x: 1 by default -- with the row pools the x reads are already spread well, and up to 4 copies
  // measured within +-1 % (profiles/r02_mb_packed_variants.log); the knob keeps the mechanism testable
  int XC = 1;
  if (AQLM_PK_XFIRST && PK_G == 8 && arrange && !packed_b1_slice_first(in_groups, G.RG) && tuning().packed_xcopies >= 1 && tuning().packed_xcopies <= 4) XC = std::min(pk_max_x_copies(in_groups), tuning().packed_xcopies);
  // 32-bit entries by default (two operations instead of four to form an entry's addresses); 24-bit entries (-23 % bytes; wave
  // ranges of at most 32 steps) are the compact choice for inference-only deployments.  Re-measured per shape in round 5 (profiles/r05_entry_bytes_3_vs_4.md, A/B/A/B on one box): 24-bit
  // entries cost 5.8 % on 4096 x 4096, 3.3 % on 4096 -> 11008, 3.2 % on 4096 -> 1024, 2.3 % on 8192 x 8192 and 1.3-1.4 % on
  // 4096 <-> 14336; layers of more than 32 steps per wave (the 70B MLP) cannot take them at all.  They also keep a shared-input group
  // off the pipelined kernel (4-byte entries only).  So they stay the opt-in compact form (tuning key 3, `prepack_model(compact=True)`).
  const int EB = (PK_G == 8 && tuning().packed_entry_bytes == 3 && T <= 32 && !G.vg) ? 3 : 4;  // (the 3-byte form exists for 16-B vectors and uniform geometry only)
  PackedLayout L, L4;
  if (!packed_layout(M, in_features, NW, T, L, XC, EB, groups, relabel) || !packed_layout(M, in_features, NW, T, L4, XC, 4, groups, relabel) ||
      L.used + (EB == 3 ? L4.ent_bytes + 1024 : 0) > work_end) {
    set_last_error("aqlm_hip_prepack_1x16: the rows of this layer use the codebook too differently from one another for the packed "
                   "format (longest stream %u lane-steps after balancing, %d steps per wave)", maxL, T);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  uint32_t* winfo = (uint32_t*)(base + L.off_winfo);
  // the 4-byte working layout: in place for 4-byte entries, else in the tail of the capacity
  uint32_t* ent = EB == 4 ? (uint32_t*)(base + L.off_ent) : (uint32_t*)(base + (work_end - L4.ent_bytes) / 1024 * 1024);
  aqlm_hip_packed_desc d{};
  d.magic = PK_MAGIC;
  d.version = PK_VERSION;
  d.out_features = M;
  d.in_features = in_features;
  d.slices_log2 = PK_S_LOG;
  d.waves = NW;
  d.steps = T;
  d.entry_bytes = EB;
  d.used_bytes = L.used;
  d.x_copies = (uint32_t)XC;
  d.codebook_absmax = 0.f;  // unknown: the caller sets it (see include/aqlm_hip.h) to enable the fused finalize
  d.flags = (relabel ? AQLM_HIP_PACKED_RELABELLED : 0u) | (G.vg ? AQLM_HIP_PACKED_VARGEOM : 0u);
  d.rows_per_group = G.RG;
  for (int s = 0; s < PK_S; ++s) d.slice_groups[s] = groups[s];
  if (int e = check_hip(hipMemcpyAsync(base, &d, sizeof(d), hipMemcpyHostToDevice, stream), "prepack header")) return e;
  const uint32_t null_entry = (uint32_t)in_groups << (16 + PK_VSH);
  hipLaunchKernelGGL(pk_fill_kernel, dim3(2048), dim3(256), 0, stream, ent, L4.ent_bytes / 4, null_entry);
  hipLaunchKernelGGL(pk_scatter_kernel, dim3(row_blocks), dim3(256), 0, stream, (const uint16_t*)codes, rl, a, ent, G, in_groups, NW, T);
  if (arrange)
    hipLaunchKernelGGL(pk_arrange_kernel, dim3((unsigned)nst, NW), dim3(64), (size_t)T * 1024 + (size_t)T * 256, stream, a,
                       ent, G, in_groups, NW, T, XC);
  // the local search on the greedy deal (1-3 % faster matvec) takes ~10x the greedy deal's time (27 -> 120 ms for a 29 M-code
  // layer): by default (1) only layers of <= 8 Mi codes get it -- a 70B model then prepacks in ~13 s instead of ~1 min --,
  // 3 = always, 2 = never
  if (arrange && (tuning().packed_arrange == 3 || (tuning().packed_arrange == 1 && (long)M * in_groups <= PK_IMPROVE_MAX_CODES)))
    hipLaunchKernelGGL(pk_improve_kernel, dim3((unsigned)nst, NW), dim3(64), (size_t)T * (1024 + 512 + 256 + 32), stream, a, ent, G,
                       in_groups, NW, T);
  if (PK_PARITY_BITS) hipLaunchKernelGGL(pk_parity_kernel, dim3(2048), dim3(256), 0, stream, ent, L4.ent_bytes / 4);
  hipLaunchKernelGGL(pk_flag_kernel, dim3((G.RG + 255) / 256, (unsigned)nst), dim3(256), 0, stream, a, ent, G, NW, T);
  hipLaunchKernelGGL(pk_column_kernel, dim3((unsigned)nst, NW), dim3(64), 0, stream, a, ent, winfo, G, NW, T);
  if (EB == 3)
    hipLaunchKernelGGL(pk_compress_kernel, dim3((unsigned)nst, NW), dim3(64), 0, stream, ent, base + L.off_ent, winfo, G, NW, T);
  if (int e = check_hip(hipGetLastError(), "prepack launch")) return e;
  if (relabel) {  // the permutation travels with the buffer: unpack and the codebook image are made from it
    if (int e = check_hip(hipMemcpyAsync(base + L.off_perm, old_of_new.data(), (size_t)65536 * 2, hipMemcpyHostToDevice, stream), "prepack permutation")) return e;
  }
  if (int e = check_hip(hipStreamSynchronize(stream), "prepack sync")) return e;  // `d` and the tables live on the host stack / heap
  *desc = d;
  return 0;
}

extern "C" PK_API int PK_ENTRY(prepack_1x16)(const void* codes, int out_features, int in_features, int in_group_size,
                                      void* packed, size_t packed_bytes, aqlm_hip_packed_desc* desc, void* stream_) {
  return PK_ENTRY(prepack_1x16_ex)(codes, out_features, in_features, in_group_size, packed, packed_bytes, desc, 0, stream_);
}

// codebook image of a relabelled buffer: image[new] = codebook[old_of_new[new]], one 16-B piece per thread
namespace aqlm {
namespace PK_NS {
__global__ __launch_bounds__(256) void pk_codebook_image_kernel(const uint16_t* old_of_new, const u32x4* codebook, u32x4* image) {
  constexpr uint32_t PIECES = PK_VB / 16;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // < 65536 * PIECES
  const uint32_t c = i / PIECES, h = i - c * PIECES;
  image[i] = codebook[(uint32_t)old_of_new[c] * PIECES + h];
}
}  // namespace PK_NS
}  // namespace aqlm

extern "C" PK_API int PK_ENTRY(packed_set_codebook)(aqlm_hip_packed_desc* desc, void* packed, const void* codebook, void* stream_) {
  PK_G16_FORWARD(desc, packed_set_codebook, desc, packed, codebook, stream_);
  PackedLayout L;
  if (!packed || !codebook || !desc_layout(desc, L) || !aligned16(packed) || !aligned16(codebook)) {
    set_last_error("aqlm_hip_packed_set_codebook: null / misaligned pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  if (!L.relabel) return 0;  // the kernels read the caller's codebook
  uint8_t* base = (uint8_t*)packed;
  hipLaunchKernelGGL(pk_codebook_image_kernel, dim3(65536u * (PK_VB / 16) / 256u), dim3(256), 0, (hipStream_t)stream_,
                     (const uint16_t*)(base + L.off_perm), (const u32x4*)codebook, (u32x4*)(base + L.off_cb));
  if (int e = check_hip(hipGetLastError(), "codebook image launch")) return e;
  desc->flags |= AQLM_HIP_PACKED_HAS_CODEBOOK;
  return 0;
}

extern "C" PK_API int PK_ENTRY(packed_desc_read)(const void* header_host, size_t header_bytes, aqlm_hip_packed_desc* desc) {
  if (header_host && desc && header_bytes >= sizeof(aqlm_hip_packed_desc)) {
    aqlm_hip_packed_desc h;
    memcpy(&h, header_host, sizeof(h));
    PK_G16_FORWARD(&h, packed_desc_read, header_host, header_bytes, desc);
  }
  if (!header_host || !desc || header_bytes < sizeof(aqlm_hip_packed_desc)) {
    set_last_error("aqlm_hip_packed_desc_read: need the first %zu bytes of the packed buffer", sizeof(aqlm_hip_packed_desc));
    return AQLM_HIP_E_INVALID;
  }
  aqlm_hip_packed_desc d;
  memcpy(&d, header_host, sizeof(d));
  PackedLayout L;
  if (!desc_layout(&d, L)) {
    set_last_error("aqlm_hip_packed_desc_read: not a packed 1x16 buffer of format v6");
    return AQLM_HIP_E_INVALID;
  }
  *desc = d;
  return 0;
}

extern "C" PK_API int PK_ENTRY(unpack_1x16)(const aqlm_hip_packed_desc* desc, const void* packed, void* codes, void* stream_) {
  PK_G16_FORWARD(desc, unpack_1x16, desc, packed, codes, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  if (!packed || !codes || !desc_layout(desc, L)) {
    set_last_error("aqlm_hip_unpack_1x16: null pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint16_t* perm = L.relabel ? (const uint16_t*)(base + L.off_perm) : nullptr;  // relabelled: back to the checkpoint's labels
  if (L.EB == 3)
    hipLaunchKernelGGL(pk_unpack3_kernel, dim3((unsigned)L.nst, L.NW), dim3(64), 0, stream, base + L.off_ent,
                       (const uint32_t*)(base + L.off_winfo), perm, (uint16_t*)codes, L.G, L.in_groups, L.NW, L.T);
  else
    hipLaunchKernelGGL(pk_unpack_kernel, dim3((unsigned)L.nst, L.NW), dim3(64), 0, stream, (const uint32_t*)(base + L.off_ent),
                       (const uint32_t*)(base + L.off_winfo), perm, (uint16_t*)codes, L.G, L.in_groups, L.NW, L.T);
  return check_hip(hipGetLastError(), "unpack launch");
}

// W from the packed buffer (pk_dequant_kernel).  Reads the entries, the permutation stored behind them and the CALLER's codebook:
// never the permuted codebook image, whose flag and the descriptor's codebook range are not looked at.
extern "C" PK_API int PK_ENTRY(dequant_1x16_packed)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                    const void* scales, void* W, int dtype, void* stream_) {
  PK_G16_FORWARD(desc, dequant_1x16_packed, desc, packed, codebook, scales, W, dtype, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  if (!packed || !codebook || !W || !desc_layout(desc, L)) {
    set_last_error("aqlm_hip_dequant_1x16_packed: null pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  if (!aligned16(packed) || !aligned16(codebook) || !aligned16(W)) {
    set_last_error("aqlm_hip_dequant_1x16_packed: packed, codebook and W must be 16-byte aligned");
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("aqlm_hip_dequant_1x16_packed: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)", dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint16_t* perm = L.relabel ? (const uint16_t*)(base + L.off_perm) : nullptr;
  // grid order (measured, profiles/packed_dequant.json): one row group per XCD is 7 % / 4 % faster at 4096 x 4096 / 8192 -> 28672 and 2 %
  // slower at 4096 <-> 14336 for 16-B vectors; with 32-B vectors (a quarter of a line per store) the stream-major grid is 6 % faster
  const int knob = tuning().packed_dequant_by_xcd;
  const int by_xcd = !L.G.vg && (knob == 2 || (knob == 1 && PK_G == 8)) ? 1 : 0;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)(L.nst * L.NW)), dim3(64), 0, stream, base + L.off_ent, (const uint32_t*)(base + L.off_winfo), perm,
                       (const u32x4*)codebook, (const uint16_t*)scales, (uint16_t*)W, L.G, L.in_groups, L.NW, L.T, by_xcd);
    return check_hip(hipGetLastError(), "packed dequant launch");
  };
#define AQLM_PK_DQ(TT, EE) (perm ? go(pk_dequant_kernel<TT, EE, true>) : go(pk_dequant_kernel<TT, EE, false>))
#if AQLM_PK_G == 8
  if (L.EB == 3) return dtype == AQLM_HIP_F16 ? AQLM_PK_DQ(F16, 3) : AQLM_PK_DQ(BF16, 3);
#endif
  return dtype == AQLM_HIP_F16 ? AQLM_PK_DQ(F16, 4) : AQLM_PK_DQ(BF16, 4);
#undef AQLM_PK_DQ
}

// The fused finalize needs the layer's codebook range (descriptor field) and can be switched off for A/B runs.
static bool packed_fused(const aqlm_hip_packed_desc* desc) {
  return tuning().packed_fused_finalize != 0 && desc->codebook_absmax > 0.f && desc->codebook_absmax < __builtin_inff();
}

// main kernel of one launch (<= packed_max_batch rows).  With `fused.y` it also finalizes (accumulator cells inside the
// packed buffer, no workspace); without, it leaves fp32 slice partials [16][nb][M] in the workspace.
struct PackedFused {
  const void* scales = nullptr;
  const void* bias = nullptr;
  void* y = nullptr;
  long y_row_stride = 0;
  float cb_absmax = 0.f;
  void* cells = nullptr;  // caller-owned accumulator cells [rows][M] u64, zero at rest (one set per stream); null: the cells inside the packed buffer
  // row-parallel shard: publish the fp32 totals (aqlm_hip_gemv_1x16_packed_publish) instead of writing y
  float* pub = nullptr;
  uint32_t* pub_flag = nullptr;
  uint32_t* pub_epoch = nullptr;
  uint32_t pub_max_elems = 0;
};

// the layer that runs next on the stream (chain prefetch); all null = none
struct PackedNext {
  const uint8_t* ent = nullptr;
  const uint8_t* codebook = nullptr;
  uint32_t block_bytes = 0;
};

static int packed_launch_main(const PackedLayout& L, const void* packed, const void* codebook, const uint16_t* x, int nb,
                              long x_row_stride, int dtype, void* workspace, size_t workspace_bytes, hipStream_t stream,
                              const char* who, const PackedFused& fused = PackedFused{}, const PackedNext& next = PackedNext{}) {
  const bool finalizes = fused.y || fused.pub;
  const size_t need = finalizes ? 0 : (size_t)PK_S * nb * L.M * sizeof(float);
  if (need && (!workspace || workspace_bytes < need)) {
    set_last_error("%s: workspace of %zu bytes required, got %zu", who, need, workspace_bytes);
    return AQLM_HIP_E_INVALID;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint32_t* ent = (const uint32_t*)(base + L.off_ent);
  const uint32_t* rowstart = (const uint32_t*)(base + L.off_rowstart);
  const uint8_t* cb = L.relabel ? base + L.off_cb : (const uint8_t*)codebook;  // relabelled: the permuted image (aqlm_hip_packed_set_codebook)
  // the trailing kernel argument as both launches below pass it; the ordinary one adds the publish and next-layer fields
  PackedGemvRest rest{};
  rest.winfo = (const uint32_t*)(base + L.off_winfo);
  rest.partial = (float*)workspace;
  rest.x_row_stride = x_row_stride;
  if (finalizes) {
    rest.acc = fused.cells ? (unsigned long long*)fused.cells : (unsigned long long*)(const_cast<uint8_t*>(base) + L.off_acc);
    rest.cb_absmax = fused.cb_absmax;
    rest.scales = (const uint16_t*)fused.scales;
    rest.bias = (const uint16_t*)fused.bias;
    rest.y = (uint16_t*)fused.y;
    rest.y_row_stride = fused.y_row_stride;
  }
#ifdef AQLM_PACKED_TRACE
  rest.trace = workspace && workspace_bytes >= need + (size_t)PK_NST * PK_MAX_NW * 8 * 8 ? (unsigned long long*)((uint8_t*)workspace + need) : nullptr;
  rest.dbg = tuning().packed_debug;
#endif
  // chain prefetch: up to `packed_prefetch_waves` extra waves per workgroup (default 2) when a next layer is named
  int npw = 0;
  if (next.ent && next.codebook && next.block_bytes) {
    const int want = tuning().packed_prefetch_waves < 0 ? 0 : (tuning().packed_prefetch_waves == 0 ? 2 : tuning().packed_prefetch_waves);
    npw = std::min(std::min(want, 7), PK_MAX_NW - L.NW);
  }
  const uint32_t rotate = tuning().packed_fill_rotate ? 1u : 0u;
  auto launch = [&](auto kern, auto lds_map) -> int {
    const size_t lds = decltype(lds_map)::total(L.in_groups, L.RG, npw);
    if (lds > 160 * 1024) { npw = 0; }
    const size_t lds_final = decltype(lds_map)::total(L.in_groups, L.RG, npw);
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_final)) return e;
    PackedGemvRest r = rest;
    r.pub = fused.pub;
    r.pub_flag = fused.pub_flag;
    r.pub_epoch = fused.pub_epoch;
    r.pub_max_elems = fused.pub_max_elems;
    if (npw) {
      r.next_ent = next.ent;
      r.next_codebook = next.codebook;
      r.next_block_bytes = next.block_bytes;
    }
    hipLaunchKernelGGL(kern, dim3(PK_NST), dim3((L.NW + npw) * 64), lds_final, stream, cb, x, ent, rowstart, L.in_groups,
                       (uint32_t)L.NW | ((uint32_t)L.XC << 8) | ((uint32_t)npw << 12) | (rotate << 15) | ((uint32_t)L.T << 16), L.RG,
                       (uint32_t)L.ent_bytes, L.M, r);
    return check_hip(hipGetLastError(), "gemv_1x16_packed launch");
  };
  const bool sf = nb == 1 && packed_b1_slice_first(L.in_groups, L.RG);
#if AQLM_PK_G == 8
  if (L.G.vg) {  // variable geometry: its own kernels (4-byte entries, ring depth 3 / 4, no chain prefetch, no publish)
    if (fused.pub != nullptr || L.EB != 4) {
      set_last_error("%s: a variable-geometry buffer runs on the single-layer matvec entries only (repack with "
                     "AQLM_HIP_PREPACK_UNIFORM_ONLY for the publish form)", who);
      return AQLM_HIP_E_UNSUPPORTED;
    }
    uint32_t ns[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < PK_S; ++i) ns[i >> 2] |= (uint32_t)L.G.first[i] << ((i & 3) * 8);  // first stream of every slice (< 256)
    auto launch_vg = [&](auto kern, auto lds_map) -> int {
      const size_t lds = decltype(lds_map)::total(L.in_groups, L.RG, 0);
      if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
      hipLaunchKernelGGL(kern, dim3(PK_NST), dim3(L.NW * 64), lds, stream, cb, x, ent, (uint32_t)(L.off_ent - L.off_rowstart),
                         (uint32_t)L.in_groups | ((uint32_t)L.RG << 12), (uint32_t)L.NW | ((uint32_t)L.XC << 8) | (rotate << 15) | ((uint32_t)L.T << 16),
                         L.M, ns[0], ns[1], ns[2], ns[3], rest);
      return check_hip(hipGetLastError(), "gemv_1x16_packed (variable geometry) launch");
    };
#define AQLM_PK_VG(TT, BB, PP, XW) launch_vg(gemv_1x16_packed_vg_kernel<TT, BB, PP, XW>, PackedLds<BB, XW>{})
#define AQLM_PK_VG_CASE(BB) \
  case BB:                  \
    return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, BB, 4, PK_XWIN_FULL) : AQLM_PK_VG(BF16, BB, 4, PK_XWIN_FULL);
    switch (nb) {
      case 1:
        if (sf) return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, 1, 3, 0u) : AQLM_PK_VG(BF16, 1, 3, 0u);
        return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, 1, 3, PK_XWIN_FULL) : AQLM_PK_VG(BF16, 1, 3, PK_XWIN_FULL);
      AQLM_PK_VG_CASE(2)
      AQLM_PK_VG_CASE(3)
      AQLM_PK_VG_CASE(4)
      AQLM_PK_VG_CASE(5)
      AQLM_PK_VG_CASE(6)
      AQLM_PK_VG_CASE(7)
      AQLM_PK_VG_CASE(8)
    }
#undef AQLM_PK_VG_CASE
#undef AQLM_PK_VG
    return AQLM_HIP_E_INVALID;
  }
#endif
  if (fused.pub != nullptr) return dispatch_packed<PublishKernels>(dtype, nb, pick_pd(L), L.EB, sf, launch);
  return dispatch_packed<SingleKernels>(dtype, nb, pick_pd(L), L.EB, sf, launch);
}

static int packed_check_args(const char* who, const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                             const void* x, int batch, long x_row_stride, int dtype, PackedLayout& L, int& max_b) {
  if (!packed || !codebook || !x || !desc) {
    set_last_error("%s: null pointer argument", who);
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("%s: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)", who, dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (!desc_layout(desc, L)) {
    set_last_error("%s: invalid packed descriptor", who);
    return AQLM_HIP_E_INVALID;
  }
  if (batch < 1 || batch > AQLM_HIP_MAX_GEMV_BATCH || !aligned16(packed) || !aligned16(codebook) || !aligned16(x) ||
      (batch > 1 && x_row_stride % 8 != 0)) {
    set_last_error("%s: batch must be 1..%d and packed / codebook / x rows 16-B aligned (batch %d)", who,
                   AQLM_HIP_MAX_GEMV_BATCH, batch);
    return AQLM_HIP_E_INVALID;
  }
  if (L.relabel && !(desc->flags & AQLM_HIP_PACKED_HAS_CODEBOOK)) {
    set_last_error("%s: a relabelled buffer needs its codebook image: call aqlm_hip_packed_set_codebook first (and again whenever "
                   "the codebook changes)", who);
    return AQLM_HIP_E_INVALID;
  }
  max_b = packed_max_batch(L.in_groups, L.RG);
  if (max_b == 0) {
    set_last_error("%s: layer does not fit the LDS image (in_features %d)", who, desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return 0;
}

static int gemv_1x16_packed_impl(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                 const void* scales, const void* bias, const void* x, void* y, int batch,
                                 long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                 size_t workspace_bytes, void* stream_, const PackedNext& next, void* cells = nullptr,
                                 size_t cells_bytes = 0) {
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  int max_b = 0;
  if (!scales || !y) {
    set_last_error("aqlm_hip_gemv_1x16_packed: null pointer argument");
    return AQLM_HIP_E_INVALID;
  }
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b)) return e;
  for (int b0 = 0; b0 < batch; b0 += max_b) {  // rows that do not fit one LDS image go in several launches
    const int nb = std::min(max_b, batch - b0);
    if (packed_fused(desc)) {
      PackedFused fz;
      fz.cb_absmax = desc->codebook_absmax;
      fz.scales = scales;
      fz.bias = bias;
      fz.y = (uint16_t*)y + (size_t)b0 * y_row_stride;
      fz.y_row_stride = y_row_stride;
      fz.cells = cells;  // launches of one call are stream-ordered: they share the cells
      if (int e = packed_launch_main(L, packed, codebook, (const uint16_t*)x + (size_t)b0 * x_row_stride, nb, x_row_stride, dtype,
                                     workspace, workspace_bytes, stream, "aqlm_hip_gemv_1x16_packed", fz,
                                     b0 + nb >= batch ? next : PackedNext{}))
        return e;
      continue;
    }
    if (int e = packed_launch_main(L, packed, codebook, (const uint16_t*)x + (size_t)b0 * x_row_stride, nb, x_row_stride, dtype,
                                   workspace, workspace_bytes, stream, "aqlm_hip_gemv_1x16_packed"))
      return e;
    PackedFinalizeParams f{};
    f.partial = (const float*)workspace;
    f.scales = (const uint16_t*)scales;
    f.bias = (const uint16_t*)bias;
    f.y = (uint16_t*)y + (size_t)b0 * y_row_stride;
    f.y_row_stride = y_row_stride;
    f.M = L.M;
    f.B = nb;
    if (dtype == AQLM_HIP_F16)
      hipLaunchKernelGGL(gemv_1x16_packed_finalize<F16>, dim3((L.M + 255) / 256), dim3(256), 0, stream, f.partial, f.scales, f.bias,
                         f.y, f.y_row_stride, f.M, f.B);
    else
      hipLaunchKernelGGL(gemv_1x16_packed_finalize<BF16>, dim3((L.M + 255) / 256), dim3(256), 0, stream, f.partial, f.scales, f.bias,
                         f.y, f.y_row_stride, f.M, f.B);
    if (int e = check_hip(hipGetLastError(), "gemv_1x16_packed_finalize launch")) return e;
  }
  return 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_cells)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                const void* scales, const void* bias, const void* x, void* y, int batch,
                                                long x_row_stride, long y_row_stride, int dtype, void* cells,
                                                size_t cells_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_cells, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, cells, cells_bytes, stream_);
  if (!cells || !desc || !(desc->codebook_absmax > 0.f) || cells_bytes < (size_t)std::min(batch, AQLM_HIP_MAX_GEMV_BATCH) * desc->out_features * 8 ||
      (reinterpret_cast<uintptr_t>(cells) & 7u)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_cells: needs a descriptor with the codebook range and %zu bytes of 8-B aligned, "
                   "zero-filled cells", desc ? (size_t)std::min(batch, AQLM_HIP_MAX_GEMV_BATCH) * desc->out_features * 8 : (size_t)0);
    return AQLM_HIP_E_INVALID;
  }
  if (!tuning().packed_fused_finalize) {
    set_last_error("aqlm_hip_gemv_1x16_packed_cells: the fused finalize is switched off (tuning knob packed_fused_finalize)");
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return gemv_1x16_packed_impl(desc, const_cast<void*>(packed), codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype,
                               nullptr, 0, stream_, PackedNext{}, cells, cells_bytes);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                          const void* scales, const void* bias, const void* x, void* y, int batch,
                                          long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace, workspace_bytes, stream_);
  return gemv_1x16_packed_impl(desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace,
                               workspace_bytes, stream_, PackedNext{});
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_chain)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                                const void* scales, const void* bias, const void* x, void* y, int batch,
                                                long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                                size_t workspace_bytes, const aqlm_hip_packed_desc* next_desc,
                                                const void* next_packed, const void* next_codebook, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_chain, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace, workspace_bytes, next_desc, next_packed, next_codebook, stream_);
  PackedNext next;
  PackedLayout LN;
  if (next_desc && next_packed && next_codebook) {
    if (!desc_layout(next_desc, LN) || !aligned16(next_packed) || !aligned16(next_codebook)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_chain: invalid descriptor / misaligned buffer of the next layer");
      return AQLM_HIP_E_INVALID;
    }
    next.ent = (const uint8_t*)next_packed + LN.off_ent;
    next.codebook = LN.relabel ? (const uint8_t*)next_packed + LN.off_cb : (const uint8_t*)next_codebook;
    next.block_bytes = (uint32_t)(LN.ent_bytes / LN.nst);
    if (LN.G.vg) next = PackedNext{};  // the hint assumes workgroup b of both layers sits on one XCD with the same slice: uniform geometry only
  }
  return gemv_1x16_packed_impl(desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace,
                               workspace_bytes, stream_, next);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_partials)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                   const void* x, int batch, long x_row_stride, int dtype, void* workspace,
                                                   size_t workspace_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_partials, desc, packed, codebook, x, batch, x_row_stride, dtype, workspace, workspace_bytes, stream_);
  PackedLayout L;
  int max_b = 0;
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed_partials", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b))
    return e;
  if (batch > max_b) {
    set_last_error("aqlm_hip_gemv_1x16_packed_partials: %d rows do not fit one LDS image (at most %d for in_features %d)", batch,
                   max_b, desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return packed_launch_main(L, packed, codebook, (const uint16_t*)x, batch, x_row_stride, dtype, workspace, workspace_bytes,
                            (hipStream_t)stream_, "aqlm_hip_gemv_1x16_packed_partials");
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_publish)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                                  const void* x, int batch, long x_row_stride, int dtype,
                                                  const aqlm_hip_xgmi* xg, void* pub_own, void* flag_own, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_publish, desc, packed, codebook, x, batch, x_row_stride, dtype, xg, pub_own, flag_own, stream_);
  PackedLayout L;
  int max_b = 0;
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed_publish", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b))
    return e;
  if (!xg || !xg->epoch || !pub_own || !flag_own || !packed_fused(desc) || batch > max_b ||
      (size_t)batch * desc->out_features > (size_t)xg->max_elems) {
    set_last_error("aqlm_hip_gemv_1x16_packed_publish: needs the one-shot all-reduce state, a descriptor with the codebook range, "
                   "and batch (%d) rows that fit one launch (<= %d) and the state (%d elements)", batch, max_b, xg ? xg->max_elems : 0);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  PackedFused fz;
  fz.cb_absmax = desc->codebook_absmax;
  fz.pub = (float*)pub_own;
  fz.pub_flag = (uint32_t*)flag_own;
  fz.pub_epoch = (uint32_t*)xg->epoch;
  fz.pub_max_elems = (uint32_t)xg->max_elems;
  return packed_launch_main(L, packed, codebook, (const uint16_t*)x, batch, x_row_stride, dtype, nullptr, 0, (hipStream_t)stream_,
                            "aqlm_hip_gemv_1x16_packed_publish", fz);
}

static int gemv_1x16_packed_multi_impl(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                       int num_segments, const void* x, int in_features, int batch, long x_row_stride,
                                       int dtype, void* workspace, size_t workspace_bytes, void* cells, size_t cells_bytes,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!segments || !descs || num_segments < 1 || num_segments > AQLM_HIP_MAX_SEGMENTS || !x) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: 1..%d segments, their descriptors and a non-null x required (got %d)",
                   AQLM_HIP_MAX_SEGMENTS, num_segments);
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)",
                   dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (batch < 1 || batch > AQLM_HIP_MAX_GEMV_BATCH || !aligned16(x) || (batch > 1 && x_row_stride % 8 != 0)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: batch must be 1..%d with 16-B aligned rows (batch %d)",
                   AQLM_HIP_MAX_GEMV_BATCH, batch);
    return AQLM_HIP_E_INVALID;
  }
  {  // a variable-geometry segment (format v7) runs on the single-layer kernels only: one launch per segment, same bits
    bool any_vg = false;
    for (int k = 0; k < num_segments; ++k) {
      PackedLayout Lk;
      any_vg = any_vg || (descs[k] && desc_layout(descs[k], Lk) && Lk.G.vg);
    }
    if (any_vg) {
      size_t coff = 0;
      for (int k = 0; k < num_segments; ++k) {
        const aqlm_hip_segment& sg = segments[k];
        if (!descs[k] || descs[k]->in_features != in_features || descs[k]->out_features != sg.out_features) {
          set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: descriptor does not match in_features %d / out_features %d", k,
                         in_features, sg.out_features);
          return AQLM_HIP_E_INVALID;
        }
        const size_t cneed = (size_t)batch * sg.out_features * 8;
        if (cells && coff + cneed > cells_bytes) {
          set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: %zu bytes of cells required, got %zu", coff + cneed, cells_bytes);
          return AQLM_HIP_E_INVALID;
        }
        if (int e = gemv_1x16_packed_impl(descs[k], const_cast<void*>(sg.codes), sg.codebook, sg.scales, sg.bias, x, sg.y, batch, x_row_stride,
                                          sg.y_row_stride, dtype, workspace, workspace_bytes, stream_, PackedNext{},
                                          cells ? (uint8_t*)cells + coff : nullptr, cells ? cneed : 0))
          return e;
        coff += cneed;
      }
      return 0;
    }
  }
  PackedMultiParams mp{};
  PackedFinalizeMultiParams fm{};
  mp.x = (const uint16_t*)x;
  mp.x_row_stride = x_row_stride;
  mp.nseg = fm.nseg = num_segments;
  size_t need = 0;
  int fblocks = 0, max_rg = 0, nw = 0, pd = 4, eb = 0;
  bool fused = true;  // every segment must know its codebook range
  for (int k = 0; k < num_segments; ++k) fused = fused && descs[k] && packed_fused(descs[k]);
  size_t cells_need = 0;
  if (cells) {  // caller-owned accumulator cells: [segment][batch][M] u64
    if (!fused) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: every descriptor must carry the codebook range");
      return AQLM_HIP_E_INVALID;
    }
    for (int k = 0; k < num_segments; ++k) cells_need += (size_t)batch * segments[k].out_features * 8;
    if (cells_bytes < cells_need) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: %zu bytes of cells required, got %zu", cells_need, cells_bytes);
      return AQLM_HIP_E_INVALID;
    }
  }
  size_t cells_off = 0;
  for (int k = 0; k < num_segments; ++k) {
    const aqlm_hip_segment& sg = segments[k];
    if (!sg.codes || !sg.codebook || !sg.scales || !sg.y) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: null pointer in segment %d", k);
      return AQLM_HIP_E_INVALID;
    }
    PackedLayout L;
    if (!desc_layout(descs[k], L) || descs[k]->in_features != in_features || descs[k]->out_features != sg.out_features ||
        !aligned16(sg.codes) || !aligned16(sg.codebook)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: invalid descriptor, or it does not match in_features "
                     "%d / out_features %d", k, in_features, sg.out_features);
      return AQLM_HIP_E_INVALID;
    }
    const uint8_t* base = (const uint8_t*)sg.codes;
    PackedSegment& ps = mp.seg[k];
    ps.ent = (const uint32_t*)(base + L.off_ent);
    ps.winfo = (const uint32_t*)(base + L.off_winfo);
    ps.rowstart = (const uint32_t*)(base + L.off_rowstart);
    if (L.relabel && !(descs[k]->flags & AQLM_HIP_PACKED_HAS_CODEBOOK)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: a relabelled buffer needs its codebook image "
                     "(aqlm_hip_packed_set_codebook)", k);
      return AQLM_HIP_E_INVALID;
    }
    ps.codebook = L.relabel ? base + L.off_cb : (const uint8_t*)sg.codebook;
    ps.partial = fused ? nullptr : (float*)((uint8_t*)workspace + need);
    if (fused) {
      ps.acc = cells ? (unsigned long long*)((uint8_t*)cells + cells_off) : (unsigned long long*)(const_cast<uint8_t*>(base) + L.off_acc);
      cells_off += (size_t)batch * sg.out_features * 8;
      ps.scales = (const uint16_t*)sg.scales;
      ps.bias = (const uint16_t*)sg.bias;
      ps.y = (uint16_t*)sg.y;
      ps.y_row_stride = sg.y_row_stride;
      ps.cb_absmax = descs[k]->codebook_absmax;
    }
    ps.M = L.M;
    ps.RG = L.RG;
    ps.NW = L.NW;
    ps.T = L.T;
    ps.XC = L.XC;
    ps.ent_bytes = (uint32_t)L.ent_bytes;
    mp.in_groups = L.in_groups;
    if (eb && eb != L.EB) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segments mix 3- and 4-byte entry formats");
      return AQLM_HIP_E_UNSUPPORTED;
    }
    eb = L.EB;
    max_rg = std::max(max_rg, L.RG);
    nw = std::max(nw, L.NW);
    pd = std::max(pd, pick_pd(L));
    PackedFinalizeSegment& fs = fm.seg[k];
    fs.f.partial = ps.partial;
    fs.f.scales = (const uint16_t*)sg.scales;
    fs.f.bias = (const uint16_t*)sg.bias;
    fs.f.y = (uint16_t*)sg.y;
    fs.f.y_row_stride = sg.y_row_stride;
    fs.f.M = sg.out_features;
    fs.f.B = batch;
    fs.block_begin = fblocks;
    fblocks += (sg.out_features + 255) / 256;
    need += (size_t)PK_S * batch * sg.out_features * sizeof(float);
  }
  if (!fused && (!workspace || workspace_bytes < need)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: workspace of %zu bytes required, got %zu", need, workspace_bytes);
    return AQLM_HIP_E_INVALID;
  }
  if (packed_max_batch(mp.in_groups, max_rg) < batch) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: %d rows of %d features do not fit the LDS image", batch, in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  // batch 1 with the single-kernel finalize: one workgroup per CU walks all segments, slices double-buffered (pipe kernel)
  if (fused && batch == 1 && tuning().packed_pipe) {
    PackedLayout Ls[AQLM_HIP_MAX_SEGMENTS];
    for (int k = 0; k < num_segments; ++k) desc_layout(descs[k], Ls[k]);
    int prg = 0, nwc = 0, dmaw = 0;
    uint32_t xwin = PP_XWIN;
    bool oneb = false;
    if (pipe_eligible(Ls, num_segments, mp.in_groups, prg, nwc, dmaw, xwin, oneb)) {
      PipeParams pp{};
      pp.x = mp.x;
      pp.in_groups = mp.in_groups;
      pp.nseg = num_segments;
      pp.max_rg = prg;
      pp.nwc = nwc;
      pp.dma_waves = dmaw;
      pp.defer = tuning().packed_pipe == 4 ? 0 : 1;
      for (int k = 0; k < num_segments; ++k) pp.seg[k] = mp.seg[k];
      const size_t lds = pipe_lds(prg, xwin, oneb).total;
      auto go = [&](auto kern) -> int {
        if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
        hipLaunchKernelGGL(kern, dim3(PK_NST), dim3((nwc + dmaw) * 64), lds, stream, pp);
        return check_hip(hipGetLastError(), "gemv_1x16_packed_pipe launch");
      };
#define AQLM_PP_GO(SELF, XWV, OB) \
  (dtype == AQLM_HIP_F16 ? go(gemv_1x16_packed_pipe_kernel<F16, SELF, XWV, OB>) : go(gemv_1x16_packed_pipe_kernel<BF16, SELF, XWV, OB>))
      if (xwin == PP_XWIN_SMALL) {
        if (dmaw == 0) return AQLM_PP_GO(true, PP_XWIN_SMALL, false);
        return oneb ? AQLM_PP_GO(false, PP_XWIN_SMALL, true) : AQLM_PP_GO(false, PP_XWIN_SMALL, false);
      }
      if (dmaw == 0) return AQLM_PP_GO(true, PP_XWIN, false);
      return oneb ? AQLM_PP_GO(false, PP_XWIN, true) : AQLM_PP_GO(false, PP_XWIN, false);
#undef AQLM_PP_GO
    }
  }
  auto launch = [&](auto kern, auto lds_map) -> int {
    const size_t lds = decltype(lds_map)::total(mp.in_groups, max_rg);
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, dim3(PK_NST * num_segments), dim3(nw * 64), lds, stream, mp);
    return check_hip(hipGetLastError(), "gemv_1x16_packed_multi launch");
  };
  if (int e = dispatch_packed<MultiKernels>(dtype, batch, pd, eb, batch == 1 && packed_b1_slice_first(mp.in_groups, max_rg), launch)) return e;
  if (fused) return 0;
  if (dtype == AQLM_HIP_F16)
    hipLaunchKernelGGL(gemv_1x16_packed_finalize_multi<F16>, dim3(fblocks), dim3(256), 0, stream, fm);
  else
    hipLaunchKernelGGL(gemv_1x16_packed_finalize_multi<BF16>, dim3(fblocks), dim3(256), 0, stream, fm);
  return check_hip(hipGetLastError(), "gemv_1x16_packed_finalize_multi launch");
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_multi)(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                                int num_segments, const void* x, int in_features, int batch,
                                                long x_row_stride, int dtype, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
  PK_G16_FORWARD(descs && num_segments >= 1 ? descs[0] : nullptr, gemv_1x16_packed_multi, segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, workspace, workspace_bytes, stream_);
  return gemv_1x16_packed_multi_impl(segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, workspace,
                                     workspace_bytes, nullptr, 0, stream_);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_multi_cells)(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                                      int num_segments, const void* x, int in_features, int batch,
                                                      long x_row_stride, int dtype, void* cells, size_t cells_bytes,
                                                      void* stream_) {
  PK_G16_FORWARD(descs && num_segments >= 1 ? descs[0] : nullptr, gemv_1x16_packed_multi_cells, segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, cells, cells_bytes, stream_);
  if (!cells || (reinterpret_cast<uintptr_t>(cells) & 7u) || !tuning().packed_fused_finalize) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: needs 8-B aligned, zero-filled cells and the fused finalize switched on");
    return AQLM_HIP_E_INVALID;
  }
  return gemv_1x16_packed_multi_impl(segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, nullptr, 0,
                                     cells, cells_bytes, stream_);
}

// ---------------------------------------------------------------------------------------------- expert-routed launch (MoE decode)
#include "gemv_packed_routed.h"

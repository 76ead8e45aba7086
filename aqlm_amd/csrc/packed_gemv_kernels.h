// Part of gemv_packed.hip (inside namespace aqlm::PK_NS): the matvec -- parameter structs, LDS helpers and maps (PackedLds), the body
// (gemv_1x16_packed_body), its kernel wrappers (single layer, variable geometry, shared input, grouped and folded grouped) and
// the finalize kernels.  Needs packed_format.h (and group_fold.h, which aqlm_common.h brings).

struct PackedGemvParams {
  const uint32_t* ent;
  const uint32_t* winfo;
  const uint32_t* rowstart;  // [nst][RG + 1]
  const uint8_t* codebook;
  const uint16_t* x;
  float* partial;  // [S][B][M]
  long x_row_stride;
  int M, in_groups, RG, NW, T, XC;
  uint32_t ent_bytes;
  // fused finalize (acc != nullptr): the 16 slice workgroups of a row meet in ONE 64-bit cell per (input row, output row)
  unsigned long long* acc;  // [B][M], zero at rest
  float cb_absmax;          // largest |codebook entry| of the layer (bounds the slice sums)
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* y;
  long y_row_stride;
  // chain prefetch (optional): the layer that runs NEXT on this stream.  NPW extra waves of every workgroup pull the
  // next layer's stream of the same workgroup index (same XCD under the observed block % 8 placement) and a share of
  // its codebook slice towards this XCD's L2 while the other waves compute -- the next launch then starts L2-warm.
  // row-parallel shards (one-shot all-reduce over xGMI, xgmi_reduce.hip): instead of writing y, the workgroup that owns
  // a row's total PUBLISHES it -- fp32, system-scope store -- in this rank's pub buffer, and the last workgroup of the
  // launch raises the rank's flag.  nullptr: ordinary launch.
  float* pub;                    // this rank's pub[2][max_elems]
  uint32_t* pub_flag;            // this rank's flag[2]
  uint32_t* pub_epoch;           // [0] epoch, [4..11] arrival counters of the 8 workgroup shards, [12] top counter
  uint32_t pub_max_elems;
  const uint8_t* next_ent;       // entry area of the next layer's packed buffer (nullptr: no prefetch)
  const uint8_t* next_codebook;
  uint32_t next_block_bytes;     // bytes of one workgroup's stream in the next layer (NW' * T' KiB)
  int NPW;                       // prefetch waves in this launch (workgroup = NW + NPW waves)
  int fill_rotate;               // 1: workgroup g starts its slice fill at piece g * (pieces / row groups)
#ifdef AQLM_PACKED_TRACE
  unsigned long long* trace;  // [256 workgroups][8] wall-clock stamps (100 MHz), profiling builds only
  int dbg;                    // bit 0: skip the LDS reads + dot products, bit 1: no entry stream (out-of-range loads)
#endif
};

typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef __attribute__((address_space(3))) const u32x4* lds_u32x4_ptr;
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef __attribute__((address_space(1))) const void* gbl_void_ptr;
typedef const uint32_t __attribute__((address_space(4)))* const_u32_ptr;  // constant address space: uniform loads go through s_load

template <int WORD>
__device__ __forceinline__ uint32_t half_and(uint32_t w, uint32_t mask) {
  uint32_t d;  // d = ((w >> 16*WORD) & 0xffff) & mask in one instruction (sub-dword operand select)
  if constexpr (WORD == 0)
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(d) : "v"(mask), "v"(w));
  else
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(d) : "v"(mask), "v"(w));
  return d;
}

__device__ __forceinline__ void lds_store_f32(uint32_t byte_addr, float v) {
  asm volatile("ds_write_b32 %0, %1" : : "v"(byte_addr), "v"(v) : "memory");
}
// LDS reads hipcc does not see (pipelined kernel's epilogue): while LDS-DMA requests are in flight the compiler guards every
// LDS read it knows of with vmcnt(0) -- it cannot tell which addresses the DMA writes.  The caller waits (lds_asm_wait)
// before it uses the values.
__device__ __forceinline__ uint32_t lds_asm_load_b32(uint32_t byte_addr) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(byte_addr));  // no "memory" clobber: with one hipcc treats the asm as a possible LDS reader and puts vmcnt(0) in front
  return v;
}
__device__ __forceinline__ u32x4 lds_asm_load_b128(uint32_t byte_addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}
// the wait names the registers it guards ("+v"): a bare `s_waitcnt` asm orders nothing for the compiler's scheduler, which
// is free to move a USE of an asm-loaded value in front of it (it happened: wrong row sums in one build, right ones in the next)
__device__ __forceinline__ void lds_asm_wait(uint32_t& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)); }
__device__ __forceinline__ void lds_asm_wait(uint32_t& a, uint32_t& b, uint32_t& c, u32x4& d0, u32x4& d1, u32x4& d2, u32x4& d3) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));
}

// LDS map (byte offsets from the start of the workgroup's LDS, which is address 0: the kernel has no static LDS).
//   B == 1: x at 0 (XWIN bytes reserved), slice at XWIN, bookkeeping behind the slice   (x-first: both reads cost one op)
//           XWIN = PK_XWIN_FULL (65520): any x the format allows; image 135-140 KiB, one workgroup per CU
//           XWIN = PK_XWIN_COMPACT (8208): x of <= 4096 features; with the bookkeeping sized by the launch (TIGHT) the image is
//           76-83 KiB, so a workgroup of ANOTHER layer fits the CU beside it (4096->4096 + 4096->11008: 160 640 of 163 840 bytes)
//           XWIN = 0: slice first, as for B > 1 (layers whose row tables do not fit behind a window)
//   B  > 1: slice at 0, then B planes x[b][j] of XP = (in_groups + 1) * 16 bytes (a plane keeps the bank pattern of
//           the single-row case: slot j -> bank group j % 16; interleaving the rows would leave 16 / B groups), bookkeeping
//   bookkeeping: rowstart[RG + 1] u32 (LDS-DMA copy of the stream's row starts), rowval[B][RG + 1] f32 (sum of the
//   lane-steps of a row from the start of the column that holds its LAST lane-step), colend[B][16 * 64] f32 (what a
//   column accumulated after its last row end: the head of a row that continues in the next column)
template <int B, uint32_t XWIN>
struct PackedLds {
  static constexpr bool XFIRST = (B == 1) && AQLM_PK_XFIRST && XWIN != 0u;  // XWIN == 0: slice first also for one row (tall layers)
  static constexpr uint32_t SLICE = XFIRST ? XWIN : 0u;
  static constexpr uint32_t X = XFIRST ? 0u : PK_SLICE_BYTES;
  __host__ __device__ static uint32_t plane(int in_groups) { return (uint32_t)(in_groups + 1) * PK_VB; }
  __host__ __device__ static uint32_t rowstart(int in_groups) {
    return XFIRST ? XWIN + PK_SLICE_BYTES : PK_SLICE_BYTES + plane(in_groups) * B;
  }
  // TIGHT (the compact window): the image is meant to share the CU with another layer's, so the bookkeeping is sized by what
  // the launch uses -- the row-start table in the 256-byte pieces its dword DMA is issued in (a piece's lanes are guarded by
  // idx < RG + 1), colend for the `nw` waves of the stream (columns >= nw * 64 are neither written nor read) -- not by the
  // worst case.  Every other image ignores `nw` and keeps the map it had.
  static constexpr bool TIGHT = XFIRST && XWIN < PK_XWIN_FULL;
  __host__ __device__ static uint32_t rs_bytes(int RG) {  // whole DMA pieces
    return TIGHT ? ((uint32_t)(RG + 1) * 4u + 255u) & ~255u : ((uint32_t)(RG + 1) * 4u + 1023u) & ~1023u;
  }
  __host__ __device__ static uint32_t rowval(int in_groups, int RG) { return rowstart(in_groups) + rs_bytes(RG); }
  __host__ __device__ static uint32_t colend(int in_groups, int RG) { return rowval(in_groups, RG) + (uint32_t)B * (RG + 1) * 4u; }
  __host__ __device__ static uint32_t xmax(int in_groups, int RG, int nw) {  // 16-B aligned: read with ds_read_b128
    return (colend(in_groups, RG) + (uint32_t)B * (TIGHT ? (uint32_t)nw : (uint32_t)PK_MAX_NW) * 64 * 4 + 15u) & ~15u;
  }
  __host__ __device__ static uint32_t dump(int in_groups, int RG, int nw) {  // 1 KiB landing zone per prefetch wave (LDS-DMA needs a destination)
    return (xmax(in_groups, RG, nw) + (uint32_t)B * PK_MAX_NW * 4u + 15u) & ~15u;
  }
  // nw: the waves of the stream (PackedLayout::NW; for the multi launch, whose images are never TIGHT, any value)
  __host__ __device__ static size_t total(int in_groups, int RG, int npw = 0, int nw = PK_MAX_NW) {
    return npw ? (size_t)dump(in_groups, RG, nw) + (size_t)npw * 1024
               : (size_t)xmax(in_groups, RG, nw) + (size_t)B * PK_MAX_NW * 4;  // xmax[B][16 waves] u32: largest |x| seen by each wave (fused finalize)
  }
};

// `block` in [0, 256): the workgroup's index within its own layer (== blockIdx.x for a single-layer launch).
// PUB: the row-parallel shard's variant (the last arrival publishes the fp32 total for the peers instead of writing y).  A
// template parameter, not a run-time test of p.pub: carrying the publish branches in the ordinary kernel cost 0.15 us per
// launch (same box, profiles/r03_mb_ab_commits.log).
// VG: variable geometry (format v7): `ns` = the first stream of each of the 16 slices, one byte each; the workgroup finds its
// slice, row range and stream from them with a handful of instructions (no table in memory: a dependent load in front of the
// slice fill would cost more than the imbalance it repairs).
struct PackedVgArgs {
  uint32_t ns[4];
};

// NOPF: the launch has no prefetch waves (p.NPW == 0 by construction: the expert-routed launch) -- their branches go away at
// compile time.  (A run-time p.NPW == 0 leaves them in, and with them a path on which hipcc sees the LDS-DMA still in flight.)
// FOLD: the folded grouped launch (gemv_1x16_packed_group_fold_kernel).  The workgroup fills slice, x and the null slots ONCE and
// then walks `npass` streams of its slice in turn -- `block` is the stream of pass 0, pass j runs row group
// block / 16 + j * group_step -- each pass with its own entry ring, loop, row tables, scale / bias prefetch and epilogue (same
// cell protocol, same summation order, same bits in y as a workgroup of its own).  rowval / colend are reused from pass to pass
// behind a barrier; no LDS-DMA is issued after the first fill barrier (hipcc would guard every LDS read it sees with vmcnt(0)
// and drain the ring: packed_pipe_kernel.h), so the row starts of a pass come by ordinary loads like scale and bias, and the
// row-start area of the image stays unused.  Every FOLD branch is `if constexpr`: the other instances compile to what they were.
template <class T_, int B, int PD, uint32_t XWIN, int EB, bool PUB = false, bool VG = false, bool NOPF = false, bool FOLD = false>
__device__ __forceinline__ void gemv_1x16_packed_body(const PackedGemvParams& p, const int block, const int NWB,
                                                      const PackedVgArgs& vg = PackedVgArgs{}, const int npass = 1,
                                                      const int group_step = 0) {
  static_assert(!FOLD || (B == 1 && EB == 4 && !PUB && !VG && NOPF), "folded launch: one row, 4-byte entries, ordinary geometry");
  using LDS = PackedLds<B, XWIN>;
  using ring_t = typename std::conditional<EB == 3, u32x3, u32x4>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int NT = NWB << 6;  // NWB = waves in the workgroup (>= p.NW); passed in: blockDim lives in the hidden kernel arguments
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef AQLM_PACKED_TRACE
  unsigned long long tr[8];
  uint32_t tr_wait = 0, tr_work = 0;
  tr[0] = wall_clock64();
  const unsigned long long cyc0 = __builtin_readcyclecounter();  // s_memtime: shader clock
#define AQLM_TRACE(i) tr[i] = wall_clock64()
#else
#define AQLM_TRACE(i)
#endif
  // slice = block % 16: blocks are observed to land on XCD block % 8, so each XCD's L2 serves two 64 KiB slices
  // (speed only; any placement is correct).
  int slice, group, row_begin, nrows, stream_ix;
  if constexpr (VG) {
    static_assert(PK_S == 16 && PK_NST == 256, "variable geometry: 16 slices, 256 workgroups");
    // workgroups land on XCD block % 8: XCD x serves streams [32 x, 32 x + 32) -- consecutive streams share their slice
    stream_ix = ((block & 7) << 5) | (block >> 3);
    // ns = the first stream of slices 0..15, one byte each (slice 0 starts at 0, the last slice ends at 256).  Lane i < 16
    // looks at slice i: the slices that start at or before this stream answer the ballot, the last of them owns it.
    // (A scalar walk over the 16 bytes was ~280 dependent instructions in front of the first load: 0.5 us.)
    const uint32_t w = lane < 4 ? vg.ns[0] : (lane < 8 ? vg.ns[1] : (lane < 12 ? vg.ns[2] : vg.ns[3]));
    const uint32_t start_v = (w >> ((lane & 3) * 8)) & 255u;
    const unsigned long long m = __ballot((uint32_t)stream_ix >= start_v) & 0xffffull;
    const int s = __popcll(m) - 1;
    const int start = __builtin_amdgcn_readlane((int)start_v, s);
    const int end = s == PK_S - 1 ? PK_NST : __builtin_amdgcn_readlane((int)start_v, s < PK_S - 1 ? s + 1 : s);
    int n = end - start;
    n = n < 1 ? 1 : n;
    slice = s;
    group = stream_ix - start;
    const int base = p.M / n, extra = p.M - base * n;
    row_begin = group * base + (group < extra ? group : extra);
    nrows = base + (group < extra ? 1 : 0);
  } else {
    stream_ix = block;
    slice = block & (PK_S - 1);
    group = block >> PK_S_LOG;
    row_begin = group * p.RG;
    nrows = p.M - row_begin;
    nrows = nrows < 0 ? 0 : (nrows < p.RG ? nrows : p.RG);
  }
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_raw != 0u) __builtin_trap();  // LDS map above

  const int RG1 = p.RG + 1;
  const uint32_t rowstart_off = LDS::rowstart(p.in_groups);
  const uint32_t rowval_off = LDS::rowval(p.in_groups, p.RG);
  const uint32_t colend_off = LDS::colend(p.in_groups, p.RG);

  // ---- prologue: everything that needs no other data is issued first, in one burst -------------------------------
  const uint32_t XP = LDS::plane(p.in_groups);
  const uint32_t xstride16 = (uint32_t)pk_x_stride(p.in_groups) * PK_VB;
  __amdgpu_buffer_rsrc_t rs_ent = __builtin_amdgcn_make_buffer_rsrc((void*)p.ent, 0, p.ent_bytes, 0x00020000);
  const int wv = wave < p.NW ? wave : p.NW - 1;  // waves beyond the stream's wave count (shared-input launches) idle
  const uint32_t wbase = (uint32_t)(((size_t)stream_ix * p.NW + wv) * p.T) * (EB == 3 ? (uint32_t)PK_WREG3 : 1024u);
  int Tm1 = p.T - 1;  // (FOLD: -1 while the ring of a pass that does not exist is requested)
  // (0) 3-byte entries: the row-end flag words of this wave range, word t in lane t -- the OLDEST load of the queue, so
  // it has landed whenever the wait of (5) returns
  u32x2 flagw = {0u, 0u};
  if constexpr (EB == 3)
    flagw = __builtin_amdgcn_raw_buffer_load_b64(rs_ent, (uint32_t)(lane < Tm1 ? lane : Tm1) * 8u, wbase, 0);
  // Chain prefetch: the last p.NPW waves of the workgroup take no part in the fill or the loop.  They ask for the NEXT
  // layer's bytes (LDS-DMA into a 1 KiB dump zone each: no registers, nothing to wait for before the fill barrier) and
  // meet the others at the barriers.
  const int NWD = NWB - p.NPW;  // waves that fill and compute
  const bool pfw = !NOPF && wave >= NWD;
  if (pfw) {
    const int pw = wave - NWD;
    const uint32_t dump = LDS::dump(p.in_groups, p.RG, p.NW) + (uint32_t)pw * 1024u;
    const uint8_t* nsrc = p.next_ent + (size_t)block * p.next_block_bytes;
    for (uint32_t off = (uint32_t)pw * 1024u; off < p.next_block_bytes; off += (uint32_t)p.NPW * 1024u)
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)(nsrc + off + lane * 16), (lds_void_ptr)(size_t)dump, 16, 0, AUX_NT);
    constexpr uint32_t SHARE = PK_SLICE_BYTES / PK_NG;  // the PK_NG workgroups of a slice split its next-layer image
    const uint8_t* csrc = p.next_codebook + (size_t)slice * PK_SLICE_BYTES + (size_t)group * SHARE;
    for (uint32_t off = (uint32_t)pw * 1024u; off < SHARE; off += (uint32_t)p.NPW * 1024u)
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)(csrc + off + lane * 16), (lds_void_ptr)(size_t)dump, 16, 0, 0);
  }
  // (1) LDS-DMA: the 64 KiB slice (shared by the 16 workgroups of the XCD that hold it -> L2 hits) and x
  if (!pfw) {
    const uint8_t* src = p.codebook + (size_t)slice * PK_SLICE_BYTES;
    // rotated start: the PK_NG workgroups that fill the same slice from the same L2 walk it from different pieces, so at
    // any moment they ask different L2 channels (and, cold, each pulls a different part from HBM first)
    constexpr int PIECES = (int)(PK_SLICE_BYTES / 1024);
    const int rot = p.fill_rotate ? (group & (PK_NG - 1)) * (PIECES / PK_NG) : 0;
    for (int i0 = wave; i0 < PIECES; i0 += NWD) {
      const int i = (i0 + rot) & (PIECES - 1);
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)(src + i * 1024 + lane * 16),
                                       (lds_void_ptr)(size_t)(LDS::SLICE + (uint32_t)i * 1024u), 16, 0, 0);
    }
    const int x16 = p.in_groups * (int)(PK_VB / 16);  // 16-byte units of a row of x
    const int nchunk = (x16 + 63) >> 6;              // KiB pieces per row of x
    // B == 1: XC rotated copies of the row (copy c at slot c * xstride); B > 1: one plane per row
    const int ncopy = B == 1 ? p.XC : B;
    for (int c = wave; c < nchunk * ncopy; c += NWD) {
      const int b = c / nchunk, i = c - b * nchunk;
      const int idx = i * 64 + lane;
      const uint32_t dst = LDS::X + (uint32_t)b * (B == 1 ? xstride16 : XP) + (uint32_t)i * 1024u;
      if (idx < x16)
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(p.x + (B == 1 ? (size_t)0 : (size_t)b * p.x_row_stride) + (size_t)idx * 8),
                                         (lds_void_ptr)(size_t)dst, 16, 0, 0);
    }
    // the stream's row starts (needed by the epilogue only; as an LDS-DMA they are older than the ring loads, see (5)).
    // Rows of the table are only 4-B aligned -> dword DMA, 256 B per wave-instruction.
    // (FOLD: every pass fetches the two row starts of its thread's row into registers, below)
    if constexpr (!FOLD) {
      const uint32_t* rs_src = p.rowstart + (size_t)stream_ix * RG1;
      for (int i = wave; i * 64 < RG1; i += NWD) {
        const int idx = i * 64 + lane;
        if (idx < RG1)
          __builtin_amdgcn_global_load_lds((gbl_void_ptr)(rs_src + idx), (lds_void_ptr)(size_t)(rowstart_off + (uint32_t)i * 256u), 4, 0, 0);
      }
    }
  }
  // (2) the entry stream of this wave: fixed addresses, PD steps ahead in a register ring with compile-time slots
  const uint32_t voff = (uint32_t)lane * (EB == 3 ? 12u : 16u);
  uint32_t ebase = EB == 3 ? wbase + (uint32_t)p.T * 8u : wbase;  // (FOLD: of the pass whose ring is requested)
  auto fetch = [&](int t) -> ring_t {  // unconditional (a load under a branch derails hipcc's wait counts); steps past the
    // end of the range get an out-of-range offset: the buffer unit answers them with zeros and touches no memory
#ifdef AQLM_PACKED_TRACE
    const uint32_t vo = (t <= Tm1 && !(p.dbg & 2)) ? voff : 0xfffffff0u;
#else
    const uint32_t vo = t <= Tm1 ? voff : 0xfffffff0u;
#endif
    if constexpr (EB == 3) return __builtin_amdgcn_raw_buffer_load_b96(rs_ent, vo, ebase + (uint32_t)t * (uint32_t)PK_STEP3, AUX_NT);
    else return __builtin_amdgcn_raw_buffer_load_b128(rs_ent, vo, ebase + (uint32_t)t * 1024u, AUX_NT);
  };
  ring_t ring[PD];
#pragma unroll
  for (int k = 0; k < PD; ++k) ring[k] = fetch(pfw ? 0x7fffffff : k);  // prefetch waves: out-of-range requests (zeros, no memory traffic)
  // (3) steps of this wave through the scalar cache (not a VMEM op: it must not sit in the vmcnt queue, see (5))
  // 4-byte entries need neither: the start rows ride in the entries, and every wave range runs all T steps (the tail of a
  // stream is padded with null entries up to T steps -- the workgroup waits for its full ranges anyway)
  int steps = wave < p.NW ? p.T : 0;
  [[maybe_unused]] uint32_t wave_start_row = 0u;
  if constexpr (EB == 3) {
    const const_u32_ptr wi = (const_u32_ptr)(uintptr_t)(p.winfo + ((size_t)stream_ix * p.NW + wv) * 4);
    steps = wave < p.NW ? (int)wi[2] : 0;
    wave_start_row = wi[3];
  }
  // (4) LDS that needs no data: the zero vectors the null entries point at
  if (tid < B * (int)(PK_VB / 16))  // the null entries' x: PK_VB zero bytes per row of x
    *reinterpret_cast<u32x4*>(smem_raw + LDS::X + (uint32_t)(tid / (int)(PK_VB / 16)) * XP + (uint32_t)p.in_groups * PK_VB +
                              (uint32_t)(tid % (int)(PK_VB / 16)) * 16u) = u32x4{0u, 0u, 0u, 0u};
  const uint32_t xmax_off = LDS::xmax(p.in_groups, p.RG, p.NW);
  if (tid < B * PK_MAX_NW) *reinterpret_cast<uint32_t*>(smem_raw + xmax_off + (uint32_t)tid * 4u) = 0u;  // slots of absent waves
  AQLM_TRACE(1);  // every load of the prologue has been issued
  // (5) the slice and x are older in the VMEM queue than the PD ring loads: wait for everything BUT the ring, so the
  // stream keeps flowing while the loop starts (a __syncthreads() here would emit vmcnt(0) and drain it)
  // (the builtin, not an asm string: hipcc's wait-count pass must learn that the LDS-DMA ops have retired, or it guards
  // the first use of the ring with vmcnt(0))
  // the parameters of the epilogue (the non-preloaded tail of the kernel arguments) are fetched NOW, under the LDS fill:
  // left to the compiler their s_load sits at the first use, behind the loop, with its whole latency exposed (0.3 us)
  asm volatile("" : : "s"(p.acc), "s"(p.partial), "s"(p.scales), "s"(p.bias), "s"(p.y), "s"(p.y_row_stride), "s"(p.cb_absmax));
  // ... and so are scale and bias of the row this thread finalizes (cold they are an HBM round trip: requested behind the
  // last-arrival test they sat at the very end of the kernel's critical path).  Unconditional, always-valid addresses
  // (a branch around a load ends in a vmcnt(0) at the join); younger than the ring, so the wait below lets them fly too.
  uint16_t scale_h, bias_h;
  [[maybe_unused]] uint32_t q0_h = 0u, q1_h = 0u;  // FOLD: the row starts of this thread's first row (rs[r], rs[r + 1])
  // FOLD: what a pass requests for its thread's first row -- scale, bias and the two row starts of row `tid` of row group `g`,
  // clamped to addresses that exist when the group is short or empty (the table of a stream has RG + 1 words)
  [[maybe_unused]] auto pass_loads = [&](int g, uint16_t& sc, uint16_t& bi, uint32_t& q0, uint32_t& q1) {
    const int rb = g * p.RG;
    int n = p.M - rb;
    n = n < 0 ? 0 : (n < p.RG ? n : p.RG);
    const int r = tid < n ? tid : (n > 0 ? n - 1 : 0);
    const int row = rb + r < p.M ? rb + r : p.M - 1;
    const uint16_t* bp = p.bias ? p.bias : p.scales;
    const uint32_t* rs_g = p.rowstart + (size_t)(g * PK_S + slice) * RG1;
    sc = p.scales[row];
    bi = bp[row];
    // rs[r] and rs[r + 1] as ONE 8-byte load of 4-byte alignment (hipcc fuses two dword loads into it anyway): the fill wait
    // below counts loads, so their number is fixed here and not left to the optimiser
    typedef uint32_t rs_pair __attribute__((ext_vector_type(2), aligned(4)));
    const rs_pair q = *reinterpret_cast<const rs_pair*>(rs_g + r);
    q0 = q.x;
    q1 = q.y;
  };
  if constexpr (FOLD) {
    pass_loads(group, scale_h, bias_h, q0_h, q1_h);
  } else {
    const int r = tid < nrows ? tid : (nrows > 0 ? nrows - 1 : 0);
    const uint16_t* sp = p.scales ? p.scales : reinterpret_cast<const uint16_t*>(p.rowstart);  // partials mode: unused
    const uint16_t* bp = p.bias ? p.bias : sp;
    scale_h = sp[row_begin + r];
    bias_h = bp[row_begin + r];
  }
  constexpr int PDW = PD + (FOLD ? 3 : 2);  // behind the last LDS-DMA: the ring, scale, bias (FOLD: and the row-start pair)
  if (!pfw) __builtin_amdgcn_s_waitcnt((PDW & 15) | (7 << 4) | (0 << 8) | ((PDW >> 4) << 14));  // vmcnt(PD + 2) lgkmcnt(0) (FOLD: PD + 3)
  else __builtin_amdgcn_s_waitcnt(63 | (7 << 4) | (0 << 8) | (3 << 14));                          // prefetch waves: lgkmcnt(0) only
  __builtin_amdgcn_s_barrier();
  AQLM_TRACE(2);

  uint32_t mask = PK_HMASK;
  asm volatile("" : "+v"(mask));  // the SDWA operand must sit in a VGPR
  // One accumulator chain per row of x for every batch size: a row's result must not depend on how many rows share the
  // launch (tested bit for bit).  Several independent chains per row were measured: no gain (the loop is not bound by
  // the dependent latency of v_dot2c).
  constexpr int NA = 1;
  float acc[B][NA];
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[b][a] = 0.f;
  uint32_t row_addr = 0;  // LDS byte address of rowval[0][current row of this column]

  // One lane-step = 4 entries.  Per entry: a_cb / a_x = LDS byte offsets of the codebook vector (inside the slice) and of
  // x[j] (inside the x area; for B > 1 `copy` is the x copy the entry names -- the planes hold one, so its offset is
  // taken out again).  ALL LDS reads of a group of entries are issued before the first dot product: with 2 waves per SIMD
  // the loop is bound by LDS latency, not bandwidth (traced: 0.3 us per step with two entries in flight per wave).
  constexpr int NV = (int)(PK_VB / 16);  // 16-byte reads per vector: 1 (8 elements) or 2 (16 elements)
  constexpr int EG0 = B <= 2 ? 4 : (B <= 4 ? 2 : 1);
  constexpr int EG = NV > 1 && EG0 > 1 && B > 1 ? EG0 / 2 : EG0;  // entries per read batch (registers: EG * NV * (1 + B) * 4)
  auto entries = [&](const uint32_t (&a_cb)[4], const uint32_t (&a_x)[4], const uint32_t (&copy)[4]) {
#ifdef AQLM_PACKED_TRACE
    if (p.dbg & 1) { acc[0][0] += __uint_as_float(a_cb[0] ^ a_x[1] ^ a_cb[2] ^ a_x[3]); return; }
#endif
#pragma unroll
    for (int g0 = 0; g0 < 4; g0 += EG) {
      u32x4 ev[EG][NV], xv[EG][B][NV];
#ifdef AQLM_PACKED_TRACE
      if (p.dbg & 8) {  // no LDS reads: the dot products run on register garbage (what does the VALU part cost alone?)
#pragma unroll
        for (int k = 0; k < EG; ++k)
#pragma unroll
          for (int h = 0; h < NV; ++h) {
            ev[k][h] = u32x4{a_cb[g0 + k], a_x[g0 + k], a_cb[g0 + k] ^ 0x3c00u, a_x[g0 + k] ^ 0x3c00u};
#pragma unroll
            for (int b = 0; b < B; ++b) xv[k][b][h] = u32x4{a_x[g0 + k], a_cb[g0 + k], a_x[g0 + k] ^ 0x3c00u, a_cb[g0 + k]};
          }
      } else
#endif
#pragma unroll
      for (int k = 0; k < EG; ++k) {
#pragma unroll
        for (int h = 0; h < NV; ++h) ev[k][h] = *(lds_u32x4_ptr)(size_t)((a_cb[g0 + k] ^ ((uint32_t)h * 16u)) + LDS::SLICE);
        if constexpr (B == 1) {
#pragma unroll
          for (int h = 0; h < NV; ++h) xv[k][0][h] = *(lds_u32x4_ptr)(size_t)((a_x[g0 + k] ^ ((uint32_t)h * 16u)) + LDS::X);
        } else {
#pragma unroll
          for (int h = 0; h < NV; ++h) {
            const uint32_t ax = (a_x[g0 + k] ^ ((uint32_t)h * 16u)) + LDS::X - copy[g0 + k] * xstride16;
#pragma unroll
            for (int b = 0; b < B; ++b) xv[k][b][h] = *(lds_u32x4_ptr)(size_t)(ax + (uint32_t)b * XP);
          }
        }
      }
#ifdef AQLM_PACKED_TRACE
      if (p.dbg & 4) {  // LDS reads but no dot products: one op per entry keeps the reads alive
#pragma unroll
        for (int k = 0; k < EG; ++k) acc[0][0] += __uint_as_float((ev[k][NV - 1].x ^ xv[k][0][NV - 1].w) & 0x007fffffu);
        continue;
      }
#endif
#pragma unroll
      for (int k = 0; k < EG; ++k)
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
          for (int h = 0; h < NV; ++h) acc[b][(g0 + k) % NA] = dot8<T_>(ev[k][h], xv[k][b][h], acc[b][(g0 + k) % NA]);
    }
  };
  auto total = [&](int b) -> float {  // fixed summation order of the chains
    float v = acc[b][0];
#pragma unroll
    for (int a = 1; a < NA; ++a) v += acc[b][a];
    return v;
  };
  auto flush = [&]() {  // a row ends here: exactly one lane-step per row does, so the store has a unique writer
#pragma unroll
    for (int b = 0; b < B; ++b) {
      lds_store_f32(row_addr + (uint32_t)(b * RG1) * 4u, total(b));
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[b][a] = 0.f;
    }
    row_addr += 4u;
  };
  uint32_t cmask = 0u;  // 3-byte entries: bit t = this column's lane-step t ends a row
  [[maybe_unused]] uint32_t xrecip = 0u;
  if constexpr (EB == 3 && B > 1) xrecip = 0xffffffffu / (xstride16 >> 4) + 1u;  // slot / stride == mulhi(slot, xrecip) for slot < 2^16
  auto step = [&](const ring_t& e) {
    uint32_t a_cb[4], a_x[4], copy[4] = {0u, 0u, 0u, 0u};
    if constexpr (EB == 4) {
      const uint32_t w[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a_cb[k] = half_and<0>(w[k], mask);  // (plain v_and / v_lshrrev instead of the two SDWA ops: measured, no change)
        a_x[k] = half_and<1>(w[k], mask);
        if constexpr (B > 1) copy[k] = (w[k] >> 16) & 3u;
      }
      entries(a_cb, a_x, copy);
      if (e.x & 1u) flush();
    } else {
      // 96 bits = 4 x (slot:12 | code:12), entry k at bit 24 k
      const uint32_t w0 = e.x, w1 = e.y, w2 = e.z;
      const uint32_t t1 = __builtin_amdgcn_alignbit(w1, w0, 24);   // bits 24.. : code 1 in [11:0]
      const uint32_t t2 = __builtin_amdgcn_alignbit(w2, w1, 28);   // bits 60.. : slot 2 in [11:0]
      a_cb[0] = (w0 << 4) & 0xfff0u;   a_x[0] = (w0 >> 8) & 0xfff0u;
      a_cb[1] = (t1 << 4) & 0xfff0u;   a_x[1] = w1 & 0xfff0u;
      a_cb[2] = (w1 >> 12) & 0xfff0u;  a_x[2] = (t2 << 4) & 0xfff0u;
      a_cb[3] = (w2 >> 4) & 0xfff0u;   a_x[3] = half_and<1>(w2, mask);
      if constexpr (B > 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) copy[k] = __umulhi(a_x[k] >> 4, xrecip);
      }
      entries(a_cb, a_x, copy);
      if (cmask & 1u) flush();
      cmask >>= 1;
    }
  };

  // FOLD: pass j of the workgroup starts here -- ring, scale_h / bias_h / q0_h / q1_h and the row range are those of its stream,
  // acc and row_addr are zero, and every wave has left epilogue j - 1 (its reads of rowval / colend).  A backward goto and not a
  // loop around 180 lines: the body of the other instances stays the text (and the instructions) it was.
  [[maybe_unused]] int pass = 0;
next_pass:
  if (steps > 0) {
    if constexpr (EB == 4) {  // the column's starting row rides in the spare bits of its first lane-step
      const uint32_t f = pk_get_start_row(ring[0].x, ring[0].y, ring[0].z, ring[0].w);
      row_addr = rowval_off + f * 4u;
    } else {  // flag word t sits in lane t: collect this lane's bit of every word, and count the row ends of the columns before it
      uint32_t pre = 0u;
      const uint32_t l31 = (uint32_t)lane & 31u;
      for (int t = 0; t < steps; ++t) {
        const uint32_t slo = (uint32_t)__builtin_amdgcn_readlane((int)flagw.x, t), shi = (uint32_t)__builtin_amdgcn_readlane((int)flagw.y, t);
        const uint32_t sel = lane >= 32 ? shi : slo;
        cmask |= ((sel >> l31) & 1u) << t;
        pre = __builtin_amdgcn_mbcnt_hi(shi, __builtin_amdgcn_mbcnt_lo(slo, pre));
      }
      row_addr = rowval_off + (wave_start_row + pre) * 4u;
    }
    int t = 0;
    for (; t + PD <= steps; t += PD) {
#pragma unroll
      for (int k = 0; k < PD; ++k) {  // single back-edge, static ring slots: no in-flight register is ever copied
#ifdef AQLM_PACKED_TRACE
        // profiling build: split a step into "waiting for its entries" and "LDS reads + dot products" (shader cycles)
        const unsigned long long c0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_waitcnt(((PD - 1) & 15) | (7 << 4) | (15 << 8));
        const unsigned long long c1 = __builtin_amdgcn_s_memtime();
        step(ring[k]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long c2 = __builtin_amdgcn_s_memtime();
        tr_wait += (uint32_t)(c1 - c0);
        tr_work += (uint32_t)(c2 - c1);
#else
        step(ring[k]);                 // the slot's words are dead once their addresses are formed ...
#endif
        ring[k] = fetch(t + PD + k);   // ... so the refill lands in the same registers (no copy at the back-edge)
      }
    }
    const int rem = steps - t;
#pragma unroll
    for (int k = 0; k < PD - 1; ++k)
      if (k < rem) step(ring[k]);
  }
  // Fused finalize: the largest |x| of every input row, as the 15-bit magnitude pattern of the storage type (integer
  // order == magnitude order; a NaN compares above Inf, so it surfaces).  x sits in LDS and every workgroup of the layer
  // sees the same x, so all of them derive the same fixed-point scale from it in the epilogue.  Done AFTER the loop: the
  // waves finish it at different times (the SIMDs favour their older waves), so for most of them this is idle time, and
  // right behind the fill barrier it would stand between every wave and its first lane-step (measured: 0.35 us).
  // (FOLD: x stays, so once, behind the loop of pass 0)
  if (p.acc != nullptr && (!FOLD || pass == 0)) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int b = 0; b < B; ++b) {
      us2 m = {0, 0};
      for (int idx = tid; idx < p.in_groups * (int)(PK_VB / 16); idx += NT) {
        const u32x4 v = *(lds_u32x4_ptr)(size_t)(LDS::X + (uint32_t)b * (B == 1 ? 0u : XP) + (uint32_t)idx * 16u);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) m = __builtin_elementwise_max(m, __builtin_bit_cast(us2, w[k] & 0x7fff7fffu));
      }
      // wave maximum on the VALU (DPP), one slot per wave: no LDS atomics, no shuffle round trips on the way to the loop
      const uint32_t mm = wave_max_u32(m.x > m.y ? (uint32_t)m.x : (uint32_t)m.y);
      if (lane == 0) *reinterpret_cast<uint32_t*>(smem_raw + xmax_off + (uint32_t)(b * PK_MAX_NW + wave) * 4u) = mm;
    }
  }

  // what the column gathered after its last row end belongs to a row that continues in the next column (0 otherwise)
  if (wave < p.NW) {
#pragma unroll
    for (int b = 0; b < B; ++b) lds_store_f32(colend_off + (uint32_t)((b * PK_MAX_NW + wave) * 64 + lane) * 4u, total(b));
  }
  AQLM_TRACE(4);
  asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");  // the asm LDS stores above are invisible to the compiler's counters
  __syncthreads();
  AQLM_TRACE(5);
  // FOLD: what pass j + 1 needs first is requested HERE, in front of epilogue j, so the epilogue's atomic round trip runs under
  // it: scale, bias and row starts of the thread's row, then the first PD ring steps (the ring's registers are dead: the loop is
  // over).  Unconditional; behind the last pass the small loads repeat this pass's addresses and the ring steps are out of
  // range (zeros, no memory traffic).  Nothing here is an LDS-DMA, so hipcc puts no vmcnt(0) in front of the epilogue's LDS reads.
  [[maybe_unused]] uint16_t scale_n = 0, bias_n = 0;
  [[maybe_unused]] uint32_t q0_n = 0u, q1_n = 0u;
  if constexpr (FOLD) {
    const bool more = pass + 1 < npass;
    const int g = more ? group + group_step : group;
    pass_loads(g, scale_n, bias_n, q0_n, q1_n);
    ebase = (uint32_t)(((size_t)(g * PK_S + slice) * p.NW + wv) * p.T) * 1024u;
    Tm1 = more ? p.T - 1 : -1;
#pragma unroll
    for (int k = 0; k < PD; ++k) ring[k] = fetch(k);
  }
  // ---- epilogue: row r = rowval[r] + the column remainders of the columns it crosses, in column order -------------
  float* pub_half = nullptr;
  uint32_t pub_e = 0u;
  if (PUB && p.pub != nullptr && p.acc != nullptr) {  // row-parallel shard: publish instead of writing y (epoch parity picks the half)
    pub_e = __hip_atomic_load(p.pub_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pub_half = p.pub + (size_t)(pub_e & 1u) * p.pub_max_elems;
  }
  {
    const uint32_t* rs = reinterpret_cast<const uint32_t*>(smem_raw + rowstart_off);
    const float* rowval = reinterpret_cast<const float*>(smem_raw + rowval_off);
    const float* colend = reinterpret_cast<const float*>(smem_raw + colend_off);
    const uint32_t T = (uint32_t)p.T;
    for (int r = tid; r < nrows; r += NT) {
      uint32_t q0, q1;
      if constexpr (FOLD) {  // requested a loop ago.  The launch code folds only layers with RG <= the block size, so r == tid:
        q0 = q0_h;           // a load for a further row here would be waited for with vmcnt(0), the next pass's ring in front
        q1 = q1_h;           // of it, before this row's atomic could go out
      } else {
        q0 = rs[r];
        q1 = rs[r + 1];
      }
      const uint32_t c0 = q0 / T, c1 = (q1 - 1u) / T;  // first / last column the row touches (column = wave * 64 + lane)
      float v[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        v[b] = rowval[b * RG1 + r];
        for (uint32_t c = c0; c < c1; ++c) v[b] += colend[(size_t)b * PK_MAX_NW * 64 + c];
      }
      if (p.acc == nullptr) {
#pragma unroll
        for (int b = 0; b < B; ++b) p.partial[((size_t)slice * B + b) * p.M + row_begin + r] = v[b];
      } else {
        // Fused finalize.  The slice sum goes into the row's cell as a fixed-point number in bits 63..10 (integer adds
        // commute: the total does not depend on the order the 16 workgroups arrive in), together with +1 in the arrival
        // counter (bits 4..0) and +1 in bits 9..5 if the value is not finite.  The unit 2^-sh comes from a bound every
        // workgroup of the layer computes identically: |slice sum| <= in_features * max|codebook| * max|x| < 2^e, so
        // with sh = 47 - e sixteen addends stay below 2^52 -- no overflow whatever the data, and ~2^-47 of the bound as
        // resolution (fp32 partials carry 2^-24 of their own magnitude).  ONE returning atomic per cell is the whole
        // hand-shake: whoever reads 15 earlier arrivals owns the total, applies scale and bias, rounds once, writes y and
        // puts the cell back to zero for the next launch.
        const int row = row_begin + r;
        unsigned long long old[B], mine[B];
        int sh[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
          uint32_t xm = 0u;  // every wave of the workgroup left the maximum of its share of x
          {                  // (16 slots = four 16-B reads in flight together)
            static_assert(PK_MAX_NW == 16, "four 16-byte reads cover the slots");
            u32x4 sl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sl[q] = *(lds_u32x4_ptr)(size_t)(xmax_off + (uint32_t)(b * PK_MAX_NW + q * 4) * 4u);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const uint32_t a = sl[q].x > sl[q].y ? sl[q].x : sl[q].y, c = sl[q].z > sl[q].w ? sl[q].z : sl[q].w;
              const uint32_t d = a > c ? a : c;
              xm = d > xm ? d : xm;
            }
          }
          const float bound = (float)p.in_groups * (float)PK_G * p.cb_absmax * T_::to_float((uint16_t)xm);
          int e = 0;
          (void)frexpf(bound, &e);                               // bound < 2^e (e = 0 for bound == 0)
          const bool finite = bound < __builtin_inff() && fabsf(v[b]) <= 2.f * bound;  // false for NaN / Inf anywhere
          sh[b] = PK_FIX_BITS - e;
          const long long q = finite ? __float2ll_rn(ldexpf(v[b], sh[b])) : 0ll;
          mine[b] = ((unsigned long long)q << PK_VAL_SHIFT) + (finite ? 1ull : 1ull + (1ull << PK_CNT_BITS));
          old[b] = __hip_atomic_fetch_add(p.acc + (size_t)b * p.M + row, mine[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool first = FOLD || r == tid;  // this thread's first (usually only) row: scale and bias were requested in the prologue
        const float scale = pub_half ? 1.f : T_::to_float(first ? scale_h : p.scales[row]);
        const float bias = (pub_half || !p.bias) ? 0.f : T_::to_float(first ? bias_h : p.bias[row]);
#pragma unroll
        for (int b = 0; b < B; ++b) {
          if ((old[b] & PK_CNT_MASK) == (unsigned long long)(PK_S - 1)) {
            const unsigned long long cell = old[b] + mine[b];
            const long long sum = (long long)cell >> PK_VAL_SHIFT;
            float sv = (float)ldexp((double)sum, -sh[b]);
            if ((cell >> PK_CNT_BITS) & PK_CNT_MASK) sv = __builtin_nanf("");
            if (pub_half)  // the shard's fp32 total, visible to the peers (write-through, system scope); scale / bias later
              __hip_atomic_store(pub_half + (size_t)b * p.M + row, sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else
              p.y[(size_t)b * p.y_row_stride + row] = T_::from_float(__builtin_fmaf(sv, scale, bias));
            __hip_atomic_store(p.acc + (size_t)b * p.M + row, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
  }
  if (pub_half) {
    // Every row total of this launch is published by exactly one workgroup before that workgroup arrives here: when all
    // PK_NST workgroups have arrived (8 sharded counters of PK_NST / 8 arrivals, then one of 8 -- a single counter would
    // serialise 256 device-scope atomics), everything is out and the rank's flag goes up.  Stores are drained first
    // (write-through + vmcnt(0) == published, cdna_hip_programming.md Guideline 16 R1).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      uint32_t* shard = p.pub_epoch + 4 + (block & 7);
      const uint32_t a = __hip_atomic_fetch_add(shard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a + 1u == (uint32_t)(PK_NST / 8)) {
        __hip_atomic_store(shard, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t t = __hip_atomic_fetch_add(p.pub_epoch + 12, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t + 1u == 8u) {
          __hip_atomic_store(p.pub_epoch + 12, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(p.pub_flag + (pub_e & 1u), pub_e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
  if constexpr (FOLD) {
    if (++pass < npass) {  // the next row group of this slice: what was requested in front of the epilogue is its own now
      group += group_step;
      stream_ix = group * PK_S + slice;
      row_begin = group * p.RG;
      nrows = p.M - row_begin;
      nrows = nrows < 0 ? 0 : (nrows < p.RG ? nrows : p.RG);
      scale_h = scale_n;
      bias_h = bias_n;
      q0_h = q0_n;
      q1_h = q1_n;
#pragma unroll
      for (int b = 0; b < B; ++b)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[b][a] = 0.f;
      row_addr = 0;
      // every row of this pass has a writer and every column of the stream's waves stores its remainder, so nothing of pass j
      // is read in pass j + 1 -- but loop j + 1 must not write rowval / colend while a wave still reads them in epilogue j.
      // The bare barrier, not __syncthreads(): its vmcnt(0) would wait for the ring that was just requested.
      asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
      __builtin_amdgcn_s_barrier();
      goto next_pass;
    }
  }
#ifdef AQLM_PACKED_TRACE
  AQLM_TRACE(6);
  if (p.trace && lane == 0) {
    unsigned long long* o = p.trace + ((size_t)block * PK_MAX_NW + wave) * 8;
    tr[3] = __builtin_readcyclecounter() - cyc0;  // shader cycles from entry to end (slot 3 is not a time stamp)
    tr[7] = ((unsigned long long)tr_wait << 32) | tr_work;  // steps of the main loop: cycles waiting for entries | cycles in LDS reads + dots
    for (int i = 0; i < 8; ++i) o[i] = tr[i];
  }
#endif
}

// What the prologue needs before it can issue its first load comes as individual leading arguments: with
// -amdgpu-kernarg-preload-count (Makefile) the command processor delivers those 14 dwords in SGPRs at wave launch, and
// the cold s_load round trip of the kernel-argument segment leaves the head of the critical path.  Struct arguments
// are not preloaded; the rest of the parameters (needed after the LDS fill) stay in one.
struct PackedGemvRest {
  const uint32_t* winfo;
  float* partial;
  long x_row_stride;
  unsigned long long* acc;
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* y;
  long y_row_stride;
  float cb_absmax;
  const uint8_t* next_ent;
  const uint8_t* next_codebook;
  uint32_t next_block_bytes;
  float* pub;
  uint32_t* pub_flag;
  uint32_t* pub_epoch;
  uint32_t pub_max_elems;
#ifdef AQLM_PACKED_TRACE
  unsigned long long* trace;
  int dbg;
#endif
};

template <class T_, int B, int PD, uint32_t XWIN, int EB, bool PUB = false>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_kernel(const uint8_t* codebook, const uint16_t* x, const uint32_t* ent,
                                                                const uint32_t* rowstart, int in_groups, uint32_t geom, int RG,
                                                                uint32_t ent_bytes, int M, const PackedGemvRest rest) {
  // geom: waves 0..7 | x copies 8..11 | prefetch waves 12..14 | rotated fill 15 | steps 16..31
  const int NW = (int)(geom & 0xffu), XC = (int)((geom >> 8) & 0xfu), NPW = (int)((geom >> 12) & 7u), T = (int)(geom >> 16);
  PackedGemvParams p;
  p.NPW = NPW;
  p.fill_rotate = (int)((geom >> 15) & 1u);
  p.next_ent = rest.next_ent;
  p.next_codebook = rest.next_codebook;
  p.next_block_bytes = rest.next_block_bytes;
  p.pub = rest.pub;
  p.pub_flag = rest.pub_flag;
  p.pub_epoch = rest.pub_epoch;
  p.pub_max_elems = rest.pub_max_elems;
  p.ent = ent;
  p.winfo = rest.winfo;
  p.rowstart = rowstart;
  p.codebook = codebook;
  p.x = x;
  p.partial = rest.partial;
  p.acc = rest.acc;
  p.cb_absmax = rest.cb_absmax;
  p.scales = rest.scales;
  p.bias = rest.bias;
  p.y = rest.y;
  p.y_row_stride = rest.y_row_stride;
  p.x_row_stride = rest.x_row_stride;
  p.M = M;
  p.in_groups = in_groups;
  p.RG = RG;
  p.NW = NW;
  p.T = T;
  p.XC = XC;
  p.ent_bytes = ent_bytes;
#ifdef AQLM_PACKED_TRACE
  p.trace = rest.trace;
  p.dbg = rest.dbg;
#endif
  gemv_1x16_packed_body<T_, B, PD, XWIN, EB, PUB>(p, blockIdx.x, NW + NPW);
}

#if AQLM_PK_G == 8
// Variable-geometry twin (format v7, flag AQLM_HIP_PACKED_VARGEOM): same body; the 14 preloaded dwords now also carry the row
// groups of the 16 slices, so three of the ordinary kernel's arguments travel compressed: the row-start table as its distance
// in front of the entries, in_groups and the row-table size in one word, and the entry bytes are derived (4-byte entries only).
template <class T_, int B, int PD, uint32_t XWIN>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_vg_kernel(const uint8_t* codebook, const uint16_t* x, const uint32_t* ent,
                                                                   uint32_t rowstart_back, uint32_t ig_rg, uint32_t geom, int M,
                                                                   uint32_t ns0, uint32_t ns1, uint32_t ns2, uint32_t ns3,
                                                                   const PackedGemvRest rest) {
  // geom: waves 0..7 | x copies 8..11 | rotated fill 15 | steps 16..31;  ig_rg: in_groups 0..11 | rows per group 12..27
  const int NW = (int)(geom & 0xffu), XC = (int)((geom >> 8) & 0xfu), T = (int)(geom >> 16);
  PackedGemvParams p;
  p.NPW = 0;
  p.fill_rotate = (int)((geom >> 15) & 1u);
  p.next_ent = nullptr;
  p.next_codebook = nullptr;
  p.next_block_bytes = 0;
  p.pub = nullptr;
  p.pub_flag = nullptr;
  p.pub_epoch = nullptr;
  p.pub_max_elems = 0;
  p.ent = ent;
  p.winfo = rest.winfo;
  p.rowstart = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ent) - rowstart_back);
  p.codebook = codebook;
  p.x = x;
  p.partial = rest.partial;
  p.acc = rest.acc;
  p.cb_absmax = rest.cb_absmax;
  p.scales = rest.scales;
  p.bias = rest.bias;
  p.y = rest.y;
  p.y_row_stride = rest.y_row_stride;
  p.x_row_stride = rest.x_row_stride;
  p.M = M;
  p.in_groups = (int)(ig_rg & 0xfffu);
  p.RG = (int)(ig_rg >> 12);
  p.NW = NW;
  p.T = T;
  p.XC = XC;
  p.ent_bytes = (uint32_t)PK_NST * (uint32_t)NW * (uint32_t)T * 1024u;
#ifdef AQLM_PACKED_TRACE
  p.trace = rest.trace;
  p.dbg = rest.dbg;
#endif
  const PackedVgArgs vg{{ns0, ns1, ns2, ns3}};
  gemv_1x16_packed_body<T_, B, PD, XWIN, 4, false, true>(p, blockIdx.x, NW, vg);
}
#endif

// Several prepacked layers that multiply the same x (q/k/v, gate/up) in one launch of 256 workgroups per layer; the
// next layer's workgroups start as CUs free up, so one layer's tail and the next one's LDS fill overlap.
struct PackedSegment {
  const uint32_t* ent;
  const uint32_t* winfo;
  const uint32_t* rowstart;
  const uint8_t* codebook;
  float* partial;
  int M, RG, NW, T, XC;
  uint32_t ent_bytes;
  // fused finalize (acc != nullptr)
  unsigned long long* acc;
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* y;
  long y_row_stride;
  float cb_absmax;
};

struct PackedMultiParams {
  const uint16_t* x;
  long x_row_stride;
  int in_groups, nseg;
  PackedSegment seg[AQLM_HIP_MAX_SEGMENTS];
};

template <class T_, int B, int PD, uint32_t XWIN, int EB>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_multi_kernel(const PackedMultiParams mp) {
  const int sidx = (int)blockIdx.x / PK_NST;
  PackedGemvParams p{};
  p.x = mp.x;
  p.x_row_stride = mp.x_row_stride;
  p.in_groups = mp.in_groups;
#pragma unroll
  for (int k = 0; k < AQLM_HIP_MAX_SEGMENTS; ++k) {
    if (k == 0 || sidx == k) {  // scalar select chain (no dynamic indexing of the kernel-argument struct)
      p.ent = mp.seg[k].ent;
      p.winfo = mp.seg[k].winfo;
      p.rowstart = mp.seg[k].rowstart;
      p.codebook = mp.seg[k].codebook;
      p.partial = mp.seg[k].partial;
      p.M = mp.seg[k].M;
      p.RG = mp.seg[k].RG;
      p.NW = mp.seg[k].NW;
      p.T = mp.seg[k].T;
      p.XC = mp.seg[k].XC;
      p.ent_bytes = mp.seg[k].ent_bytes;
      p.acc = mp.seg[k].acc;
      p.scales = mp.seg[k].scales;
      p.bias = mp.seg[k].bias;
      p.y = mp.seg[k].y;
      p.y_row_stride = mp.seg[k].y_row_stride;
      p.cb_absmax = mp.seg[k].cb_absmax;
    }
  }
  gemv_1x16_packed_body<T_, B, PD, XWIN, EB>(p, (int)blockIdx.x % PK_NST, (int)blockDim.x >> 6);
}

#if AQLM_PK_G == 8
// Several INDEPENDENT one-row layers in one launch of 256 workgroups per layer: what capture overlap makes of launches that
// may share a graph node (capture_overlap.h, "Grouped launches").  Every segment is a complete single-layer launch -- its own
// x, codebook, stream, cells, y and geometry, exactly the arguments of gemv_1x16_packed_kernel / _vg_kernel -- and all of a
// launch's segments have the block size and the LDS image of one kernel instance.  Within the launch the dispatcher puts a
// workgroup of the next layer on a CU the moment one leaves; between graph nodes that costs a launch boundary and the tail of
// the slowest workgroup.  No prefetch waves, no publish form.
constexpr int PK_GROUP_MAX = capture_overlap::kMaxMerge;  // the planner never puts more launches into a node
struct PackedGroupSegment {
  const uint8_t* codebook;
  const uint16_t* x;
  const uint32_t* ent;
  const uint32_t* rowstart;
  int in_groups, RG, M;
  uint32_t geom;  // as the single-layer kernels take it (prefetch waves 0)
  uint32_t ent_bytes;
  uint32_t ns[4];  // variable geometry: PackedVgArgs
  PackedGemvRest rest;
};
struct PackedGroupParams {
  PackedGroupSegment seg[PK_GROUP_MAX];
};

// The segment is read where the launch put it: the kernel arguments are memory (the kernarg segment, constant address space),
// `gp` is the only argument and so starts at offset 0, and a segment's fields are a few uniform loads at sidx * sizeof(segment)
// from there.  (Indexing the by-value `gp` with sidx makes hipcc copy it to scratch first; a select chain over the segments,
// as in the shared-input kernel, costs ~130 scalar instructions in front of the first load of every workgroup.)
typedef const PackedGroupSegment __attribute__((address_space(4)))* group_segment_ptr;
template <class T_, int PD, uint32_t XWIN, int EB, bool VG>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_group_kernel(const PackedGroupParams gp) {
  (void)gp;
  const int sidx = (int)blockIdx.x / PK_NST;
  const group_segment_ptr s = (group_segment_ptr)__builtin_amdgcn_kernarg_segment_ptr() + sidx;
  PackedGemvParams p{};  // (no prefetch waves, no next layer, no publish: zero)
  PackedVgArgs vg{};
  p.codebook = s->codebook;
  p.x = s->x;
  p.ent = s->ent;
  p.rowstart = s->rowstart;
  p.in_groups = s->in_groups;
  p.RG = s->RG;
  p.M = s->M;
  const uint32_t geom = s->geom;
  p.ent_bytes = s->ent_bytes;
  if constexpr (VG) {
    vg.ns[0] = s->ns[0];
    vg.ns[1] = s->ns[1];
    vg.ns[2] = s->ns[2];
    vg.ns[3] = s->ns[3];
  }
  p.winfo = s->rest.winfo;
  p.partial = s->rest.partial;
  p.x_row_stride = s->rest.x_row_stride;
  p.acc = s->rest.acc;
  p.cb_absmax = s->rest.cb_absmax;
  p.scales = s->rest.scales;
  p.bias = s->rest.bias;
  p.y = s->rest.y;
  p.y_row_stride = s->rest.y_row_stride;
#ifdef AQLM_PACKED_TRACE
  p.trace = s->rest.trace;
  p.dbg = s->rest.dbg;
#endif
  // geom: waves 0..7 | x copies 8..11 | rotated fill 15 | steps 16..31
  p.NW = (int)(geom & 0xffu);
  p.XC = (int)((geom >> 8) & 0xfu);
  p.fill_rotate = (int)((geom >> 15) & 1u);
  p.T = (int)(geom >> 16);
  gemv_1x16_packed_body<T_, 1, PD, XWIN, EB, false, VG>(p, (int)blockIdx.x % PK_NST, (int)blockDim.x >> 6, vg);
}

// The folded form of the grouped launch (ordinary geometry only: the row groups of a variable-geometry slice differ).  A node
// of at least F members (F = 2 or 4, the second argument; one instance serves both) runs as members * 256 / F workgroups: in the
// unfolded grid the 16 row-group workgroups of a (layer, slice) each pull the same 64 KiB slice and 8 KiB of x through their
// CU's L1 into LDS before they touch a code, and a node of several members holds more workgroups than the chip has LDS slots
// anyway.  Here one workgroup keeps slice and x and walks F of those row groups in turn (gemv_1x16_packed_body, FOLD); where it
// sits is group_fold::place (group_fold.h), shared with the host.  Same LDS image, same block size, same bits in y.
template <class T_, int PD, uint32_t XWIN, int EB>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_group_fold_kernel(const PackedGroupParams gp, const int fold) {
  (void)gp;
  static_assert(PK_S == group_fold::kSlices && PK_NST == group_fold::kStreams, "group_fold.h: 16 slices x 16 row groups");
  const group_fold::Place at = group_fold::place(blockIdx.x, fold);
  const group_segment_ptr s = (group_segment_ptr)__builtin_amdgcn_kernarg_segment_ptr() + at.segment;
  PackedGemvParams p{};
  p.codebook = s->codebook;
  p.x = s->x;
  p.ent = s->ent;
  p.rowstart = s->rowstart;
  p.in_groups = s->in_groups;
  p.RG = s->RG;
  p.M = s->M;
  const uint32_t geom = s->geom;
  p.ent_bytes = s->ent_bytes;
  p.winfo = s->rest.winfo;
  p.partial = s->rest.partial;
  p.x_row_stride = s->rest.x_row_stride;
  p.acc = s->rest.acc;
  p.cb_absmax = s->rest.cb_absmax;
  p.scales = s->rest.scales;
  p.bias = s->rest.bias;
  p.y = s->rest.y;
  p.y_row_stride = s->rest.y_row_stride;
#ifdef AQLM_PACKED_TRACE
  p.trace = s->rest.trace;
  p.dbg = s->rest.dbg;
#endif
  p.NW = (int)(geom & 0xffu);
  p.XC = (int)((geom >> 8) & 0xfu);
  p.fill_rotate = (int)((geom >> 15) & 1u);
  p.T = (int)(geom >> 16);
  gemv_1x16_packed_body<T_, 1, PD, XWIN, EB, false, false, true, true>(p, group_fold::stream(at, 0), (int)blockDim.x >> 6, PackedVgArgs{},
                                                                       fold, at.group_step);
}
#endif

struct PackedFinalizeParams {
  const float* partial;  // [S][B][M]
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* y;
  long y_row_stride;
  int M, B;
};

template <class T_>
__device__ __forceinline__ void packed_finalize_row(const PackedFinalizeParams& p, int row) {
  if (row >= p.M) return;
  const float scale = T_::to_float(p.scales[row]);
  const float bias = p.bias ? T_::to_float(p.bias[row]) : 0.f;
  for (int b = 0; b < p.B; ++b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PK_S; ++k) s += p.partial[((size_t)k * p.B + b) * p.M + row];
    p.y[(size_t)b * p.y_row_stride + row] = T_::from_float(__builtin_fmaf(s, scale, bias));
  }
}

// scalar arguments: preloaded into SGPRs at wave launch (see gemv_1x16_packed_kernel); this kernel is one dependent load
// round trip long, the kernel-argument fetch would be a second one
template <class T_>
__global__ __launch_bounds__(256) void gemv_1x16_packed_finalize(const float* partial, const uint16_t* scales, const uint16_t* bias,
                                                                 uint16_t* y, long y_row_stride, int M, int B) {
  PackedFinalizeParams p;
  p.partial = partial;
  p.scales = scales;
  p.bias = bias;
  p.y = y;
  p.y_row_stride = y_row_stride;
  p.M = M;
  p.B = B;
  packed_finalize_row<T_>(p, blockIdx.x * 256 + threadIdx.x);
}

struct PackedFinalizeSegment {
  PackedFinalizeParams f;
  int block_begin;
};

struct PackedFinalizeMultiParams {
  int nseg;
  PackedFinalizeSegment seg[AQLM_HIP_MAX_SEGMENTS];
};

template <class T_>
__global__ __launch_bounds__(256) void gemv_1x16_packed_finalize_multi(const PackedFinalizeMultiParams mp) {
  PackedFinalizeParams p = mp.seg[0].f;
  int begin = 0;
#pragma unroll
  for (int k = 1; k < AQLM_HIP_MAX_SEGMENTS; ++k) {
    if (k < mp.nseg && (int)blockIdx.x >= mp.seg[k].block_begin) {
      p = mp.seg[k].f;
      begin = mp.seg[k].block_begin;
    }
  }
  packed_finalize_row<T_>(p, ((int)blockIdx.x - begin) * 256 + threadIdx.x);
}

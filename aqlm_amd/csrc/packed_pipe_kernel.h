// Part of gemv_packed.hip (inside namespace aqlm::PK_NS): the pipelined shared-input kernel -- PP_* constants, its LDS map (PipeLds,
// pipe_lds), PipeParams, gemv_1x16_packed_pipe_kernel and the host rule that admits a call to it (pipe_eligible).  Needs
// packed_format.h and the segment struct, LDS helpers and finalize arithmetic of packed_gemv_kernels.h.

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

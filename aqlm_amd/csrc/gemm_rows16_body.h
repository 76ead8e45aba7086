// Body of the 16-row fused 1x16 MFMA GEMM (gemm_1x16_rows16.h, a part of gemm_mfma.hip, describes the design), shared TEXTUALLY
// by two kernels: it is #included inside the braces of gemm_1x16_rows16_kernel (there) and gemm_1x16_grouped_kernel (moe_grouped.hip).  A
// function, even a force-inlined one, is simplified on its own before it is inlined and the kernels' instruction streams moved
// (operand order, scheduling); the fragment keeps gemm_1x16_rows16_kernel's code exactly what it was when the body lived in it.
//
// The including kernel has template parameters T, G, NBT, CPB, an R16Params `p` and defines
//   R16_ROW0       first output row of the block
//   R16_X_ROW(b)   the X row batch row b reads, valid for every b < 16 NBT (rows past p.B: a valid row, computed, never stored)
//   R16_Y_ROW(b)   the Y row batch row b < p.B writes
// The fragment undefines the three.  No include guard: one copy per kernel.
{
  using LDS = R16Lds<NBT, CPB>;
  constexpr int NSW = LDS::NSW, NSX = LDS::NSX;
  extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)glds_smem != 0u) __builtin_trap();  // LDS map of gemm_rows16.h starts at 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = lane & 15, kg = lane >> 4;
  const int row0 = R16_ROW0;
  const int n = p.nsteps;  // >= max(NSW, NSX) - 1 (host)

  if (wave == 0) {
    // ============================================ gather producer ====================================================
    __builtin_amdgcn_s_setprio(3);
    constexpr int P0 = 1 + 2 * CPB;  // LDS-DMA operations per step: codes, 2 fragments per chunk
    static_assert((NSW - 2) * P0 < 64, "vmcnt is 6 bits");
    // codes of a step: row r holds ROW_BYTES = CPB x 16 B (g = 8: 8 codes per chunk) or CPB x 8 B (g = 16: 4 codes); one DMA
    // instruction moves the 16 rows in pieces of 16 B (4 B when a row has only 8), lanes in (row, piece) order, so a slot of the
    // ring reads [row][chunk][codes]
    constexpr uint32_t CHUNK_BYTES = G == 8 ? 16u : 8u;  // code bytes of one row and chunk
    constexpr uint32_t RB = CHUNK_BYTES * CPB;
    constexpr uint32_t DMA_BYTES = RB >= 16u ? 16u : 4u;
    constexpr int PARTS = (int)(RB / DMA_BYTES);          // lanes per row
    constexpr int CODE_LANES = 16 * PARTS;
    static_assert(CODE_LANES <= 64, "one DMA instruction moves the codes of a step");
    const uint8_t* code_src;
    {
      int r = row0 + lane / PARTS;
      r = r < p.M ? r : p.M - 1;
      code_src = p.codes + ((size_t)r * p.in_groups) * 2 + (size_t)(lane % PARTS) * DMA_BYTES;
    }
    constexpr uint32_t ROW_BYTES = CHUNK_BYTES * CPB;
    constexpr uint32_t CODE_STEP = G == 8 ? 8u : 4u;  // bytes between the codes of k step 0 and k step 1 of a chunk
    const uint32_t code_off0 = (uint32_t)arow * ROW_BYTES + (G == 8 ? (uint32_t)kg * 2u : (uint32_t)(kg >> 1) * 2u);
    const uint32_t half_off = G == 8 ? 0u : (uint32_t)(kg & 1) * 16u;
    auto dma_codes = [&](int step) {  // step may run past K: clamped (the slot is written, never used)
      const int cc = step < n ? step : n - 1;
      if (lane < CODE_LANES) {
        ggbl_void_ptr src = (ggbl_void_ptr)(code_src + (size_t)cc * RB);
        glds_void_ptr dst = (glds_void_ptr)(size_t)(LDS::CODES + (uint32_t)(step & (LDS::NSLOT - 1)) * LDS::CODE_SLOT);
        if constexpr (DMA_BYTES == 16u) __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
        else __builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);
      }
    };
    auto read_codes = [&](int step, uint32_t (&c)[2 * CPB]) {
      const uint32_t a = LDS::CODES + (uint32_t)(step & (LDS::NSLOT - 1)) * LDS::CODE_SLOT + code_off0;
#pragma unroll
      for (int u = 0; u < CPB; ++u)
#pragma unroll
        for (int s = 0; s < 2; ++s) c[u * 2 + s] = *(glds_u16_ptr)(size_t)(a + (uint32_t)u * CHUNK_BYTES + (uint32_t)s * CODE_STEP);
    };
    auto dma_stage = [&](int stage, const uint32_t (&c)[2 * CPB]) {
#pragma unroll
      for (int f = 0; f < 2 * CPB; ++f)
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(p.codebook + (size_t)c[f] * (G * 2) + half_off),
                                         (glds_void_ptr)(size_t)(LDS::W + (uint32_t)stage * LDS::W_STAGE + (uint32_t)f * 1024u), 16, 0, 0);
    };
    uint32_t creg[2 * CPB];
#pragma unroll
    for (int j = 0; j < NSW; ++j) dma_codes(j);
    __builtin_amdgcn_s_waitcnt(gl_vmcnt(0));
    read_codes(0, creg);
    for (int q = 0; q < NSW - 1; ++q) {  // steps 0 .. NSW - 2 before the first barrier
      dma_codes(q + NSW);
      dma_stage(q, creg);
      read_codes(q + 1, creg);  // requested before the wait above (q + 1 < NSW)
    }
    int stage = NSW - 1;  // stage of step i + NSW - 1
    int i = 0;
    for (; i + NSW - 1 < n; ++i) {
      __builtin_amdgcn_s_waitcnt(gl_vmcnt((NSW - 2) * P0));  // what this wave issued NSW - 1 iterations ago has landed
      __builtin_amdgcn_s_barrier();                           // step i is complete; the consumers are done with step i - 1
      const int q = i + NSW - 1;
      dma_codes(q + NSW);
      dma_stage(stage, creg);
      read_codes(q + 1, creg);  // requested NSW - 1 iterations ago: covered by the wait that opened this iteration
      stage = stage == NSW - 1 ? 0 : stage + 1;
    }
    r16_drain<NSW - 2, P0>();  // steps n - NSW + 1 .. n - 1 are in flight, one more lands per barrier
    return;
  }

  if (wave <= LDS::NXP) {
    // ============================================== X producer =======================================================
    constexpr int PX = LDS::PXW;
    constexpr int PPC = 2 * NBT;  // pieces per chunk
    static_assert((NSX - 2) * PX < 64, "vmcnt is 6 bits");
    const int xw = wave - 1;
    const uint8_t* x_src[PX];
    uint32_t x_dst[PX];
#pragma unroll
    for (int x = 0; x < PX; ++x) {
      const int piece = xw * PX + x;             // of the step: chunk piece / PPC, chunk piece piece % PPC
      const int u = piece / PPC, pc = piece % PPC;
      const int s = pc * 64 + lane;              // slot of the chunk image: batch row s >> 3, k piece (s & 7) ^ swizzle
      const int b = s >> 3;
      const int c = (s & 7) ^ ((b >> 1) & 7);
      x_src[x] = (const uint8_t*)(p.X + (size_t)(R16_X_ROW(b)) * p.xs + c * 8) + (size_t)u * 128;
      x_dst[x] = LDS::X + (uint32_t)u * LDS::X_CHUNK + (uint32_t)pc * 1024u;
    }
    auto dma_x = [&](int step, int stage) {
      const int cc = step < n ? step : n - 1;
#pragma unroll
      for (int x = 0; x < PX; ++x)
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(x_src[x] + (size_t)cc * (128 * CPB)),
                                         (glds_void_ptr)(size_t)(x_dst[x] + (uint32_t)stage * LDS::X_STAGE), 16, 0, 0);
    };
    for (int q = 0; q < NSX - 1; ++q) dma_x(q, q);
    int stage = NSX - 1;
    int i = 0;
    for (; i + NSX - 1 < n; ++i) {
      __builtin_amdgcn_s_waitcnt(gl_vmcnt((NSX - 2) * PX));
      __builtin_amdgcn_s_barrier();
      dma_x(i + NSX - 1, stage);
      stage = stage == NSX - 1 ? 0 : stage + 1;
    }
    r16_drain<NSX - 2, PX>();
    return;
  }

  // ================================================ consumer ============================================================
  constexpr int CT = NBT >= R16_NC ? NBT / R16_NC : 1;  // batch tiles per consumer wave
  const int cw = wave - 1 - LDS::NXP;
  const bool active = cw * CT < NBT;
  f32x4 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int sw = 0, sx = 0;
  for (int c = 0; c < n; ++c) {
    __builtin_amdgcn_s_barrier();
    if (active) {
      const uint32_t wbase = LDS::W + (uint32_t)sw * LDS::W_STAGE, xbase = LDS::X + (uint32_t)sx * LDS::X_STAGE;
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        u32x4 a[2], b[2][CT];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          a[s] = *(glds_u32x4_ptr)(size_t)(wbase + (uint32_t)(u * 2 + s) * 1024u + (uint32_t)lane * 16u);
#pragma unroll
          for (int t = 0; t < CT; ++t)
            b[s][t] = *(glds_u32x4_ptr)(size_t)(xbase + (uint32_t)u * LDS::X_CHUNK + (uint32_t)xswz((cw * CT + t) * 16 + arow, s * 4 + kg) * 16u);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int t = 0; t < CT; ++t) acc[t] = mfma16<T>(a[s], b[s][t], acc[t]);
      }
    }
    sw = sw == NSW - 1 ? 0 : sw + 1;
    sx = sx == NSX - 1 ? 0 : sx + 1;
  }
  if (!active) return;
  // ---- epilogue: lane (arow, kg) holds rows 4 kg .. 4 kg + 3 of the block, batch column 16 (cw CT + t) + arow --------------
  const int m = row0 + kg * 4;
  if (m >= p.M) return;
  float sc[4], bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mm = m + r < p.M ? m + r : p.M - 1;
    sc[r] = T::to_float(p.scales[mm]);
    bi[r] = p.bias ? T::to_float(p.bias[mm]) : 0.f;
  }
  const bool vec = (p.M & 3) == 0 && (p.ys & 3) == 0 && ((uintptr_t)p.Y & 7u) == 0;  // (Y only 2- / 4-byte aligned: scalar stores)
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int b = (cw * CT + t) * 16 + arow;
    if (b < p.B) {
      uint16_t* dst = p.Y + (size_t)(R16_Y_ROW(b)) * p.ys + m;
      uint16_t h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = T::from_float(__builtin_fmaf(acc[t][r], sc[r], bi[r]));
      if (vec) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
      else
        for (int r = 0; r < 4; ++r)
          if (m + r < p.M) dst[r] = h[r];
    }
  }
}
#undef R16_ROW0
#undef R16_X_ROW
#undef R16_Y_ROW

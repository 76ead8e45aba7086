// Part of gemm_mfma.hip (read there, inside namespace aqlm): the K-split LDS-DMA pipeline of the 1x16 scheme, its finalize kernel (which
// the K-split form of the K x 8 kernel shares), plan and launches.
// ---------------------------------------------------------------------------------------------------------------
// LDS-DMA pipeline (default since round 3): every global read of the main loop is a global_load_lds -- the X tiles,
// the codes AND the codebook gathers -- so nothing of the stream occupies VGPRs, the wave's VMEM queue holds one kind
// of operation (hipcc waits with vmcnt(0) for any register load that sits beside an LDS-DMA, cdna_hip_programming.md
// section 5 trap (b)) and all waits are counted by hand (static counts, raw s_barrier).
//
//   block  = 8 waves = 128 output rows (16 per wave) x one K slice x <= 128 batch columns; 1 block per CU
//   MFMA   = v_mfma_f32_16x16x32: A = W (lane (r, kg): row r, 8 k of k-group kg = ONE codebook vector for g = 8, one
//            half of one for g = 16), B = X^T (lane (r, kg): batch column 16 t + r, the same 8 k), C = 4 consecutive
//            output rows of one batch column per lane -> partial / Y stores of 16 B
//   gather = one global_load_lds_dwordx4 per 32-deep k step and wave: lane (r, kg) names the address of ITS fragment,
//            the DMA drops the 64 fragments into LDS in lane order, and the A operand is read back with one
//            conflict-free ds_read_b128.  The gathered entry is still the MFMA fragment; LDS is only the landing zone
//            that lets NS - 1 = 3 chunks (48 wave-gathers = 3072 lane-gathers per CU) be in flight without registers.
//   codes  = 16 B per row and 64-deep chunk, DMA'd 2 NS - 1 chunks ahead into a wave-private ring, read back one
//            iteration before the gather that needs them
//   X      = Bpad x 64 k chunks into the XOR-swizzled image of xswz() (swizzle applied to the SOURCE address: the DMA
//            writes lane-linear), shared by the 8 waves
//   K split over the blocks of one XCD (block -> XCD affinity b % 8, speed only): fp32 partials [ks][b][m] stay in that
//   XCD's L2 for the finalize kernel, which is mapped the same way.  One barrier per chunk.
//
// Per-CU traffic through the L1 fill path for 4096 x 4096, B = 128: 8192 gathered lines (1 MiB) + 128 KiB of X.

struct GldsParams {
  const uint8_t* codes;     // [M][in_groups] u16
  const uint8_t* codebook;  // [65536][G] halfs
  const uint16_t* X;        // [B][xs]
  float* partial;           // [ksplit][B][M] fp32 (ksplit > 1)
  const uint16_t* scales;   // ksplit == 1: the block writes Y itself
  const uint16_t* bias;
  uint16_t* Y;
  long xs, ys;
  int M, B, in_groups;
  int row_blocks, ksplit;
  int chunks_base, chunks_rem;  // K slice ks covers chunks_base + (ks < chunks_rem) chunks of 64 k
  int store_nt;                 // partial stores with the non-temporal hint (tuning knob, A/B runs)
  int dbg;                      // knock-out switches for timing experiments (results are wrong): 1 no MFMA, 2 no fragment reads, 4 no stores, 8 no X DMA, 16 gathers from one line
};

constexpr int GL_NS = 4;       // stages of the W / X ring
constexpr int GL_NSLOT = 8;    // slots of a wave's code ring (>= GL_NS + 1, power of two)
constexpr int GL_WAVES = 8;      // consumer waves (16 output rows each)
constexpr int GL_PRODUCERS = 4;  // DMA waves
constexpr uint32_t GL_W_BYTES = GL_WAVES * 2048u;  // per stage: 2 fragments of 1 KiB per wave

template <int XW>
struct GldsLds {
  static constexpr uint32_t X_BYTES = XW * 64u * 128u;        // XW * 64 batch rows x 64 k
  static constexpr uint32_t W_BYTES = GL_W_BYTES;             // per stage: 2 fragments of 1 KiB per consumer wave
  static constexpr uint32_t STAGE = W_BYTES + X_BYTES;
  static constexpr uint32_t CODES = GL_NS * STAGE;            // [producer][slot][512 B]
  static constexpr uint32_t TOTAL = CODES + GL_PRODUCERS * GL_NSLOT * 512u;
};


// Roles.  Measured with every wave doing both jobs (round 3, profiles/r03_mb_gemm_symmetric.log): a chunk took
// TA time + compute time -- a wave that is issuing LDS-DMA sits in the issue stage while the texture addresser works
// through the 64 scattered lines of each gather (its queue is a few instructions deep), and the addresser idles while the
// waves compute.  So the block is split: 8 consumer waves (16 rows each) only read fragments and run MFMAs, 4 producer
// waves (one per SIMD) only issue DMA -- codes, gathers, X -- and are parked in the issue stage almost all the time,
// which keeps the addresser fed.  One s_barrier per chunk joins them: the producers arrive when the chunk's DMA has
// landed (counted vmcnt), the consumers when they are done with the previous chunk (whose stage is refilled next).
template <class T, int G, int NBT, int XW>  // NBT = 16-column batch tiles computed; XW * 64 = batch rows staged
__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(3, 3))) void gemm_1x16_glds_kernel(const GldsParams p) {
  using LDS = GldsLds<XW>;
  constexpr int P = 1 + 4 + 2 * XW;  // LDS-DMA operations per producer wave and chunk: codes, 4 fragments, 2 XW pieces of X
  static_assert((GL_NS - 2) * P < 64, "vmcnt is 6 bits");
  extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)glds_smem != 0u) __builtin_trap();  // LDS map below starts at 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = lane & 15, kg = lane >> 4;

  // block -> (row block, K slice): the K slices of a row block run on one XCD (observed placement: block b on XCD b % 8)
  const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
  const int rb_hi = slot / p.ksplit;
  const int row_blk = rb_hi * 8 + xcd, ks = slot - rb_hi * p.ksplit;
  if (row_blk >= p.row_blocks) return;
  const int n = p.chunks_base + (ks < p.chunks_rem ? 1 : 0);                                // chunks of this block, >= GL_NS - 1
  const int chunk0 = ks * p.chunks_base + (ks < p.chunks_rem ? ks : p.chunks_rem);

  if (wave >= GL_WAVES) {
    // ============================================ producer ============================================================
    const int pw = wave - GL_WAVES;                 // serves consumer waves 2 pw and 2 pw + 1: 32 rows
    if (!(p.dbg & 32)) __builtin_amdgcn_s_setprio(3);  // the address arithmetic of the DMA wave goes ahead of the consumers' issue slots
    const int prow0 = row_blk * 128 + pw * 32;
    // codes: g = 8: lanes 0..31 move 16 B (8 codes) of row prow0 + lane; g = 16: all lanes move 4 B (2 codes), row lane / 2
    constexpr int CODE_LANES = G == 8 ? 32 : 64;
    constexpr int CODE_BYTES_PER_CHUNK = G == 8 ? 16 : 8;  // per row
    const uint8_t* code_src;
    {
      int r = prow0 + (G == 8 ? lane : (lane >> 1));
      r = r < p.M ? r : p.M - 1;
      code_src = p.codes + ((size_t)r * p.in_groups) * 2 + (size_t)chunk0 * CODE_BYTES_PER_CHUNK + (G == 8 ? 0 : (lane & 1) * 4);
    }
    // X: piece (pw * 2 XW + x) of a chunk image = 64 slots of 16 B; slot s holds batch row s >> 3, k piece (s & 7) ^ swizzle
    const uint8_t* x_src[2 * XW];
#pragma unroll
    for (int x = 0; x < 2 * XW; ++x) {
      const int s = (pw * 2 * XW + x) * 64 + lane;
      int b = s >> 3;
      const int c = (s & 7) ^ ((b >> 1) & 7);
      b = b < p.B ? b : p.B - 1;  // rows past the batch: a valid row, computed and never stored
      x_src[x] = (const uint8_t*)(p.X + (size_t)b * p.xs + (size_t)chunk0 * 64 + c * 8);
    }
    const uint32_t code_ring = LDS::CODES + (uint32_t)pw * (GL_NSLOT * 512u);
    // this lane's codes of a chunk inside a ring slot: consumer wave cw, k step s -> row 16 cw + arow; g = 8: code 4 s + kg,
    // g = 16: code 2 s + kg / 2 (and the lane takes the 16-B half kg & 1 of the 32-B entry)
    constexpr uint32_t ROW_BYTES = G == 8 ? 16u : 8u;
    constexpr uint32_t CODE_STEP = G == 8 ? 8u : 4u;  // bytes between the codes of k step 0 and k step 1
    const uint32_t code_off0 = (uint32_t)arow * ROW_BYTES + (G == 8 ? (uint32_t)kg * 2u : (uint32_t)(kg >> 1) * 2u);
    const uint32_t half_off = G == 8 ? 0u : (uint32_t)(kg & 1) * 16u;

    auto dma_codes = [&](int chunk) {  // chunk may run past the slice: clamped (the slot is written, never used)
      const int cc = chunk < n ? chunk : n - 1;
      if (lane < CODE_LANES) {
        ggbl_void_ptr src = (ggbl_void_ptr)(code_src + (size_t)cc * CODE_BYTES_PER_CHUNK);
        glds_void_ptr dst = (glds_void_ptr)(size_t)(code_ring + (uint32_t)(chunk & (GL_NSLOT - 1)) * 512u);
        if constexpr (G == 8) __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
        else __builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);
      }
    };
    auto read_codes = [&](int chunk, uint32_t (&c)[4]) {
      const uint32_t a = code_ring + (uint32_t)(chunk & (GL_NSLOT - 1)) * 512u + code_off0;
#pragma unroll
      for (int cw = 0; cw < 2; ++cw)
#pragma unroll
        for (int s = 0; s < 2; ++s) c[cw * 2 + s] = *(glds_u16_ptr)(size_t)(a + (uint32_t)cw * (16u * ROW_BYTES) + (uint32_t)s * CODE_STEP);
    };
    auto dma_stage = [&](int chunk, int stage, const uint32_t (&c)[4]) {
      const uint32_t base = (uint32_t)stage * LDS::STAGE;
#pragma unroll
      for (int f = 0; f < 4; ++f)  // fragment f = (consumer wave 2 pw + f / 2, k step f % 2)
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(p.codebook + (size_t)((p.dbg & 16) ? (c[f] & 7u) : c[f]) * (G * 2) + half_off),
                                         (glds_void_ptr)(size_t)(base + (uint32_t)(2 * pw) * 2048u + (uint32_t)f * 1024u), 16, 0, 0);
#pragma unroll
      for (int x = 0; x < 2 * XW; ++x)
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(x_src[x] + (size_t)((p.dbg & 8) ? 0 : chunk) * 128),
                                         (glds_void_ptr)(size_t)(base + LDS::W_BYTES + (uint32_t)(pw * 2 * XW + x) * 1024u), 16, 0, 0);
    };
    // prologue: codes of the first NS chunks (one exposed round trip: the gathers depend on them), then NS - 1 issue
    // iterations.  Issue iteration i: codes of chunk i + 2 NS - 1, stage of chunk q = i + NS - 1, read back the codes of
    // chunk q + 1 (their DMA is NS iterations old: covered by the wait that opens iteration i).
    uint32_t creg[4];
#pragma unroll
    for (int j = 0; j < GL_NS; ++j) dma_codes(j);
    __builtin_amdgcn_s_waitcnt(gl_vmcnt(0));
    read_codes(0, creg);
#pragma unroll
    for (int i = -(GL_NS - 1); i < 0; ++i) {
      const int q = i + GL_NS - 1;
      dma_codes(q + GL_NS);
      dma_stage(q, q, creg);
      read_codes(q + 1, creg);
    }
    int stage = 0;  // = i % NS
    int i = 0;
    for (; i + GL_NS - 1 < n; ++i) {
      __builtin_amdgcn_s_waitcnt(gl_vmcnt((GL_NS - 2) * P));  // what this wave issued NS - 1 iterations ago has landed
      __builtin_amdgcn_s_barrier();                           // chunk i is complete; the consumers are done with chunk i - 1
      const int q = i + GL_NS - 1;
      const int qstage = stage == 0 ? GL_NS - 1 : stage - 1;  // = q % NS
      dma_codes(q + GL_NS);
      dma_stage(q, qstage, creg);
      read_codes(q + 1, creg);
      stage = stage == GL_NS - 1 ? 0 : stage + 1;
    }
    static_assert(GL_NS == 4, "the tail below is written out for three iterations");
    __builtin_amdgcn_s_waitcnt(gl_vmcnt(2 * P));
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_waitcnt(gl_vmcnt(1 * P));
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_waitcnt(gl_vmcnt(0));
    __builtin_amdgcn_s_barrier();
    return;
  }

  // ============================================== consumer ==============================================================
  // register blocking: a wave owns RT row tiles x CT batch tiles (2 x NBT / 2 from two batch tiles on): per k step
  // RT + CT fragment reads feed RT * CT MFMAs -- the consumers' ds_reads share the LDS port with the landing DMA
  constexpr int RT = NBT >= 2 ? 2 : 1, CT = NBT / RT;
  static_assert(RT * CT == NBT, "batch tiles split evenly");
  const int rp = wave % (GL_WAVES / RT), bh = wave / (GL_WAVES / RT);  // row-tile group, batch-tile group
  f32x4 acc[RT][CT];
#pragma unroll
  for (int j = 0; j < RT; ++j)
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int stage = 0;
  for (int c = 0; c < n; ++c) {
    __builtin_amdgcn_s_barrier();
    const uint32_t base = (uint32_t)stage * LDS::STAGE;
    // all fragment reads of the chunk are issued before the first MFMA (left alone, hipcc pairs every read with an
    // lgkmcnt(0) and the wave pays one LDS latency per MFMA)
    if (p.dbg & 2) continue;
    u32x4 a[2][RT], b[2][CT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int j = 0; j < RT; ++j)
        a[s][j] = *(glds_u32x4_ptr)(size_t)(base + (uint32_t)(rp * RT + j) * 2048u + (uint32_t)s * 1024u + (uint32_t)lane * 16u);
#pragma unroll
      for (int t = 0; t < CT; ++t)
        b[s][t] = *(glds_u32x4_ptr)(size_t)(base + LDS::W_BYTES + (uint32_t)xswz((bh * CT + t) * 16 + arow, s * 4 + kg) * 16u);
    }
    if (p.dbg & 1) {  // reads kept alive, no matrix work
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < RT; ++j)
#pragma unroll
          for (int t = 0; t < CT; ++t) acc[j][t][0] += __uint_as_float((a[s][j].x ^ b[s][t].y) & 0x007fffffu);
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < RT; ++j)
#pragma unroll
          for (int t = 0; t < CT; ++t) acc[j][t] = mfma16<T>(a[s][j], b[s][t], acc[j][t]);
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * (RT + CT), 0);  // DS reads first ...
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NBT, 0);        // ... then the MFMAs
    }
    stage = stage == GL_NS - 1 ? 0 : stage + 1;
  }

  // ---- epilogue: lane (arow, kg) holds rows 4 kg .. 4 kg + 3 of row tile rp RT + j, batch column 16 (bh CT + t) + arow ------
  if (p.dbg & 4) {  // no stores (one lane keeps the accumulators alive)
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < RT; ++j)
#pragma unroll
      for (int t = 0; t < CT; ++t) v += acc[j][t][0] + acc[j][t][1] + acc[j][t][2] + acc[j][t][3];
    if (v == 1.2345e-30f) p.partial[0] = v;
    return;
  }
  const bool vec = (p.M & 3) == 0;  // 16-B aligned partial rows / 8-B aligned Y rows
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int m = row_blk * 128 + (rp * RT + j) * 16 + kg * 4;
    if (p.ksplit > 1) {
      float* out = p.partial + (size_t)ks * p.B * p.M;
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int b = (bh * CT + t) * 16 + arow;
        if (b < p.B && m < p.M) {
          float* dst = out + (size_t)b * p.M + m;
          if (vec) {
            if (p.store_nt) __builtin_nontemporal_store(acc[j][t], reinterpret_cast<f32x4*>(dst));
            else *reinterpret_cast<f32x4*>(dst) = acc[j][t];
          } else
            for (int r = 0; r < 4; ++r)
              if (m + r < p.M) dst[r] = acc[j][t][r];
        }
      }
    } else {
      float sc[4], bi[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = m + r < p.M ? m + r : p.M - 1;
        sc[r] = T::to_float(p.scales[mm]);
        bi[r] = p.bias ? T::to_float(p.bias[mm]) : 0.f;
      }
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int b = (bh * CT + t) * 16 + arow;
        if (b < p.B && m < p.M) {
          uint16_t* dst = p.Y + (size_t)b * p.ys + m;
          uint16_t h[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) h[r] = T::from_float(__builtin_fmaf(acc[j][t][r], sc[r], bi[r]));
          if (vec && (p.ys & 3) == 0 && ((uintptr_t)dst & 7u) == 0) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
          else
            for (int r = 0; r < 4; ++r)
              if (m + r < p.M) dst[r] = h[r];
        }
      }
    }
  }
}

// Y[b][m] = (sum_ks partial[ks][b][m]) * scales[m] + bias[m]: thread = 4 consecutive m of one batch row, all K slices
// requested before the first add.  Blocks are mapped like the main kernel's (row block -> XCD row_blk % 8), so the
// partials are read from the L2 they were written to (speed only).
struct GldsFinalizeParams {
  const float* partial;
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  long ys;
  int M, B, ksplit, row_blocks, bchunks, rb_rows;  // rb_rows: rows of a row block (128 or 64), 32 threads x 4 rows cover 128
};

template <class T>
__global__ __launch_bounds__(256) void gemm_glds_finalize_kernel(const GldsFinalizeParams p) {
  const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
  const int rb_hi = slot / p.bchunks;
  const int row_blk = rb_hi * 8 + xcd, bc = slot - rb_hi * p.bchunks;
  if (row_blk >= p.row_blocks) return;
  // a block covers 128 consecutive rows: one row block of the main kernel, or two of its 64-row blocks (same XCD pairing
  // is not attempted for those: speed only)
  const int m = row_blk * 128 + ((int)threadIdx.x & 31) * 4;
  const int b = bc * 8 + ((int)threadIdx.x >> 5);
  if (m >= p.M || b >= p.B) return;
  const size_t plane = (size_t)p.B * p.M;
  const float* src = p.partial + (size_t)b * p.M + m;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  float sc[4], bi[4];  // requested before the partials: one exposed round trip instead of two
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mm = m + r < p.M ? m + r : p.M - 1;
    sc[r] = T::to_float(p.scales[mm]);
    bi[r] = p.bias ? T::to_float(p.bias[mm]) : 0.f;
  }
  if ((p.M & 3) == 0) {
    int k = 0;
    for (; k + 8 <= p.ksplit; k += 8) {
      f32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(k + j) * plane);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += v[j][r];
    }
    for (; k < p.ksplit; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)k * plane);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] += v[r];
    }
  } else {
    for (int k = 0; k < p.ksplit; ++k)
      for (int r = 0; r < 4; ++r)
        if (m + r < p.M) s[r] += src[(size_t)k * plane + r];
  }
  uint16_t h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = T::from_float(__builtin_fmaf(s[r], sc[r], bi[r]));
  uint16_t* dst = p.Y + (size_t)b * p.ys + m;
  if ((p.M & 3) == 0 && (p.ys & 3) == 0 && ((uintptr_t)dst & 7u) == 0) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
  else
    for (int r = 0; r < 4; ++r)
      if (m + r < p.M) dst[r] = h[r];
}

struct GldsPlan {
  int row_blocks, ksplit, chunks_base, chunks_rem, nbt, xw;
};

// K split: enough blocks for one round of the chip, K slices of >= 8 chunks (512 k) where K allows, never fewer than
// NS - 1 chunks (the pipeline's prologue), chunks dealt evenly.
static bool plan_glds(int B, int M, int K, GldsPlan& g) {
  const int kchunks = K / BK;
  if (K % BK != 0 || kchunks < GL_NS - 1 || B < 1 || B > 128) return false;
  g.row_blocks = (M + 127) / 128;
  int ksplit = std::max(1, 256 / g.row_blocks);
  ksplit = std::min(ksplit, std::max(1, kchunks / 8));
  ksplit = std::min(ksplit, kchunks / (GL_NS - 1));
  g.ksplit = std::max(1, ksplit);
  g.chunks_base = kchunks / g.ksplit;
  g.chunks_rem = kchunks % g.ksplit;
  const int nbt = (B + 15) / 16;
  g.nbt = nbt <= 2 ? nbt : (nbt <= 4 ? 4 : (nbt <= 6 ? 6 : 8));
  g.xw = g.nbt <= 4 ? 1 : 2;
  return true;
}

template <class T, int G>
static int launch_glds(const GldsParams& p, const GldsPlan& g, hipStream_t stream) {
  const int rb8 = ((p.M + 127) / 128 + 7) / 8;  // 128-row groups per XCD
  const dim3 grid((unsigned)(8 * rb8 * p.ksplit));
  auto go = [&](auto kern, size_t lds) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3((GL_WAVES + GL_PRODUCERS) * 64), lds, stream, p);
    return check_hip(hipGetLastError(), "gemm_1x16_glds launch");
  };
  switch (g.nbt) {
    case 1: return go(gemm_1x16_glds_kernel<T, G, 1, 1>, GldsLds<1>::TOTAL);
    case 2: return go(gemm_1x16_glds_kernel<T, G, 2, 1>, GldsLds<1>::TOTAL);
    case 4: return go(gemm_1x16_glds_kernel<T, G, 4, 1>, GldsLds<1>::TOTAL);
    case 6: return go(gemm_1x16_glds_kernel<T, G, 6, 2>, GldsLds<2>::TOTAL);
    default: return go(gemm_1x16_glds_kernel<T, G, 8, 2>, GldsLds<2>::TOTAL);
  }
}

// The K slices meet: partial[ksplit][B][M] -> Y, summed in slice order, scaled, biased, rounded once.  Also the second launch of the
// K-split form of gemm_kx8_rows16_kernel, which leaves its partials in the same layout; `what` labels a launch that fails.
static int launch_glds_finalize(int dtype, const void* partial, const void* scales, const void* bias, uint16_t* Y, long ys, int M, int B,
                                int ksplit, hipStream_t stream, const char* what) {
  GldsFinalizeParams f{};
  f.partial = (const float*)partial;
  f.scales = (const uint16_t*)scales;
  f.bias = (const uint16_t*)bias;
  f.Y = Y;
  f.ys = ys;
  f.M = M;
  f.B = B;
  f.ksplit = ksplit;
  f.row_blocks = (M + 127) / 128;
  f.bchunks = (B + 7) / 8;
  f.rb_rows = 128;
  const dim3 grid((unsigned)(8 * ((f.row_blocks + 7) / 8) * f.bchunks));
  if (dtype == AQLM_HIP_F16) hipLaunchKernelGGL(gemm_glds_finalize_kernel<F16>, grid, dim3(256), 0, stream, f);
  else hipLaunchKernelGGL(gemm_glds_finalize_kernel<BF16>, grid, dim3(256), 0, stream, f);
  return check_hip(hipGetLastError(), what);
}

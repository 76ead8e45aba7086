// Part of gemm_mfma.hip (read there, inside namespace aqlm): the streaming 16-row kernel of the K x 8-bit schemes, its plan and launch.
// ---------------------------------------------------------------------------------------------------------------------------
// K x 8-bit schemes, large batch (round 4): Y = X W^T with W never materialised.  Replaces (behaviour) Code2x8Dequant /
// CodeKx8Dequant + F::linear + the epilogue launches of code2x8_matmat_dequant / code1x8_matmat_dequant
// (cuda_kernel.cpp:450-484, 615-649).  Unlike 1x16 there is no gather floor: the codebooks (K x 4 KiB) live in LDS, so a weight
// vector costs an LDS read, and 2-bit codes + the streamed X are all that moves: the op is FASTER than a dense fp16 GEMM at every
// batch size it takes.  Same frame as the 16-row kernel above (a block owns 16 output rows over all of K; X by LDS-DMA into a
// ring of steps; one barrier per step), but the four compute waves split K, not the batch: within a step of 2 CPB k-steps (32 k
// each) wave c takes k-steps c, c + 4, ...; for each it reads its lane's code (row = lane % 16, group = 4 t + lane / 16: K bytes,
// prefetched 3 steps ahead in registers), gathers the K codebook vectors from LDS -- each IS a lane of a 16 x 32 MFMA A fragment
// -- and multiplies each with every batch tile of the step's X: the K terms of a weight meet in the fp32 accumulator (K MFMAs per
// tile; the matrix cores have room), so W is never rounded -- exact fp16 / bf16 products summed in fp32, like the matvec kernels.  The four partial accumulators meet in LDS at the end in wave order (deterministic), then
// scale + bias + one rounding.
constexpr int KX_NC = 4;   // compute waves
constexpr int KX_PD = 3;   // steps the codes are requested ahead

template <int K, int NBT, int CPB, int RT>
struct KxLds {
  static constexpr int NXP = 2 * NBT >= 4 ? 4 : 2 * NBT;            // X producer waves
  static constexpr int PXW = CPB * 2 * NBT / NXP;                   // 1-KiB pieces (8 batch rows x 64 k) per X wave and step
  static constexpr uint32_t X_CHUNK = (uint32_t)NBT * 2048u;
  static constexpr uint32_t X_STAGE = CPB * X_CHUNK;
  static constexpr int NSX = CPB == 4 ? (NBT <= 1 ? 4 : 3) : (NBT <= 4 ? 4 : 3);
  static constexpr uint32_t CB = 0;                                 // [K][256][16 B]
  static constexpr uint32_t X = (uint32_t)K * 4096u;
  static constexpr uint32_t TOTAL = X + NSX * X_STAGE;
  static constexpr uint32_t RED = X;                                // [KX_NC][RT][NBT][1 KiB] fp32 partial tiles, after the last step
  static constexpr int WAVES = NXP + KX_NC;
  static_assert(KX_NC * RT * NBT * 1024u <= NSX * X_STAGE, "the reduction reuses the X ring");
  static_assert(TOTAL <= 160u * 1024u, "LDS");
};

struct KxParams {
  const uint8_t* codes;      // [M][in_groups][K] u8
  const uint8_t* codebooks;  // [K][256][8] halfs
  const uint16_t* X;         // [B][xs]
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  long xs, ys;
  int M, B, in_groups, nsteps;  // nsteps = steps of 64 CPB features of ONE K slice
  // K split (round 5): block = (row block blockIdx.x % row_blocks, K slice blockIdx.x / row_blocks); with ksplit > 1 the block leaves
  // its fp32 tile in partial[ks][b][m] and gemm_glds_finalize_kernel sums the slices, scales, adds the bias and rounds once
  float* partial;
  int ksplit, row_blocks;
};

// RT = 16-row tiles per block: every block streams all of X through its L1, so tall layers (>= 8192 rows: still >= 256 blocks)
// take two tiles per block -- half the X traffic, every X fragment feeds two MFMAs.
template <class T, int K, int NBT, int CPB, int RT>
__global__ __launch_bounds__((KxLds<K, NBT, CPB, RT>::WAVES * 64)) void gemm_kx8_rows16_kernel(const KxParams p) {
  using LDS = KxLds<K, NBT, CPB, RT>;
  constexpr int NSX = LDS::NSX;
  extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)glds_smem != 0u) __builtin_trap();  // LDS map above starts at 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = lane & 15, kg = lane >> 4;
  const int ks = p.ksplit > 1 ? (int)blockIdx.x / p.row_blocks : 0;
  const int row0 = (p.ksplit > 1 ? (int)blockIdx.x - ks * p.row_blocks : (int)blockIdx.x) * (16 * RT);
  const int n = p.nsteps;  // >= NSX - 1 (host)
  const size_t s0 = (size_t)ks * (size_t)n;  // first step of this block's K slice

  if (wave < LDS::NXP) {
    // ============================================== X producer =======================================================
    constexpr int PX = LDS::PXW;
    constexpr int PPC = 2 * NBT;  // pieces per chunk
    static_assert((NSX - 2) * PX < 64, "vmcnt is 6 bits");
    const uint8_t* x_src[PX];
    uint32_t x_dst[PX];
#pragma unroll
    for (int x = 0; x < PX; ++x) {
      const int piece = wave * PX + x;
      const int u = piece / PPC, pc = piece % PPC;
      const int s = pc * 64 + lane;  // slot of the chunk image: batch row s >> 3, k piece (s & 7) ^ swizzle
      int b = s >> 3;
      const int c = (s & 7) ^ ((b >> 1) & 7);
      b = b < p.B ? b : p.B - 1;
      x_src[x] = (const uint8_t*)(p.X + (size_t)b * p.xs + c * 8) + (size_t)u * 128;
      x_dst[x] = LDS::X + (uint32_t)u * LDS::X_CHUNK + (uint32_t)pc * 1024u;
    }
    auto dma_x = [&](int step, int stage) {
      const int cc = step < n ? step : n - 1;
#pragma unroll
      for (int x = 0; x < PX; ++x)
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(x_src[x] + (s0 + (size_t)cc) * (128 * CPB)),
                                         (glds_void_ptr)(size_t)(x_dst[x] + (uint32_t)stage * LDS::X_STAGE), 16, 0, 0);
    };
    for (int q = 0; q < NSX - 1; ++q) dma_x(q, q);
    __builtin_amdgcn_s_barrier();  // the codebooks are in LDS (compute waves)
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

  // ================================================ compute =============================================================
  const int cw = wave - LDS::NXP;
  constexpr int KS = 2 * CPB / KX_NC;  // k-steps of a step per wave: k-step t = cw + 4 j
  static_assert(KS >= 1 && KS * KX_NC == 2 * CPB, "k-steps deal evenly");
  // codebooks -> LDS (the compute waves only: the X waves are already streaming)
  for (int i = tid - LDS::NXP * 64; i < K * 256; i += KX_NC * 64)
    *reinterpret_cast<u32x4*>(glds_smem + LDS::CB + (uint32_t)i * 16u) = reinterpret_cast<const u32x4*>(p.codebooks)[i];
  // this lane's codes: row (tile rt) arow, group (step * 8 CPB) + 4 t + kg -> K bytes; requested KX_PD steps ahead, static ring slots
  const uint8_t* code_base[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int r = row0 + rt * 16 + arow;
    r = r < p.M ? r : p.M - 1;
    code_base[rt] = p.codes + ((size_t)r * p.in_groups + kg) * K;
  }
  auto load_codes = [&](int step, uint32_t (&c)[RT][KS]) {  // unconditional; steps past the end re-read the last one
    const int cc = step < n ? step : n - 1;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        const uint8_t* src = code_base[rt] + ((s0 + (size_t)cc) * (8 * CPB) + 4 * (cw + KX_NC * j)) * K;
        if constexpr (K == 2) c[rt][j] = *reinterpret_cast<const uint16_t*>(src);
        else c[rt][j] = *src;
      }
  };
  uint32_t cring[KX_PD][RT][KS];
#pragma unroll
  for (int q = 0; q < KX_PD; ++q) load_codes(q, cring[q]);
  f32x4 acc[RT][NBT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NBT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // codebooks visible to every compute wave

  int sx = 0;
  auto do_step = [&](const uint32_t (&c)[RT][KS]) {
    __builtin_amdgcn_s_barrier();  // the step's X has landed; everybody is done with the stage that is refilled next
    const uint32_t xbase = LDS::X + (uint32_t)sx * LDS::X_STAGE;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int t = cw + KX_NC * j;  // k-step of the step: chunk t / 2, half t % 2
      u32x4 w[RT][K];  // one A fragment lane per codebook: the K terms are accumulated by K MFMAs, never summed in the storage type
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int k = 0; k < K; ++k)
          w[rt][k] = *(glds_u32x4_ptr)(size_t)(LDS::CB + (uint32_t)k * 4096u + ((c[rt][j] >> (8 * k)) & 0xffu) * 16u);
      u32x4 b[NBT];
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt)
        b[bt] = *(glds_u32x4_ptr)(size_t)(xbase + (uint32_t)(t >> 1) * LDS::X_CHUNK + (uint32_t)xswz(bt * 16 + arow, (t & 1) * 4 + kg) * 16u);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int bt = 0; bt < NBT; ++bt) acc[rt][bt] = mfma16<T>(w[rt][k], b[bt], acc[rt][bt]);
    }
    sx = sx == NSX - 1 ? 0 : sx + 1;
  };
  int i = 0;
  for (; i + KX_PD <= n; i += KX_PD) {
#pragma unroll
    for (int q = 0; q < KX_PD; ++q) {  // static ring slots: the refill lands in the registers just consumed
      do_step(cring[q]);
      load_codes(i + KX_PD + q, cring[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < KX_PD - 1; ++q)
    if (i + q < n) do_step(cring[q]);

  // ---- the four K shares meet in LDS (the X ring is free once every compute wave is past its last step) ----------------
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt)
      *reinterpret_cast<f32x4*>(glds_smem + LDS::RED + (uint32_t)((cw * RT + rt) * NBT + bt) * 1024u + (uint32_t)lane * 16u) = acc[rt][bt];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  // wave cw finishes tiles cw, cw + 4, ... of the RT x NBT output tiles: lane (arow, kg) holds rows 4 kg .. 4 kg + 3, batch column arow
  const bool vec = (p.M & 3) == 0 && (p.ys & 3) == 0 && ((uintptr_t)p.Y & 7u) == 0;  // (Y only 2- / 4-byte aligned: scalar stores)
  for (int tile = cw; tile < RT * NBT; tile += KX_NC) {
    const int rt = tile / NBT, bt = tile - rt * NBT;
    f32x4 v = *reinterpret_cast<const f32x4*>(glds_smem + LDS::RED + (uint32_t)tile * 1024u + (uint32_t)lane * 16u);
#pragma unroll
    for (int w = 1; w < KX_NC; ++w) {  // wave order: the result does not depend on who finishes
      const f32x4 o = *reinterpret_cast<const f32x4*>(glds_smem + LDS::RED + (uint32_t)(w * RT * NBT + tile) * 1024u + (uint32_t)lane * 16u);
      v = v + o;
    }
    const int m = row0 + rt * 16 + kg * 4;
    const int b = bt * 16 + arow;
    if (b < p.B && m < p.M) {
      if (p.ksplit > 1) {  // this K slice's share of the tile: fp32, summed by the finalize kernel in slice order
        float* dst = p.partial + ((size_t)ks * p.B + b) * p.M + m;
        if ((p.M & 3) == 0) *reinterpret_cast<f32x4*>(dst) = v;
        else
          for (int r = 0; r < 4; ++r)
            if (m + r < p.M) dst[r] = v[r];
        continue;
      }
      uint16_t* dst = p.Y + (size_t)b * p.ys + m;
      uint16_t h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = m + r < p.M ? m + r : p.M - 1;
        const float sc = T::to_float(p.scales[mm]), bi = p.bias ? T::to_float(p.bias[mm]) : 0.f;
        h[r] = T::from_float(__builtin_fmaf(v[r], sc, bi));
      }
      if (vec) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
      else
        for (int r = 0; r < 4; ++r)
          if (m + r < p.M) dst[r] = h[r];
    }
  }
}

struct KxPlan {
  int nbt, cpb, rt, nsteps, ksplit;  // nsteps: per K slice
};

constexpr int KX_MAX_KSPLIT = 4;

// `can_split`: the caller gave a workspace for fp32 partials (aqlm_hip_gemm_kx8_mfma_ws).
static bool plan_kx8(int B, int M, int Kf, KxPlan& r, bool can_split = false) {
  if (Kf % (2 * BK) != 0 || B < 1 || B > 128) return false;
  const int t = (B + 15) / 16;
  r.nbt = t <= 1 ? 1 : (t <= 2 ? 2 : (t <= 4 ? 4 : 8));
  const int chunks = Kf / BK;
  // (steps of 4 chunks at 64 / 128 rows -- X ring of 3 x 32 / 2 x 64 KiB -- measured in round 5: 4096^2 at 64 rows 13.4 -> 12.0 us, every other
  // shape and 128 rows equal or up to 16 % slower, profiles/r05_gemm_kx8_steps_of_4_chunks.log: not kept)
  r.cpb = (r.nbt <= 2 && chunks % 4 == 0) ? 4 : 2;
  r.nsteps = chunks / r.cpb;
  r.ksplit = 1;
  // two row tiles per block where that still fills the chip AND X is what the block mostly moves (measured, 4096 -> 11008: 128 rows
  // 46.5 -> 39.6 us, 64 rows 28.5 -> 26.9, but 16 rows 18.2 -> 20.8: 344 blocks are 1.3 rounds of the chip)
  r.rt = ((M + 31) / 32 >= 256 && r.nbt >= 4) ? 2 : 1;
  if (r.nsteps < 3) return false;  // the X ring's prologue (NSX <= 4)
  // K split (round 5, given a workspace): the K range dealt to 2 / 4 blocks whose fp32 tiles a finalize launch sums (+ ~3 us).  Measured
  // (profiles/r05_gemm_kx8_ksplit.log, 2x8 g8, 128 rows, us; no split -> split): it pays (a) where the layer has too few rows to fill the
  // chip -- 4096 -> 1024: 64 blocks, 15.2 -> 11.0 with 4 slices of one tile -- and (b) on long K with two tiles per block, where a step's
  // X fragments feed twice the MFMAs -- 11008 -> 4096: 45.7 -> 35.0 (64 rows: 37.5 -> 24.7); it does NOT pay at 4096 x 4096 (16.6 -> 18.0:
  // a 32-step block is not X-bound, the finalize is pure cost) nor where two tiles per block already fill the chip (8192 x 8192).
  const int force_ks = tuning().kx8_ksplit, force_rt = tuning().kx8_rt;
  if (can_split && r.nbt >= 4 && force_ks != 1) {
    const int rb16 = (M + 15) / 16, rb32 = (M + 31) / 32;
    int rt = 0, ks = 1;
    if (force_ks > 1) {
      rt = force_rt == 1 ? 1 : 2;
      ks = force_ks;
    } else if (rb16 <= 128) {
      rt = 1;
      ks = std::min(KX_MAX_KSPLIT, 256 / rb16);
    } else if (Kf >= 8192 && rb32 < 256) {
      rt = 2;
      ks = std::min(KX_MAX_KSPLIT, std::max(1, 256 / rb32));
    }
    while (ks > 1 && (r.nsteps % ks != 0 || r.nsteps / ks < 3)) --ks;
    if (ks > 1) {
      r.rt = rt;
      r.ksplit = ks;
      r.nsteps /= ks;
    }
  } else if (force_rt == 1 || force_rt == 2) {
    r.rt = force_rt;
  }
  return true;
}

template <class T, int K>
static int launch_kx8(const KxParams& p, const KxPlan& r, hipStream_t stream) {
  const dim3 grid((unsigned)(((p.M + 16 * r.rt - 1) / (16 * r.rt)) * r.ksplit));
  auto go = [&](auto kern, size_t lds, int waves) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(waves * 64), lds, stream, p);
    return check_hip(hipGetLastError(), "gemm_kx8_rows16 launch");
  };
#define AQLM_KX_CASE(NBT_, CPB_, RT_) return go(gemm_kx8_rows16_kernel<T, K, NBT_, CPB_, RT_>, KxLds<K, NBT_, CPB_, RT_>::TOTAL, KxLds<K, NBT_, CPB_, RT_>::WAVES)
#define AQLM_KX_RT(NBT_, CPB_)        \
  do {                                \
    if (r.rt == 2) AQLM_KX_CASE(NBT_, CPB_, 2); \
    AQLM_KX_CASE(NBT_, CPB_, 1);      \
  } while (0)
  if (r.cpb == 4) {
    if (r.nbt == 1) AQLM_KX_RT(1, 4);
    AQLM_KX_RT(2, 4);
  }
  switch (r.nbt) {
    case 1: AQLM_KX_RT(1, 2);
    case 2: AQLM_KX_RT(2, 2);
    case 4: AQLM_KX_RT(4, 2);
    default: AQLM_KX_RT(8, 2);
  }
#undef AQLM_KX_RT
#undef AQLM_KX_CASE
}

// Part of gemm_mfma.hip (read there, after `using namespace aqlm`): the X-resident kernels of the K x 8-bit schemes -- whole image and
// phased -- with the rule that says which calls fit and their launches.
// ---------------------------------------------------------------------------------------------------------------------------
// K x 8-bit schemes at <= 16 batch rows (round 5): X RESIDENT in LDS.  The 16-row kernel above streams all of X through every
// block's L1 and LDS (128 KiB per 16 output rows at 4096 features) behind one barrier per step; traced at 16 rows it spent its
// time in that chain (8.1 us for ~1 us of bytes on 4096 x 4096, 18 us on 4096 -> 11008: 688 blocks x 128 KiB of X).  For the
// batches that matter most here -- the 3..8 rows of a decode call, a 16-row speculative verify -- X is SMALL: B rows x K x 2 bytes
// (<= 128 KiB) fit the LDS next to the codebooks.  So a workgroup loads X ONCE (LDS-DMA, all 8 waves), then walks its 16-row
// output tiles (tile = blockIdx.x, += gridDim.x) with NOTHING left to synchronise inside a tile: the 8 waves split K, each runs
// code (8 B per lane: its row's 4 consecutive groups = 4 k-steps) -> 2 K codebook gathers + 1 X fragment per k-step -> MFMA chains
// on two accumulators, the partial tiles meet in LDS (double-buffered: one barrier per tile) and wave 0 scales, adds the bias,
// rounds once and stores while the others are already in the next tile.  The k-step -> group mapping is the lane's own
// (k-step j of quad q = groups 16 q + 4 kg + j for lane piece kg): A and B fragments only have to agree on it.
// X image: [64-k chunk][row b < B][8 pieces of 16 B], piece index XOR-ed with s(b) = ((b >> 1) & 7) ^ ((b & 8) >> 1): the 16 lanes
// of every LDS service group read 16 distinct bank groups (rows >= B read row B - 1: same address, broadcast).
// Numerics: exact products, fp32 sums (per wave over its quads in order, then the 8 waves in wave order): a row's bits do not
// depend on the other rows of the call, nor on B.
constexpr int KR_NW = 8;
constexpr int KR_MAX_SEG = AQLM_HIP_MAX_SEGMENTS;

// One layer, or (round 5) up to KR_MAX_SEG layers that multiply the SAME X (q / k / v, gate / up: aqlm_hip_gemv_kx8_multi): the X
// image is loaded once, every layer's codebooks (K x 4 KiB each) sit side by side in LDS, and the tile walk runs over the layers'
// tiles back to back (tile -> layer by three comparisons).  A tile's arithmetic does not know about the other layers: outputs are
// bit-identical to separate launches.
struct KrSeg {
  const uint8_t* codes;      // [M][in_groups][K] u8
  const uint8_t* codebooks;  // [K][256][8] halfs
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  long ys;
  int M;
  int tile0;                 // first tile of the layer in the launch's tile sequence
};

template <int NSEG>
struct KrParams {
  KrSeg seg[NSEG];
  const uint16_t* X;         // [B][xs]
  long xs;
  int B, in_groups, ntiles, nseg;
};

template <int K>
struct KrLds {  // sized by the number of layers of the launch: two layers leave room for a second workgroup per CU where four would not
  static constexpr uint32_t CB = 0;                                                        // [layer][K][256][16 B]
  static constexpr uint32_t red(int nseg) { return (uint32_t)nseg * K * 4096u; }          // [2][KR_NW][64 lanes][16 B] fp32 partial tiles
  static constexpr uint32_t x(int nseg) { return red(nseg) + 2u * KR_NW * 1024u; }        // the X image, rounded up to whole KiB (DMA granularity)
  static size_t total(int B, int in_features, int nseg) { return (size_t)x(nseg) + (((size_t)B * in_features * 2 + 1023) & ~(size_t)1023); }
};

__device__ __forceinline__ uint32_t kr_swz(uint32_t b) { return ((b >> 1) & 7u) ^ ((b & 8u) >> 1); }

template <class T, int K, int NSEG>
__global__ __launch_bounds__(KR_NW * 64) void gemm_kx8_xres_kernel(const KrParams<NSEG> p) {
  using LDS = KrLds<K>;
  extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)glds_smem != 0u) __builtin_trap();  // LDS map above starts at 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = lane & 15, kg = lane >> 4;
  const uint32_t B = (uint32_t)p.B;
  const int nquads = p.in_groups >> 4;  // 128 k each (host: in_features % 128 == 0)
  const uint32_t lds_red = LDS::red(NSEG == 1 ? 1 : p.nseg), lds_x = LDS::x(NSEG == 1 ? 1 : p.nseg);
  auto seg_of = [&](int tile) -> int {  // wave-uniform
    if constexpr (NSEG == 1) return 0;
    else return (int)(tile >= p.seg[1].tile0) + (int)(tile >= p.seg[2].tile0) + (int)(tile >= p.seg[3].tile0);  // (absent layers: tile0 = ntiles)
  };

  // ---- prologue: codebooks and the whole of X by LDS-DMA; the first tile's codes are requested before anything is waited for
  for (int i = wave; i < K * 4 * (NSEG == 1 ? 1 : p.nseg); i += KR_NW) {
    const int sg = i / (K * 4), off = i - sg * (K * 4);
    __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(p.seg[sg].codebooks + (size_t)off * 1024 + lane * 16),
                                     (glds_void_ptr)(size_t)(LDS::CB + (uint32_t)i * 1024u), 16, 0, 0);
  }
  {
    // piece q = (chunk c, row b, 16-byte piece sl) = (q / ppc, (q % ppc) / 8, q % 8).  ONE division per lane; after that (c, r) are
    // stepped by the quotient and remainder of the 512 pieces all waves advance together, and the source is a 32-bit byte offset
    // (host: 16 rows x the row stride fit): the first cut recomputed q / ppc and a 64-bit b * xs per KiB -- ~33 VALU instructions
    // with quarter-rate multiplies, 16 times per wave at 16 rows, which the fill had to wait for (counters: VALU 2.2 us per SIMD)
    const uint32_t ppc = B * 8u;                                  // pieces per chunk
    const uint32_t npieces = (uint32_t)(p.in_groups >> 3) * ppc;  // chunks x rows x 8
    const uint32_t dq = (KR_NW * 64u) / ppc, dr = (KR_NW * 64u) - dq * ppc;
    const uint32_t xs2 = (uint32_t)p.xs * 2u;                     // bytes per row of X (< 2^24: host)
    uint32_t q = (uint32_t)wave * 64u + (uint32_t)lane;
    uint32_t c = q / ppc, r = q - c * ppc;
    const uint8_t* xb = (const uint8_t*)p.X;
    for (uint32_t q0 = (uint32_t)wave * 64u; q0 < npieces; q0 += KR_NW * 64u) {
      const bool in = q < npieces;  // (the last KiB may be partly padding: any valid source will do)
      const uint32_t cc = in ? c : 0u, rr = in ? r : 0u;
      const uint32_t b = rr >> 3, sl = rr & 7u;
      const uint32_t off = (b & 0xffu) * (xs2 & 0xffffffu) + cc * 128u + ((sl ^ kr_swz(b)) << 4);
      __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(xb + off), (glds_void_ptr)(size_t)(lds_x + q0 * 16u), 16, 0, 0);
      q += KR_NW * 64u;
      c += dq;
      r += dr;
      if (r >= ppc) {
        r -= ppc;
        c += 1u;
      }
    }
  }
  const uint32_t brow = (uint32_t)arow < B ? (uint32_t)arow : B - 1u;  // batch column of this lane's B fragments
  const uint32_t bsw = kr_swz(brow);
  typedef typename std::conditional<K == 2, u32x2, uint32_t>::type code_t;
  auto code_ptr = [&](int tile, int quad) -> const code_t* {
    const int sg = seg_of(tile);
    int r = (tile - p.seg[sg].tile0) * 16 + arow;
    r = r < p.seg[sg].M ? r : p.seg[sg].M - 1;
    return reinterpret_cast<const code_t*>(p.seg[sg].codes + ((size_t)r * p.in_groups + (size_t)quad * 16 + (size_t)kg * 4) * K);
  };
  int tile = (int)blockIdx.x;
  code_t cnext{};
  if (tile < p.ntiles && wave < nquads) cnext = *code_ptr(tile, wave);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // X and the codebooks are in LDS, for good

  int buf = 0;
  for (; tile < p.ntiles; tile += (int)gridDim.x) {
    const int sg = seg_of(tile);
    const uint32_t cb = LDS::CB + (uint32_t)sg * (uint32_t)(K * 4096);  // this layer's codebooks
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int quad = wave; quad < nquads; quad += KR_NW) {
      const code_t cw = cnext;
      // the next code word of this wave: the next quad of the tile, else the first quad of its next tile
      {
        int nq = quad + KR_NW, nt = tile;
        if (nq >= nquads) { nq = wave; nt = tile + (int)gridDim.x; }
        if (nt < p.ntiles && nq < nquads) cnext = *code_ptr(nt, nq);
      }
      uint32_t cwords[2];
      if constexpr (K == 2) { cwords[0] = cw.x; cwords[1] = cw.y; } else { cwords[0] = cw; cwords[1] = 0u; }
      u32x4 w[4][K], xb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const uint32_t byte = K == 2 ? (cwords[j >> 1] >> (16 * (j & 1) + 8 * k)) & 0xffu : (cwords[0] >> (8 * j)) & 0xffu;
          w[j][k] = *(glds_u32x4_ptr)(size_t)(cb + (uint32_t)k * 4096u + byte * 16u);
        }
        const uint32_t c = (uint32_t)quad * 2u + (uint32_t)(kg >> 1), pc = (uint32_t)(kg & 1) * 4u + (uint32_t)j;
        xb[j] = *(glds_u32x4_ptr)(size_t)(lds_x + ((c * B + brow) * 8u + (pc ^ bsw)) * 16u);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[(j * K + k) & 1] = mfma16<T>(w[j][k], xb[j], acc[(j * K + k) & 1]);
    }
    // ---- the eight K shares meet in LDS; wave 0 finishes the tile while the others start the next one
    const f32x4 mine = acc[0] + acc[1];
    *reinterpret_cast<f32x4*>(glds_smem + lds_red + (uint32_t)(buf * KR_NW + wave) * 1024u + (uint32_t)lane * 16u) = mine;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wave == 0) {
      f32x4 v = mine;
#pragma unroll
      for (int w8 = 1; w8 < KR_NW; ++w8)  // wave order: the result does not depend on who finishes first
        v = v + *reinterpret_cast<const f32x4*>(glds_smem + lds_red + (uint32_t)(buf * KR_NW + w8) * 1024u + (uint32_t)lane * 16u);
      const KrSeg& S = p.seg[sg];
      const int m = (tile - S.tile0) * 16 + kg * 4;
      const int b = arow;
      if (b < p.B && m < S.M) {
        uint16_t* dst = S.Y + (size_t)b * S.ys + m;
        uint16_t h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mm = m + r < S.M ? m + r : S.M - 1;
          const float sc = T::to_float(S.scales[mm]), bi = S.bias ? T::to_float(S.bias[mm]) : 0.f;
          h[r] = T::from_float(__builtin_fmaf(v[r], sc, bi));
        }
        if ((S.M & 3) == 0 && (S.ys & 3) == 0 && ((uintptr_t)dst & 7u) == 0) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        else
          for (int r = 0; r < 4; ++r)
            if (m + r < S.M) dst[r] = h[r];
      }
    }
    buf ^= 1;
  }
}

// does the X-resident kernel take the call?  <= 16 rows whose image fits the LDS next to the codebooks and the partial tiles
template <int K>
static bool xres_fits(int B, int in_features, long xs, int nseg = 1) {
  return B >= 1 && B <= 16 && in_features % 128 == 0 && KrLds<K>::total(B, in_features, nseg) <= 160u * 1024u && xs > 0 && xs < (1l << 22);
}
static bool xres_fits(int K, int B, int in_features, long xs, int nseg = 1) {  // K is 1 or 2 (checked by every caller)
  return K == 2 ? xres_fits<2>(B, in_features, xs, nseg) : xres_fits<1>(B, in_features, xs, nseg);
}

static int device_cus() {
  static const int cus = [] {  // (initialised once, thread-safe; every GPU of a node is the same part)
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  return cus;
}

// one layer of a launch: `tile0` = the tiles of the layers in front of it
static KrSeg kr_seg(const void* codes, const void* codebooks, const void* scales, const void* bias, void* Y, long ys, int M, int tile0) {
  return KrSeg{(const uint8_t*)codes, (const uint8_t*)codebooks, (const uint16_t*)scales, (const uint16_t*)bias, (uint16_t*)Y, ys, M, tile0};
}

template <class T, int K, int NSEG>
static int launch_kx8_xres(const KrParams<NSEG>& p, int in_features, hipStream_t stream) {
  auto kern = gemm_kx8_xres_kernel<T, K, NSEG>;
  const size_t lds = KrLds<K>::total(p.B, in_features, p.nseg);
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
  // one workgroup per CU and as many as fit its LDS (small X: two or more share a CU and overlap their latencies)
  const int per_cu = std::max(1, std::min(4, (int)((160u * 1024u) / lds)));
  const int grid = std::min(p.ntiles, device_cus() * per_cu);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(KR_NW * 64), lds, stream, p);
  return check_hip(hipGetLastError(), "gemm_kx8_xres launch");
}

// ---------------------------------------------------------------------------------------------------------------------------
// X-resident kernel in PHASES (round 5): down-projection-shaped layers (11008 / 14336 / 28672 input features) at 7..16 rows have an X
// image of 150-900 KiB -- it does not fit the LDS, and the call fell to the streaming 16-row kernel (16.7 us for 8 rows of
// 11008 -> 4096 where 6 rows cost 10.6).  Here the image is loaded in nphases pieces of `qpp` quads (128 features each): all waves
// walk the block's one to three tiles over the quads of the piece that is resident, the fp32 accumulators of the tiles stay in
// registers across the phases (TPB x 2 x f32x4 per wave), and the K shares meet in LDS once, at the end.  The fill of a phase is
// not overlapped with the arithmetic of the previous one (one image buffer) -- it costs what the bytes cost (X once per
// workgroup) instead of the streaming kernel's step chain.  Same arithmetic per (row, quad) as gemm_kx8_xres_kernel and the
// same summation order (per wave over its quads in ascending order, then the waves in wave order): the results are bit-identical
// to the single-phase kernel's, so a row's bits still depend neither on the other rows nor on their number.
struct KpParams {
  const uint8_t* codes;      // [M][in_groups][K] u8
  const uint8_t* codebooks;  // [K][256][8] halfs
  const uint16_t* X;         // [B][xs]
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  long xs, ys;
  int M, B, in_groups, ntiles, nphases, qpp;
};

template <int K, int TPB, int NBT>
struct KpLds {
  static constexpr uint32_t CB = 0;                                        // [K][256][16 B]
  static constexpr uint32_t RED = (uint32_t)K * 4096u;                     // [KR_NW][TPB][NBT][64 lanes][16 B] fp32 partial tiles
  static constexpr uint32_t X = RED + (uint32_t)KR_NW * TPB * NBT * 1024u; // the image of one phase
  static size_t image_bytes(int B, int qpp) { return (size_t)B * qpp * 256; }
};

// NBT = 16-column batch tiles (17 .. 32 rows: two; the A fragments of a k-step feed both)
template <class T, int K, int TPB, int NBT>
__global__ __launch_bounds__(KR_NW * 64) void gemm_kx8_xres_phased_kernel(const KpParams p) {
  using LDS = KpLds<K, TPB, NBT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];
  if ((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)glds_smem != 0u) __builtin_trap();  // LDS map above starts at 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int arow = lane & 15, kg = lane >> 4;
  const uint32_t B = (uint32_t)p.B;
  const int nquads = p.in_groups >> 4;
  const int grid = (int)gridDim.x;

  if (wave < K * 4)
    __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(p.codebooks + (size_t)wave * 1024 + lane * 16),
                                     (glds_void_ptr)(size_t)(LDS::CB + (uint32_t)wave * 1024u), 16, 0, 0);
  uint32_t brow[NBT], bsw[NBT];  // batch column of this lane's B fragments, per batch tile
#pragma unroll
  for (int bt = 0; bt < NBT; ++bt) {
    brow[bt] = (uint32_t)(bt * 16 + arow) < B ? (uint32_t)(bt * 16 + arow) : B - 1u;
    bsw[bt] = kr_swz(brow[bt]);
  }
  typedef typename std::conditional<K == 2, u32x2, uint32_t>::type code_t;
  auto code_ptr = [&](int tile, int quad) -> const code_t* {
    int r = tile * 16 + arow;
    r = r < p.M ? r : p.M - 1;
    return reinterpret_cast<const code_t*>(p.codes + ((size_t)r * p.in_groups + (size_t)quad * 16 + (size_t)kg * 4) * K);
  };
  f32x4 acc[TPB][NBT][2];
#pragma unroll
  for (int ts = 0; ts < TPB; ++ts)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) acc[ts][bt][0] = acc[ts][bt][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ph = 0; ph < p.nphases; ++ph) {
    const int q_lo = ph * p.qpp, q_hi = q_lo + p.qpp < nquads ? q_lo + p.qpp : nquads;
    // wave w owns the quads = w (mod 8) whatever the phases are (the single-phase kernel's deal): the summation order of a row does
    // not depend on how the image was cut, i.e. not on the number of rows of the call
    const int q_first = q_lo + ((wave - q_lo) & (KR_NW - 1));
    // the first code word of the phase is requested before its image (it does not depend on it)
    code_t cnext{};
    if ((int)blockIdx.x < p.ntiles && q_first < q_hi) cnext = *code_ptr((int)blockIdx.x, q_first);
    if (ph > 0) __builtin_amdgcn_s_barrier();  // every wave is done with the previous image
    {
      // the image of quads [q_lo, q_hi): chunk c (64 features) of the piece, row b, 16-byte piece sl (stepped as in gemm_kx8_xres_kernel)
      const uint32_t ppc = B * 8u;
      const uint32_t npieces = (uint32_t)(q_hi - q_lo) * 2u * ppc;
      const uint32_t dq = (KR_NW * 64u) / ppc, dr = (KR_NW * 64u) - dq * ppc;
      const uint32_t xs2 = (uint32_t)p.xs * 2u;
      uint32_t q = (uint32_t)wave * 64u + (uint32_t)lane;
      uint32_t c = q / ppc, r = q - c * ppc;
      const uint8_t* xb = (const uint8_t*)p.X + (size_t)q_lo * 256;  // 128 features x 2 bytes per quad
      for (uint32_t q0 = (uint32_t)wave * 64u; q0 < npieces; q0 += KR_NW * 64u) {
        const bool in = q < npieces;
        const uint32_t cc = in ? c : 0u, rr = in ? r : 0u;
        const uint32_t b = rr >> 3, sl = rr & 7u;
        const uint32_t off = (b & 0xffu) * (xs2 & 0xffffffu) + cc * 128u + ((sl ^ kr_swz(b)) << 4);
        __builtin_amdgcn_global_load_lds((ggbl_void_ptr)(xb + off), (glds_void_ptr)(size_t)(LDS::X + q0 * 16u), 16, 0, 0);
        q += KR_NW * 64u;
        c += dq;
        r += dr;
        if (r >= ppc) {
          r -= ppc;
          c += 1u;
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the image (and, in phase 0, the codebooks) are in LDS
#pragma unroll
    for (int ts = 0; ts < TPB; ++ts) {
      const int tile = (int)blockIdx.x + ts * grid;
      if (tile >= p.ntiles) break;
      for (int quad = q_first; quad < q_hi; quad += KR_NW) {
        const code_t cw = cnext;
        {  // the next code word of this wave: the next quad of the tile, else the first quad of the block's next tile in this phase
          int nq = quad + KR_NW, nt = tile;
          if (nq >= q_hi) { nq = q_first; nt = tile + grid; }
          if (nt < p.ntiles && nt < (int)blockIdx.x + TPB * grid && nq < q_hi) cnext = *code_ptr(nt, nq);
        }
        uint32_t cwords[2];
        if constexpr (K == 2) { cwords[0] = cw.x; cwords[1] = cw.y; } else { cwords[0] = cw; cwords[1] = 0u; }
        u32x4 w[4][K], xb[4][NBT];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const uint32_t byte = K == 2 ? (cwords[j >> 1] >> (16 * (j & 1) + 8 * k)) & 0xffu : (cwords[0] >> (8 * j)) & 0xffu;
            w[j][k] = *(glds_u32x4_ptr)(size_t)(LDS::CB + (uint32_t)k * 4096u + byte * 16u);
          }
          const uint32_t c = (uint32_t)(quad - q_lo) * 2u + (uint32_t)(kg >> 1), pc = (uint32_t)(kg & 1) * 4u + (uint32_t)j;
#pragma unroll
          for (int bt = 0; bt < NBT; ++bt)
            xb[j][bt] = *(glds_u32x4_ptr)(size_t)(LDS::X + ((c * B + brow[bt]) * 8u + (pc ^ bsw[bt])) * 16u);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) acc[ts][bt][(j * K + k) & 1] = mfma16<T>(w[j][k], xb[j][bt], acc[ts][bt][(j * K + k) & 1]);
      }
    }
  }
  // ---- the eight K shares of every (row tile, batch tile) meet in LDS; wave ts NBT + bt finishes that pair
#pragma unroll
  for (int ts = 0; ts < TPB; ++ts)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt)
      *reinterpret_cast<f32x4*>(glds_smem + LDS::RED + (uint32_t)(((wave * TPB + ts) * NBT + bt) * 1024) + (uint32_t)lane * 16u) = acc[ts][bt][0] + acc[ts][bt][1];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wave < TPB * NBT) {
    const int ts = wave / NBT, bt = wave - ts * NBT, tile = (int)blockIdx.x + ts * grid;
    if (tile < p.ntiles) {
      f32x4 v = *reinterpret_cast<const f32x4*>(glds_smem + LDS::RED + (uint32_t)((ts * NBT + bt) * 1024) + (uint32_t)lane * 16u);
#pragma unroll
      for (int w8 = 1; w8 < KR_NW; ++w8)  // wave order, as in the single-phase kernel
        v = v + *reinterpret_cast<const f32x4*>(glds_smem + LDS::RED + (uint32_t)(((w8 * TPB + ts) * NBT + bt) * 1024) + (uint32_t)lane * 16u);
      const int m = tile * 16 + kg * 4;
      const int b = bt * 16 + arow;
      if (b < p.B && m < p.M) {
        uint16_t* dst = p.Y + (size_t)b * p.ys + m;
        uint16_t h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mm = m + r < p.M ? m + r : p.M - 1;
          const float sc = T::to_float(p.scales[mm]), bi = p.bias ? T::to_float(p.bias[mm]) : 0.f;
          h[r] = T::from_float(__builtin_fmaf(v[r], sc, bi));
        }
        if ((p.M & 3) == 0 && (p.ys & 3) == 0 && ((uintptr_t)dst & 7u) == 0) *reinterpret_cast<u32x2*>(dst) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        else
          for (int r = 0; r < 4; ++r)
            if (m + r < p.M) dst[r] = h[r];
      }
    }
  }
}

// plan + launch; AQLM_HIP_E_UNSUPPORTED when the layer has more tiles than four (17+ rows: three) per CU, or a phase would hold fewer than 8 quads
template <class T, int K>
static int launch_kx8_xres_phased(KpParams p, int in_features, hipStream_t stream) {
  const int cus = device_cus();
  int tpb = (p.ntiles + cus - 1) / cus;  // tiles per workgroup: 1 .. 4 (their accumulators live in registers across the phases)
  const int nbt = p.B <= 16 ? 1 : 2;
  const int exp_tpb = tuning().kx8_phase_tpb, exp_q = tuning().kx8_phase_quads;  // experiments: tiles per workgroup, quads per phase
  if (exp_tpb >= 1 && exp_tpb <= 4) tpb = exp_tpb;
  if (tpb > (nbt == 1 ? 4 : 3) || p.B > 32) return AQLM_HIP_E_UNSUPPORTED;
  const size_t fixed = (size_t)KpLds<K, 1, 1>::RED + (size_t)KR_NW * tpb * nbt * 1024u;
  const int nquads = in_features / 128;
  const int qmax = (int)((160u * 1024u - fixed) / ((size_t)p.B * 256));  // quads whose image fits
  if (qmax < KR_NW) return AQLM_HIP_E_UNSUPPORTED;
  const int qcap = exp_q >= KR_NW && exp_q < qmax ? exp_q : qmax;
  p.nphases = (nquads + qcap - 1) / qcap;
  p.qpp = (nquads + p.nphases - 1) / p.nphases;
  const size_t lds = fixed + (((size_t)p.B * p.qpp * 256 + 1023) & ~(size_t)1023);
  const int grid = (p.ntiles + tpb - 1) / tpb;
  auto go = [&](auto kern) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(KR_NW * 64), lds, stream, p);
    return check_hip(hipGetLastError(), "gemm_kx8_xres_phased launch");
  };
  if (nbt == 2) return tpb == 1 ? go(gemm_kx8_xres_phased_kernel<T, K, 1, 2>) : (tpb == 2 ? go(gemm_kx8_xres_phased_kernel<T, K, 2, 2>) : go(gemm_kx8_xres_phased_kernel<T, K, 3, 2>));
  switch (tpb) {
    case 1: return go(gemm_kx8_xres_phased_kernel<T, K, 1, 1>);
    case 2: return go(gemm_kx8_xres_phased_kernel<T, K, 2, 1>);
    case 3: return go(gemm_kx8_xres_phased_kernel<T, K, 3, 1>);
    default: return go(gemm_kx8_xres_phased_kernel<T, K, 4, 1>);
  }
}

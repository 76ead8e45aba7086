// Part of gemm_mfma.hip (read there, inside namespace aqlm): the register-staged 1x16 kernel that the header of gemm_mfma.hip describes
// (round 1; behind gemm_variant 1 and wherever the LDS-DMA pipeline has no plan), its finalize kernel, plan and launch.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <class T>
__device__ __forceinline__ f32x16 mfma32(const u32x4& a, const u32x4& b, const f32x16& c);
template <>
__device__ __forceinline__ f32x16 mfma32<F16>(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 mfma32<BF16>(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

struct GemmParams {
  const uint8_t* codes;
  const uint8_t* codebook;
  const uint16_t* X;
  float* partial;  // [ksplit][M][Bpad]
  int M, K, B, Bpad;
  int in_groups;
  int kslice;  // k elements per block (multiple of 64)
  int ksplit;
  long xs;
  int cb_bytes;
  uint32_t x_bytes;  // extent of the X slab (rows >= B read as zeros through the bounds-checked descriptor)
};


template <class T, int G, int NBT>
__global__ __launch_bounds__(256) void gemm_1x16_mfma_kernel(const GemmParams p) {
  constexpr int NROWS_X = NBT * 32;
  constexpr int PIECES = NROWS_X * 8;          // 16-B pieces per chunk
  constexpr int PER_THREAD = (PIECES + 255) / 256;
  constexpr int CODES_PER_CHUNK = BK / G;      // 8 (g8) or 4 (g16)
  constexpr int CWN = CODES_PER_CHUNK / 2;     // dwords of codes per chunk per row
  __shared__ __attribute__((aligned(16))) u32x4 xl[2][PIECES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5;
  const int row_blk = blockIdx.x / p.ksplit;
  const int ks = blockIdx.x - row_blk * p.ksplit;
  const int row_tile0 = row_blk * 128 + wave * 32;
  int my_row = row_tile0 + (lane & 31);
  const bool row_ok = my_row < p.M;
  if (!row_ok) my_row = p.M - 1;  // clamp: computed but never stored
  const int k_begin = ks * p.kslice;
  const int k_end = k_begin + p.kslice < p.K ? k_begin + p.kslice : p.K;
  const int nchunks = (k_end - k_begin + BK - 1) / BK;

  __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.codebook, 0, p.cb_bytes, 0x00020000);
  const uint8_t* code_row = p.codes + (long)my_row * p.in_groups * 2;

  f32x16 acc[NBT];
#pragma unroll
  for (int t = 0; t < NBT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // global -> register staging of one X chunk.  The loads are UNCONDITIONAL buffer loads (rows >= B and k >= k_end
  // read as zeros through the bounds-checked descriptor / an out-of-range offset): with the load under a branch hipcc
  // emitted vmcnt(0) right behind it, i.e. every chunk step first waited ~1 us for X and only then issued the
  // codebook gathers of the next chunk (traced through the ISA: one L2 latency + one gather latency per 64-deep chunk).
  __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.x_bytes, 0x00020000);
  static_assert(PIECES % 256 == 0, "the X chunk splits evenly over the block");
  u32x4 xr[2][PER_THREAD];  // X chunks run two ahead in registers, one ahead in LDS
  uint32_t xoff[PER_THREAD];
#pragma unroll
  for (int s = 0; s < PER_THREAD; ++s) {
    const int q = tid + s * 256;
    xoff[s] = (uint32_t)(((long)(q >> 3) * p.xs + k_begin + (q & 7) * 8) * 2);
  }
  auto load_x = [&](int chunk, u32x4 (&dst)[PER_THREAD]) {
#pragma unroll
    for (int s = 0; s < PER_THREAD; ++s) {
      const bool in_k = k_begin + chunk * BK + (int)((tid + s * 256) & 7) * 8 < k_end;
      dst[s] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, in_k ? xoff[s] + (uint32_t)chunk * (BK * 2) : 0xfffffff0u, 0, 0);
    }
  };
  auto store_x = [&](int buf, const u32x4 (&src)[PER_THREAD]) {
#pragma unroll
    for (int s = 0; s < PER_THREAD; ++s) {
      const int q = tid + s * 256;
      xl[buf][xswz(q >> 3, q & 7)] = src[s];
    }
  };
  const int last_chunk = nchunks - 1;
  auto load_codes = [&](int chunk, uint32_t (&cw)[CWN]) {  // unconditional: chunks past the slice re-read the last one
    chunk = chunk < last_chunk ? chunk : last_chunk;
    const int k0 = k_begin + chunk * BK;
    const uint8_t* src = code_row + (long)(k0 / G) * 2;
    if constexpr (CWN == 4) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(src);
      cw[0] = v.x; cw[1] = v.y; cw[2] = v.z; cw[3] = v.w;
    } else {
      const u32x2 v = *reinterpret_cast<const u32x2*>(src);
      cw[0] = v.x; cw[1] = v.y;
    }
  };

  // gathers: one 16-B entry per lane per 16-deep k step = 4 per 64-deep chunk; entry == MFMA A fragment
  auto gather = [&](const uint32_t (&cw)[CWN], u32x4 (&af)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      uint32_t code, piece;
      if constexpr (G == 8) {
        code = (cw[kk] >> (16 * half)) & 0xffffu;  // code index 2*kk + half
        piece = 0;
      } else {
        code = (cw[kk >> 1] >> (16 * (kk & 1))) & 0xffffu;  // code index kk, lane-half picks the 16-B half
        piece = half;
      }
      af[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, code * (uint32_t)(G * 2) + piece * 16, 0, 0);
    }
  };

  // Software pipeline, in batches of NBATCH chunks.  Inside a batch the code is straight-line (fully unrolled, static
  // ring slots): all code words of the batch are requested up front, codebook gathers run GD-1 = 3 chunks ahead of
  // the MFMAs that consume them (one 64-deep chunk of MFMAs is ~0.3 us, an L2 gather ~1.5 us under load: a distance of
  // one chunk left every step waiting for its own gathers), X runs two chunks ahead in registers and one in LDS, and
  // NOTHING is in flight across the loop back-edge: hipcc's wait-count pass merges the prologue and back-edge states at
  // a loop header and then waits with vmcnt(0) for every register loaded in the previous iteration.  A batch pays one
  // pipeline refill instead (none at all for K slices of <= NBATCH chunks, e.g. 4096 x 4096 with the 8-way K split).
  constexpr int NBATCH = 8, GD = 4;
  uint32_t cw[NBATCH][CWN];
  u32x4 af[GD][4];
  auto mfmas = [&](int buf, const u32x4 (&af_cur)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int t = 0; t < NBT; ++t) {
        const u32x4 bfrag = xl[buf][xswz(t * 32 + (lane & 31), kk * 2 + half)];
        acc[t] = mfma32<T>(af_cur[kk], bfrag, acc[t]);
      }
    }
  };
  for (int base = 0; base < nchunks; base += NBATCH) {
#pragma unroll
    for (int c = 0; c < NBATCH; ++c) load_codes(base + c, cw[c]);
    load_x(base, xr[0]);
    load_x(base + 1, xr[1]);
#pragma unroll
    for (int c = 0; c < GD - 1; ++c) gather(cw[c], af[c]);
    store_x(0, xr[0]);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NBATCH; ++s) {
      const int buf = s & 1;  // NBATCH is even: the first chunk of every batch uses buffer 0
      if (s + GD - 1 < NBATCH) gather(cw[s + GD - 1], af[(s + GD - 1) % GD]);   // compile-time conditions only
      if (s + 2 < NBATCH) load_x(base + s + 2, xr[s % 2]);                       // slot of chunk s: already in LDS
      mfmas(buf, af[s % GD]);
      if (s + 1 < NBATCH) store_x(buf ^ 1, xr[(s + 1) % 2]);
      __syncthreads();
    }
  }

  // fp32 partials: C layout col = lane&31 (batch), row = (r&3) + 8*(r>>2) + 4*half
  float* out = p.partial + (long)ks * p.M * p.Bpad;
#pragma unroll
  for (int t = 0; t < NBT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_tile0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (row < p.M) out[(long)row * p.Bpad + t * 32 + (lane & 31)] = acc[t][r];
    }
}

// Y[b][m] = (sum_s partial[s][m][b]) * scales[m] + bias[m]; 32x32 tile transpose through LDS.
struct FinalizeParams {
  const float* partial;
  const uint16_t* scales;
  const uint16_t* bias;
  uint16_t* Y;
  int M, B, Bpad, ksplit;
  long ys;
};

template <class T>
__global__ __launch_bounds__(256) void gemm_finalize_kernel(const FinalizeParams p) {
  __shared__ float tile[32][33];
  const int m0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + i * 8, b = b0 + tx;
    float s = 0.f;
    if (m < p.M && b < p.Bpad) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = k < p.ksplit ? p.partial[((long)k * p.M + m) * p.Bpad + b] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
      for (int k = 8; k < p.ksplit; ++k) s += p.partial[((long)k * p.M + m) * p.Bpad + b];
    }
    tile[ty + i * 8][tx] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + ty + i * 8, m = m0 + tx;
    if (m < p.M && b < p.B) {
      const float scale = T::to_float(p.scales[m]);
      const float bias = p.bias ? T::to_float(p.bias[m]) : 0.f;
      p.Y[(long)b * p.ys + m] = T::from_float(__builtin_fmaf(tile[tx][ty + i * 8], scale, bias));
    }
  }
}

struct GemmPlan {
  int ksplit, kslice, Bpad, nbt;
};

static GemmPlan plan_gemm(int B, int M, int K) {
  GemmPlan g;
  g.nbt = (std::min(B, 128) + 31) / 32;
  g.Bpad = g.nbt * 32;
  const int row_blocks = (M + 127) / 128;
  const int kchunks = (K + BK - 1) / BK;
  int ksplit = std::max(1, 256 / row_blocks);
  ksplit = std::min(ksplit, kchunks);
  const int chunks_per = (kchunks + ksplit - 1) / ksplit;
  g.kslice = chunks_per * BK;
  g.ksplit = (kchunks + chunks_per - 1) / chunks_per;
  return g;
}

template <class T, int G>
static int launch_gemm(const GemmParams& p, int nbt, hipStream_t stream) {
  const int blocks = ((p.M + 127) / 128) * p.ksplit;
  switch (nbt) {
    case 1: hipLaunchKernelGGL((gemm_1x16_mfma_kernel<T, G, 1>), dim3(blocks), dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((gemm_1x16_mfma_kernel<T, G, 2>), dim3(blocks), dim3(256), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((gemm_1x16_mfma_kernel<T, G, 3>), dim3(blocks), dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((gemm_1x16_mfma_kernel<T, G, 4>), dim3(blocks), dim3(256), 0, stream, p); break;
  }
  return check_hip(hipGetLastError(), "gemm_1x16_mfma launch");
}

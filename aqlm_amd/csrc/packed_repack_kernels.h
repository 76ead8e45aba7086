// Part of gemv_packed.hip (inside namespace aqlm::PK_NS): the kernels that run when a layer is loaded -- the repack (pk_hist_kernel
// ... pk_compress_kernel), its inverse (pk_unpack3_kernel, pk_unpack_kernel) and the dequantise from packed codes
// (pk_dequant_kernel).  Needs packed_format.h.

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

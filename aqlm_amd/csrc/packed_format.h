// Part of gemv_packed.hip (read inside namespace aqlm::PK_NS, once per build): packed format v7 on the host and the device --
// constants, stream geometry (PkGeom and its functions), the buffer layout (PackedLayout, packed_layout, desc_layout) and the
// wave-count choice (choose_waves).  Needs the build parameters of gemv_packed.hip and aqlm_common.h only.

constexpr int PK_G = AQLM_PK_G;                              // elements of a codebook vector
constexpr int PK_VSH = PK_G == 8 ? 4 : 5;                    // log2(bytes of a vector)
constexpr uint32_t PK_VB = 1u << PK_VSH;                     // bytes of a codebook vector == bytes of x per input group
constexpr uint32_t PK_HMASK = 0xfff0u;                       // LDS byte offset inside a 16-bit half of an entry
// 32-byte vectors are read as two 16-byte halves.  All vectors start at even 16-B slots, so a plain "first halves, then second
// halves" would use only 8 of the 16 bank groups per read.  Odd lanes therefore read the halves in the opposite order: bit 4 of
// BOTH halves of an entry (spare: the offsets are multiples of 32) is the parity of the lane the entry is stored for, the
// first read uses the offsets as they are, the second flips bit 4.
constexpr uint32_t PK_PARITY_BITS = PK_G == 16 ? 0x00100010u : 0u;
static_assert(PK_G == 8 || PK_G == 16, "codebook vectors of 8 or 16 elements");

constexpr int PK_S_LOG = AQLM_PK_S_LOG;
constexpr int PK_S = 1 << PK_S_LOG;          // slices
constexpr int PK_NG = 1 << AQLM_PK_NG_LOG;   // row groups
constexpr int PK_NST = PK_NG * PK_S;         // streams == workgroups of a layer
constexpr int PK_CODE_BITS = 16 - PK_S_LOG;  // bits of a code inside its slice
constexpr int PK_SLICE_ENTRIES = 1 << PK_CODE_BITS;
constexpr uint32_t PK_SLICE_BYTES = PK_SLICE_ENTRIES * PK_VB;
constexpr int PK_MAX_NW = 16;
constexpr int PK_MAX_T = 1024;
constexpr int PK_MAX_GROUPS = (int)(65536u / PK_VB) - 2;  // the x offset of a group is a 16-bit byte offset; in_groups itself is the null slot
constexpr uint32_t PK_MAGIC = 0x37505141u;   // "AQP7"
constexpr int PK_VERSION = 7;
constexpr int PK_MIN_GROUPS = PK_NG / 2;     // variable geometry: workgroups of a slice (its rows per group stay <= 2 x the uniform count)
constexpr int PK_VG_MIN_ROWS = 512;          // ... and only layers of at least this many rows (every group owns >= 1 row)
constexpr uint32_t PK_XWIN_FULL = 65520;     // x window of the batch-1 kernel (x first, slice behind it)
// ... and the compact one: the window is reserved address space, not data, and with 64 KiB of it no second workgroup fits the
// CU.  The x image of a one-row launch is in_groups vectors (the fill is guarded by idx < x16) plus the null slot behind them,
// so (4096 / 8 + 1) * 16 bytes hold inputs of <= 4096 features exactly; then two layers' workgroups share a CU.
constexpr uint32_t PK_XWIN_COMPACT = (4096u / 8u + 1u) * 16u;  // 8208
// accumulator cell of the fused finalize: [arrivals : CNT bits][non-finite contributions : CNT bits][fixed-point sum]
constexpr int PK_CNT_BITS = PK_S_LOG + 1;                       // counts 0 .. PK_S
constexpr unsigned long long PK_CNT_MASK = (1ull << PK_CNT_BITS) - 1ull;
constexpr int PK_VAL_SHIFT = 2 * PK_CNT_BITS;                   // 10 for 16 slices
// |slice sum| < 2^e is stored in units of 2^(e - PK_FIX_BITS).  The finite test lets an addend reach 2 x the bound (rounding slack, a
// slightly stale codebook range), so PK_S addends stay below 2^(PK_FIX_BITS + 1 + PK_S_LOG), which must fit the signed sum field of
// 64 - PK_VAL_SHIFT bits: PK_FIX_BITS <= 60 - 3 PK_S_LOG.  16 slices: 47 (the 51 - PK_S_LOG of rounds 2-3); 32 slices (g16): 45 -- with
// 46 a stale range could wrap the sum instead of giving the NaN the header promises.
constexpr int PK_FIX_BITS = (51 - PK_S_LOG) < (60 - 3 * PK_S_LOG) ? (51 - PK_S_LOG) : (60 - 3 * PK_S_LOG);
static_assert(PK_FIX_BITS + 1 + PK_S_LOG <= 63 - 2 * (PK_S_LOG + 1), "PK_S addends of up to twice the bound must fit the sum field");

// x copies (batch-1 kernel): copy c of x starts at 16-B slot c * stride with stride = 4 (mod 16), i.e. its bank-group
// pattern is rotated by 4 c: an entry can read the copy whose bank group is still free in its service group.
__host__ __device__ static inline int pk_x_stride(int in_groups) { return ((in_groups + 1 + 11) & ~15) + 4; }  // >= in_groups + 1
static inline int pk_max_x_copies(int in_groups) { return std::max(1, std::min(4, 4095 / pk_x_stride(in_groups))); }
// bytes of the x image of a one-row launch: the last copy's in_groups vectors and its null slot end it
static inline uint32_t pk_x_image_bytes(int in_groups, int XC) {
  return ((uint32_t)(XC - 1) * (uint32_t)pk_x_stride(in_groups) + (uint32_t)in_groups + 1u) * PK_VB;
}
// start row of a column: 15 bits over the low nibbles of its first lane-step (entry 0: bits 1-3, entries 1-3: bits 0-3)
__host__ __device__ static inline uint32_t pk_get_start_row(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
  return ((e0 >> 1) & 7u) | ((e1 & 15u) << 3) | ((e2 & 15u) << 7) | ((e3 & 15u) << 11);
}

constexpr int PK_STEP3 = 768;   // bytes of one wave step of 3-byte entries (64 lanes x 12 B)
constexpr int PK_WREG3 = 776;   // ... per step incl. its 8-B row-end flag word (flag words lead the wave range)

// Stream geometry: which slice and which rows workgroup / stream `st` owns.
//   uniform (vg == 0, formats <= v6): PK_NG row groups of RG rows for every slice, stream = group * PK_S + slice;
//   variable (vg == 1): slice s has n[s] row groups, the rows are split evenly over them (the first M % n[s] groups hold one
//   row more), streams are numbered slice by slice: stream = first[s] + group.
struct PkGeom {
  int M;
  int vg;
  int RG;                    // most rows of any stream: the row-start tables have RG + 1 entries per stream, the LDS row tables RG + 1
  uint16_t first[PK_S + 1];  // first stream of slice s (vg)
  uint8_t n[PK_S];           // row groups (= workgroups) of slice s
};

__host__ __device__ static inline void pk_group_rows(const PkGeom& G, int s, int k, int& row0, int& nrows) {
  if (!G.vg) {
    row0 = k * G.RG;
    const int n = G.M - row0;
    nrows = n < 0 ? 0 : (n < G.RG ? n : G.RG);
    return;
  }
  const int n = G.n[s], base = G.M / n, extra = G.M - base * n;
  row0 = k * base + (k < extra ? k : extra);
  nrows = base + (k < extra ? 1 : 0);
}
__host__ __device__ static inline void pk_stream_slice(const PkGeom& G, int st, int& s, int& k) {
  if (!G.vg) {
    s = st & (PK_S - 1);
    k = st >> PK_S_LOG;
    return;
  }
  s = 0;
  while (s + 1 < PK_S && (int)G.first[s + 1] <= st) ++s;
  k = st - (int)G.first[s];
}
__host__ __device__ static inline void pk_stream_rows(const PkGeom& G, int st, int& s, int& row0, int& nrows) {
  int k;
  pk_stream_slice(G, st, s, k);
  pk_group_rows(G, s, k, row0, nrows);
}
// stream and row-in-stream of (slice, row)
__host__ __device__ static inline void pk_row_stream(const PkGeom& G, int s, int row, int& st, int& r) {
  if (!G.vg) {
    const int k = row / G.RG;
    r = row - k * G.RG;
    st = k * PK_S + s;
    return;
  }
  const int n = G.n[s], base = G.M / n, extra = G.M - base * n, thr = extra * (base + 1);
  int k;
  if (row < thr) {
    k = row / (base + 1);
    r = row - k * (base + 1);
  } else {
    k = extra + (row - thr) / base;
    r = row - thr - (k - extra) * base;
  }
  st = (int)G.first[s] + k;
}

// geometry from the row groups per slice (nullptr: uniform); false if they do not describe PK_NST workgroups
static bool pk_make_geom(int M, const uint8_t* groups, PkGeom& G) {
  G.M = M;
  G.vg = 0;
  int sum = 0, mn = PK_NG;
  for (int s = 0; s < PK_S; ++s) {
    const int n = groups ? (int)groups[s] : PK_NG;
    if (n < 1) return false;
    G.n[s] = (uint8_t)n;
    G.first[s] = (uint16_t)sum;
    sum += n;
    mn = n < mn ? n : mn;
    if (n != PK_NG) G.vg = 1;
  }
  G.first[PK_S] = (uint16_t)sum;
  if (sum != PK_NST) return false;
  if (G.vg && (PK_G != 8 || M < PK_VG_MIN_ROWS)) return false;
  G.RG = G.vg ? (M + mn - 1) / mn : (M + PK_NG - 1) / PK_NG;
  return true;
}

struct PackedLayout {
  int M, in_groups, RG, NW, T, XC, EB;
  size_t nst, off_winfo, off_rowstart, off_acc, off_ent, ent_bytes, used;
  PkGeom G;
  bool relabel;            // permutation (u16 old_of_new[65536]) at off_perm, codebook image at off_cb
  size_t off_perm, off_cb;
};

__host__ __device__ static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static int packed_max_batch(int in_groups, int RG);  // rows of x whose LDS image fits a CU (0: not even one)

static bool packed_shape_ok(int out_features, int in_features, int g) {
  return g == PK_G && out_features > 0 && in_features > 0 && in_features % PK_G == 0 && in_features / PK_G <= PK_MAX_GROUPS &&
         (out_features + PK_NG - 1) / PK_NG <= 32767 - PK_MAX_NW &&
         packed_max_batch(in_features / PK_G, (out_features + PK_NG - 1) / PK_NG) >= 1;  // slice + x + the row tables of a row group in 160 KiB
}

static bool packed_layout(int out_features, int in_features, int NW, int T, PackedLayout& L, int XC = 1, int EB = 4,
                          const uint8_t* groups = nullptr, bool relabel = false) {
  if (!packed_shape_ok(out_features, in_features, PK_G) || NW < 1 || NW > PK_MAX_NW || T < 1 || T > PK_MAX_T) return false;
  if (XC < 1 || XC > pk_max_x_copies(in_features / PK_G) || (PK_G != 8 && XC != 1)) return false;
  if (EB != 4 && !(EB == 3 && T <= 32 && PK_G == 8)) return false;  // 3-byte entries: the row-end flags of a column are one 32-bit mask
  if (!pk_make_geom(out_features, groups, L.G)) return false;
  if (L.G.vg && (EB != 4 || L.G.RG > 32767 - PK_MAX_NW || packed_max_batch(in_features / PK_G, L.G.RG) < 1)) return false;
  L.XC = XC;
  L.EB = EB;
  L.M = out_features;
  L.in_groups = in_features / PK_G;
  L.RG = L.G.RG;
  L.NW = NW;
  L.T = T;
  L.nst = (size_t)PK_NST;
  L.off_winfo = 256;
  L.off_rowstart = align_up(L.off_winfo + L.nst * PK_MAX_NW * 16, 256);         // [nst][RG + 1] u32 (offset independent of NW)
  // accumulator cells of the fused finalize: [AQLM_HIP_MAX_GEMV_BATCH][M] u64, zero at rest (offset independent of NW, T)
  L.off_acc = align_up(L.off_rowstart + L.nst * (size_t)(L.RG + 1) * 4, 256);
  L.off_ent = align_up(L.off_acc + (size_t)AQLM_HIP_MAX_GEMV_BATCH * out_features * 8, 1024);
  L.ent_bytes = L.nst * NW * T * (EB == 3 ? (size_t)PK_WREG3 : (size_t)1024);
  L.relabel = relabel;
  L.off_perm = align_up(L.off_ent + L.ent_bytes, 1024);
  L.off_cb = L.off_perm + (size_t)65536 * 2;
  L.used = relabel ? L.off_cb + (size_t)65536 * PK_VB : L.off_ent + L.ent_bytes;
  return L.ent_bytes < ((size_t)1 << 32);  // 32-bit buffer offsets
}

static bool desc_layout(const aqlm_hip_packed_desc* d, PackedLayout& L) {
  return d && d->magic == PK_MAGIC && d->version == PK_VERSION && d->slices_log2 == PK_S_LOG &&
         packed_layout(d->out_features, d->in_features, d->waves, d->steps, L, (int)d->x_copies, d->entry_bytes, d->slice_groups,
                       (d->flags & AQLM_HIP_PACKED_RELABELLED) != 0) &&
         L.used == d->used_bytes && d->rows_per_group == L.RG && ((d->flags & AQLM_HIP_PACKED_VARGEOM) != 0) == (L.G.vg != 0);
}

// Wave-steps of work in the longest stream -> waves per workgroup.
// Long streams (>= 13 steps per wave at 16 waves: the 28672-row / 28672-wide layers) are bound by the entry stream and want
// every wave the CU can hold: 16 (8192 -> 28672 with 14 / 12 waves: 30.9 / 30.7 us against 25.1; r03_mb_packed_variants.log).
// Mid-size layers are bound by the LDS and run as fast or faster on 14 waves (single-kernel regime, same box: 8192 -> 8192
// 10.6 vs 10.9 us, 14336 -> 4096 10.3 vs 10.5, 4096 -> 14336 10.45 vs 10.55, 4096 -> 11008 9.10 vs 9.09) -- and 14 waves
// leave room for the two DMA waves of the pipelined shared-input kernel, whose fill then hides completely (2 x 4096 ->
// 14336 in one launch: 18.85 us packed for 14 waves, 19.75 for 16).  (Round 2's "13-15 waves are 10-18 % slower" was
// measured with the two-kernel finalize and no longer holds.)  Small layers (< 48 wave-steps per workgroup): the wave
// ranges have T = ceil(q / NW) steps each, so the capacity NW * T overshoots the content by up to NW - 1 steps, a large
// share of such a layer: pick 4..8 waves with the least overshoot.
static int choose_waves(uint32_t max_lane_steps) {
  const int q = (int)((max_lane_steps + 63) / 64);
  if (tuning().packed_waves >= 1 && tuning().packed_waves <= PK_MAX_NW) return tuning().packed_waves;
  if (q >= 48) return (q + 15) / 16 >= 13 ? 16 : 14;
  // ... and a step count that is a multiple of the ring depth (3): a remainder of one or two steps runs through the
  // kernel's tail code and leaves late requests behind (measured, profiles/r02_mb_wave_counts.log: 4096x4096 with
  // 6 waves x 6 steps 6.09 us, 7 x 5 6.23 us, 5 x 7 6.22 us; 8192->1024 with 6 x 3 = 7 x 3 5.23 us, 5 x 4 5.55 us)
  int best = 8, best_cost = 1 << 30;
  for (int nw = 8; nw >= (PK_NST > 256 ? 2 : 4); --nw) {  // many small workgroups per CU: fewer waves each
    const int t = (q + nw - 1) / nw;
    const int cost = (nw * t - q) * 8 + (8 - nw) + ((t >= 3 && t % 3 != 0) ? 12 : 0);
    if (cost < best_cost) { best_cost = cost; best = nw; }
  }
  return best;
}

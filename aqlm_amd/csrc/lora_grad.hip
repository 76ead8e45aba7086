// Weight gradients of the LoRA adapters on a DENSE layer (aqlm_hip_lora_grad), gfx950, wave64: the reduction over the rows of the
// batch that aqlm_hip_lora_grad_routed (lora_routed_bwd.hip) does per expert on the VALU, here split over workgroups and run on
// v_mfma_f32_16x16x32_{f16,bf16}.  For ONE adapter index `a` of the call
//     G[r][i] = scaling_a * sum over the rows b < rows with id(b) == a of  w[b][r] * V[b][i]        r < max_rank, i < dim, fp32
// with V storage-type rows (x for grad_A, grad_y for grad_B^T) and w fp32 rows [splits][max_rank] whose slices are added in slice
// order, as lora_sgmv_expand_body adds them (u = B^T grad_y for grad_A, the forward's t = A x for grad_B^T).  grad_x needs no
// kernel: it is aqlm_hip_lora_sgmv on the transposed table (include/aqlm_hip.h).
//
// Orientation.  The MFMA's k is the ROW index b: M = 16 ranks (operand A = w), N = 16 outputs i (operand B = V), K = 32 rows per
// step.  A workgroup of 4 waves owns a span of 256 outputs and one slab of rows; a wave takes 64 outputs as 4 N-tiles and keeps
// ALL M-tiles of the bank in accumulators (MT = 1, 2, 4 or 8 tiles of 16 ranks: rank 128 is 8 x 4 x 4 = 128 registers); only the
// ceil(rank_a / 16) tiles of the call's adapter are multiplied, and the ranks rank_a .. 16 * tiles enter as zero operands.
//
// V.  A step's 32 rows x 256 columns arrive by coalesced 16-byte global loads (a wave covers two whole 512-byte rows per load)
// and are written to one of two LDS tiles; the B operand is V column-major, so it is read with ds_read_b64_tr_b16: the 16 lanes of
// a group read 4 rows x 32 bytes and lane i receives column i of those 4 rows; two reads make the 8 k values of a lane.
// LDS row pitch: 544 bytes (512 + 32).  The transposed read is served in halves of 32 lanes, i.e. the lane groups kg = 0, 1 (or
// 2, 3), each group reading 32 contiguous bytes of 4 rows.  k is a dummy index, so the kernel is free to choose WHICH rows a lane
// group sums: group kg takes rows 4 kg .. 4 kg + 3 in its first read and 16 + 4 kg .. 16 + 4 kg + 3 in its second.  A half then
// touches 8 CONSECUTIVE rows, whose 32-byte pieces start at row * 544 = row * 32 (mod 256): eight distinct 32-byte groups of the
// 64 banks, no conflict.  (A pitch of 512 would put all eight rows on the same banks; with the natural assignment 8 kg + 4 h + q
// the rows r and r + 8 of a half would meet whatever the padding, since 8 * pad = 0 (mod 256) for a pad that keeps 32-byte pieces
// apart.)  The 16-byte image writes cover one whole row per 32 lanes.  This is argued from the addresses; no counter has measured it.
//
// w.  Per step the 32 rows' w (slices summed in slice order, fp32) are split as the forward's expand splits t: hi = round_T(w),
// lo = round_T(w - float(hi)), and staged [r][slot] in LDS, two planes, 80-byte rows (64 + 16: the 16 lanes of a 16-byte read, one
// rank each, meet 16 distinct 16-byte slots, 80 c mod 256 being a permutation of the multiples of 16).  Row 16 h + 4 kg + q of the
// step sits in slot 8 kg + 4 h + q, the order in which group kg meets it in V, so a lane's A fragment is one 16-byte read.  Two
// MFMAs per tile, hi then lo.  fp16: |w| above 65504 has no hi / lo pair, as lora_sgmv.hip states.
//
// Masking.  The ids are judged by lora_common.h.  A row that does not carry the adapter -- another adapter, an id out of range,
// b >= rows -- is ZERO in both images (a select at the write, never a product: an inf or NaN there cannot reach G), its loads go to
// clamped addresses, and columns past dim are zero and never stored.  A step none of whose rows matches (ballot over its 32 ids)
// issues no loads, no LDS traffic and no MFMA.  The loads of the next matching step are issued before the MFMAs of the current one;
// one barrier per step.
//
// Row split.  slabs = f(rows, dim) only: with spans = ceil(dim / 256) and steps = ceil(rows / 32), aim at 256 workgroups -- one per
// CU of the part --, slabs0 = min(ceil(256 / spans), steps, 64), a slab = ceil(steps / slabs0) steps, slabs = ceil(steps / that): every
// slab is a contiguous multiple of 32 rows and none is empty.  4096 rows x 4096 wide: 16 spans x 16 slabs of 8 steps.  Each
// workgroup writes its fp32 tile to the workspace [slabs][max_rank][dim]; aqlm_hip_lora_grad's second launch adds the slabs in
// ascending order, multiplies by scaling_a and writes every element of G (zeros for r >= rank_a and when no row matches).  An entry
// that is not live returns from both kernels before anything is written.  No atomics, no inter-workgroup communication: G is a
// function of the inputs and the shapes alone.
//
// Error.  Products of storage-type operands are exact; with n matching rows, |G - exact| <= |scaling| (eps_T + (n + 2) 2^-24)
// sum_b |w| |V|, eps_T the split error of w: 2^-16 (bf16), 2^-22 (fp16, plus 2^-25 sum_b |V| where lo is subnormal).
#include "lora_sgmv_body.h"

namespace aqlm {
namespace {

constexpr int kLgThreads = 256;
constexpr int kLgSpan = 256;             // outputs per workgroup
constexpr int kLgStep = 32;              // rows per step: the k of one MFMA
constexpr uint32_t kLgVPitch = 544;      // bytes of an LDS row of V (the header has the bank argument)
constexpr uint32_t kLgVBytes = kLgStep * kLgVPitch;
constexpr uint32_t kLgWPitch = 80;       // bytes of an LDS row of hi or lo: 32 slots
constexpr int kLgTargetGroups = 256;     // workgroups the slab rule aims at
constexpr int kLgMaxSlabs = 64;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* glds_s16x4_ptr;

struct LoraGradArgs {
  const aqlm_hip_lora_entry* table;
  const void* ids;
  const uint16_t* v;
  const float* w;
  float* partial;  // [slabs][max_rank][dim]
  long vs, w_row_stride, w_split_stride;
  int ids_int64, nadapters, max_rank, adapter, rows, dim, splits, slab_rows;
};

constexpr size_t lg_lds_bytes(int mt) { return 2 * (size_t)kLgVBytes + 4 * (size_t)mt * 16 * kLgWPitch; }

template <class T, int MT>
__global__ __launch_bounds__(kLgThreads) void lora_grad_kernel(const LoraGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t W_PLANE = MT * 16 * kLgWPitch;  // hi (or lo) of one buffer
  constexpr uint32_t W_BASE = 2 * kLgVBytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(a.table + a.adapter);
  const int rank = lora_rank(ent->rank, a.max_rank);
  if (rank == 0) return;  // not live: nothing of it is written, here or by the finalize
  const int mt_live = (rank + 15) >> 4;
  const int col0 = blockIdx.x * kLgSpan;
  const int b_begin = blockIdx.y * a.slab_rows, b_end = min(a.rows, b_begin + a.slab_rows);
  const int nsteps = (b_end - b_begin + kLgStep - 1) / kLgStep;

  // the rows of step s that carry the adapter, bit j = row b_begin + 32 s + j (uniform: every wave reads the same 32 ids)
  auto step_mask = [&](int s) -> uint32_t {
    const int b = b_begin + s * kLgStep + lane;
    int id = -1;
    if (lane < kLgStep && b < b_end) id = lora_row_id<int>(a.ids, a.ids_int64, b, a.nadapters);
    return (uint32_t)__builtin_amdgcn_ballot_w64(id == a.adapter);
  };
  auto next_live = [&](int s, uint32_t& m) {
    for (; s < nsteps; ++s) {
      m = step_mask(s);
      if (m) break;
    }
    return s;
  };

  // ---- this thread's share of the V image: 16-byte piece pc of rows vr, vr + 8, vr + 16, vr + 24 ---------------------------------
  const int pc = tid & 31, vr = tid >> 5;
  const bool col_ok = col0 + pc * 8 < a.dim;  // dim % 8 == 0: a piece is inside or outside as a whole
  const uint16_t* vcol = a.v + col0 + (col_ok ? pc * 8 : 0);
  u32x4 vv[4];
  auto load_v = [&](int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = min(b_begin + s * kLgStep + vr + 8 * i, a.rows - 1);  // a row past `rows`: the last row's address, masked below
      vv[i] = *reinterpret_cast<const u32x4*>(vcol + (long)b * a.vs);
    }
  };
  auto put_v = [&](int buf, uint32_t m) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = vr + 8 * i;
      const bool ok = col_ok && ((m >> rr) & 1);
      *reinterpret_cast<u32x4*>(smem + buf * kLgVBytes + rr * kLgVPitch + pc * 16) = ok ? vv[i] : zero;
    }
  };

  // ---- ... and of the w image: ranks 4 r4 .. 4 r4 + 3 of the step's rows 4 bq .. 4 bq + 3 (threads below 32 MT) -------------------
  const bool w_unit = tid < 32 * MT;
  const int r4 = tid % (4 * MT), bq = (tid / (4 * MT)) & 7;
  const bool r_ok = 4 * r4 < rank;  // rank % 8 == 0: the 4 ranks exist together; the others enter as zeros
  const uint32_t wdst = W_BASE + (uint32_t)(4 * r4) * kLgWPitch + 16u * (bq & 3) + 8u * (bq >> 2);  // slots 8 kg + 4 h ..: bq = 4 h + kg
  float4 wv[4];
  auto load_w = [&](int s) {
    if (!w_unit) return;
    const float* p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = min(b_begin + s * kLgStep + 4 * bq + j, a.rows - 1);
      p[j] = a.w + (long)b * a.w_row_stride + (r_ok ? 4 * r4 : 0);
      wv[j] = *reinterpret_cast<const float4*>(p[j]);
    }
    for (int sp = 1; sp < a.splits; ++sp) {  // slices in slice order, the 4 rows' loads of a slice together
      float4 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const float4*>(p[j] + (long)sp * a.w_split_stride);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wv[j].x += t[j].x; wv[j].y += t[j].y; wv[j].z += t[j].z; wv[j].w += t[j].w;
      }
    }
  };
  auto put_w = [&](int buf, uint32_t m) {
    if (!w_unit) return;
    float f[4][4];  // [rank of the chunk][row of the quad]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = r_ok && ((m >> (4 * bq + j)) & 1);
      f[0][j] = ok ? wv[j].x : 0.f;
      f[1][j] = ok ? wv[j].y : 0.f;
      f[2][j] = ok ? wv[j].z : 0.f;
      f[3][j] = ok ? wv[j].w : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      u32x2 h, l;
      h.x = sgmv_hi2<T>(f[c][0], f[c][1]);
      h.y = sgmv_hi2<T>(f[c][2], f[c][3]);
      l.x = sgmv_lo2<T>(f[c][0], f[c][1], h.x);
      l.y = sgmv_lo2<T>(f[c][2], f[c][3], h.y);
      unsigned char* dst = smem + buf * (2 * W_PLANE) + wdst + c * kLgWPitch;
      *reinterpret_cast<u32x2*>(dst) = h;
      *reinterpret_cast<u32x2*>(dst + W_PLANE) = l;
    }
  };

  // ---- consumer addresses ---------------------------------------------------------------------------------------------------------
  const int kg = lane >> 4, li = lane & 15;
  uint32_t vsrc[2];  // lane 4 q + p of a group: 8 bytes p of row 16 h + 4 kg + q of the wave's 64 columns (+ 32 bytes per N-tile)
#pragma unroll
  for (int h = 0; h < 2; ++h) vsrc[h] = (uint32_t)(16 * h + 4 * kg + (li >> 2)) * kLgVPitch + 128u * wave + 8u * (li & 3);
  const uint32_t asrc = W_BASE + (uint32_t)li * kLgWPitch + 16u * kg;  // rank li of an M-tile, slots 8 kg .. 8 kg + 7

  f32x4 acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) acc[mt][nn] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint32_t m = 0, mn = 0;
  int s = next_live(0, m);
  if (s < nsteps) {
    load_v(s);
    load_w(s);
  }
  int buf = 0;
  while (s < nsteps) {  // (uniform)
    put_v(buf, m);
    put_w(buf, m);
    __syncthreads();  // the one barrier of a step: the image written two steps on is this one's, and its readers passed here since
    const int sn = next_live(s + 1, mn);
    if (sn < nsteps) {  // in flight while the MFMAs run
      load_v(sn);
      load_w(sn);
    }
    u32x4 bf[4];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kLgVBytes + vsrc[0] + 32u * nn));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((glds_s16x4_ptr)(smem + buf * kLgVBytes + vsrc[1] + 32u * nn));
      const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
      bf[nn] = u32x4{l2.x, l2.y, h2.x, h2.y};
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (mt < mt_live) {  // (uniform)
        const unsigned char* ap = smem + buf * (2 * W_PLANE) + asrc + mt * 16 * kLgWPitch;
        const u32x4 ah = *reinterpret_cast<const u32x4*>(ap), al = *reinterpret_cast<const u32x4*>(ap + W_PLANE);
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          acc[mt][nn] = mfma16<T>(ah, bf[nn], acc[mt][nn]);  // D[r = 4 kg + reg][i = li]
          acc[mt][nn] = mfma16<T>(al, bf[nn], acc[mt][nn]);
        }
      }
    }
    s = sn;
    m = mn;
    buf ^= 1;
  }

  // ---- the slab's tile: lane (kg, li) holds ranks 16 mt + 4 kg + reg of output col0 + 64 wave + 16 nn + li -------------------------
  float* out = a.partial + (size_t)blockIdx.y * a.max_rank * a.dim;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      const int i = col0 + 64 * wave + 16 * nn + li;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = 16 * mt + 4 * kg + reg;
        if (r < a.max_rank && i < a.dim) out[(size_t)r * a.dim + i] = acc[mt][nn][reg];
      }
    }
}

// the slabs meet: fp32 sums in slab order, times scaling; a thread owns 4 consecutive elements (dim % 8 == 0)
__global__ __launch_bounds__(256) void lora_grad_finalize_kernel(const aqlm_hip_lora_entry* table, int adapter, int max_rank,
                                                                 const float* partial, float* g, long plane4, int slabs) {
  const lora_entry_ptr ent = (lora_entry_ptr)(uintptr_t)(table + adapter);
  if (lora_rank(ent->rank, max_rank) == 0) return;
  const float scaling = ent->scaling;
  const f32x4* src = reinterpret_cast<const f32x4*>(partial);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < plane4; i += (long)gridDim.x * 256) {
    f32x4 v = src[i];
    for (int z = 1; z < slabs; ++z) v += src[(long)z * plane4 + i];
    reinterpret_cast<f32x4*>(g)[i] = scaling * v;
  }
}

bool lg_shape_ok(int dim, int max_rank, int rows) {
  return dim >= 8 && dim % 8 == 0 && max_rank >= 8 && max_rank <= kLoraMaxRank && max_rank % 8 == 0 && rows >= 1 &&
         rows <= AQLM_HIP_MAX_LORA_SGMV_ROWS;
}

// steps of 32 rows per slab: a function of rows and dim alone (the header has the rule)
int lg_slab_steps(int rows, int dim) {
  const int spans = (dim + kLgSpan - 1) / kLgSpan, steps = (rows + kLgStep - 1) / kLgStep;
  const int slabs0 = std::max(1, std::min({(kLgTargetGroups + spans - 1) / spans, steps, kLgMaxSlabs}));
  return (steps + slabs0 - 1) / slabs0;
}
int lg_slabs(int rows, int dim) {
  const int steps = (rows + kLgStep - 1) / kLgStep, per = lg_slab_steps(rows, dim);
  return (steps + per - 1) / per;
}

template <class T, int MT>
int launch_lg(const LoraGradArgs& a, int slabs, hipStream_t stream) {
  auto kern = lora_grad_kernel<T, MT>;
  const size_t lds = lg_lds_bytes(MT);
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.dim + kLgSpan - 1) / kLgSpan), (unsigned)slabs), dim3(kLgThreads), lds, stream, a);
  return check_hip(hipGetLastError(), "lora_grad launch");
}

template <class T>
int launch_lg_rank(const LoraGradArgs& a, int slabs, hipStream_t stream) {
  if (a.max_rank <= 16) return launch_lg<T, 1>(a, slabs, stream);
  if (a.max_rank <= 32) return launch_lg<T, 2>(a, slabs, stream);
  if (a.max_rank <= 64) return launch_lg<T, 4>(a, slabs, stream);
  return launch_lg<T, 8>(a, slabs, stream);
}

}  // namespace
}  // namespace aqlm

using namespace aqlm;

extern "C" int aqlm_hip_lora_grad_supported(int dim, int max_rank, int rows) { return lg_shape_ok(dim, max_rank, rows) ? 1 : 0; }

extern "C" int aqlm_hip_lora_grad_slabs(int rows, int dim) {
  if (rows < 1 || rows > AQLM_HIP_MAX_LORA_SGMV_ROWS || dim < 1) return 0;
  return lg_slabs(rows, dim);
}

extern "C" size_t aqlm_hip_lora_grad_workspace_bytes(int rows, int max_rank, int dim) {
  if (!lg_shape_ok(dim, max_rank, rows)) return 0;
  return (size_t)lg_slabs(rows, dim) * (size_t)max_rank * (size_t)dim * 4;
}

extern "C" int aqlm_hip_lora_grad(const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, int adapter, const void* ids,
                                  int ids_int64, int rows, const void* v, long v_row_stride, int dim, const float* w,
                                  long w_row_stride, int w_splits, long w_split_stride, float* g, size_t g_bytes, void* workspace,
                                  size_t workspace_bytes, int dtype, void* stream_) {
  static const char* who = "aqlm_hip_lora_grad";
  if (int e = check_not_null(who, table && v && w && g && workspace)) return e;
  if (int e = check_aligned(who, "table / ids / w / g / workspace",
                            aligned8(table) && (!ids || ids_aligned(ids, ids_int64)) && aligned4(w) && aligned16(g) &&
                                aligned16(workspace)))
    return e;
  if (num_adapters < 1 || max_rank < 1 || rows < 1 || dim < 1 || w_splits < 1 || adapter < 0 || adapter >= num_adapters) {
    set_last_error("%s: bad sizes (adapters=%d max_rank=%d rows=%d dim=%d splits=%d: all positive; adapter=%d in [0, adapters))", who,
                   num_adapters, max_rank, rows, dim, w_splits, adapter);
    return AQLM_HIP_E_INVALID;
  }
  if (v_row_stride < dim || w_row_stride < max_rank || (w_splits > 1 && w_split_stride < max_rank)) {
    set_last_error("%s: strides (V row %ld, w row %ld, w split %ld) shorter than the rows (dim=%d, max_rank=%d)", who, v_row_stride,
                   w_row_stride, w_split_stride, dim, max_rank);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!lg_shape_ok(dim, max_rank, rows) || w_splits > kSgmvMaxSplits || !aligned16(v) || v_row_stride % 8 != 0 || !aligned16(w) ||
      w_row_stride % 4 != 0 || (w_splits > 1 && w_split_stride % 4 != 0)) {
    set_last_error("%s: shape outside the kernel (rank a multiple of 8 in 8..%d, dim %% 8 == 0, 1..%d rows, at most %d slices of w, "
                   "V and w rows 16-byte aligned; got max_rank=%d dim=%d rows=%d splits=%d strides V %ld, w %ld / %ld)", who,
                   kLoraMaxRank, AQLM_HIP_MAX_LORA_SGMV_ROWS, kSgmvMaxSplits, max_rank, dim, rows, w_splits, v_row_stride,
                   w_row_stride, w_split_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t plane = (size_t)max_rank * (size_t)dim * 4;
  if (g_bytes < plane) {
    set_last_error("%s: output of %zu bytes, %zu bytes needed", who, g_bytes, plane);
    return AQLM_HIP_E_INVALID;
  }
  const int slabs = lg_slabs(rows, dim);
  if (int e = lora_check_workspace(who, workspace_bytes, (size_t)slabs * plane)) return e;

  LoraGradArgs a{};
  a.table = table;
  a.ids = ids;
  a.v = (const uint16_t*)v;
  a.w = w;
  a.partial = (float*)workspace;
  a.vs = v_row_stride;
  a.w_row_stride = w_row_stride;
  a.w_split_stride = w_splits > 1 ? w_split_stride : 0;
  a.ids_int64 = ids_int64 ? 1 : 0;
  a.nadapters = num_adapters;
  a.max_rank = max_rank;
  a.adapter = adapter;
  a.rows = rows;
  a.dim = dim;
  a.splits = w_splits;
  a.slab_rows = lg_slab_steps(rows, dim) * kLgStep;
  hipStream_t stream = (hipStream_t)stream_;
  if (int e = dtype == AQLM_HIP_F16 ? launch_lg_rank<F16>(a, slabs, stream) : launch_lg_rank<BF16>(a, slabs, stream)) return e;
  const long plane4 = (long)max_rank * dim / 4;
  const unsigned blocks = (unsigned)std::min<long>((plane4 + 255) / 256, 1024);
  hipLaunchKernelGGL(lora_grad_finalize_kernel, dim3(blocks), dim3(256), 0, stream, table, adapter, max_rank, (const float*)a.partial,
                     g, plane4, slabs);
  return check_hip(hipGetLastError(), "lora_grad finalize launch");
}

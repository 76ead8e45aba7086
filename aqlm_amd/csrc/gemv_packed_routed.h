// Expert-routed launch of the prepacked 1x16 matvec (Mixtral decode on prepacked experts), gfx950, wave64.
// Included at the end of gemv_packed.hip, so it is built twice like the rest of that file (8- and 16-element vectors).  Needs the
// matvec body and LDS maps (packed_gemv_kernels.h), the layout (packed_format.h), packed_launch.h and packed_gemv_entries.h's packed_fused.
//
// One launch computes every (token, expert) pair of one projection of a mixture-of-experts block -- or of the two that read the
// same rows (w1 and w3) -- on the experts' PACKED buffers, with the routing read on the device only:
//   * grid = 256 streams x segments x experts, fixed by the shapes: a captured launch stays valid for any routing;
//   * every wave reads the <= 64 ids itself and ballots `id == its workgroup's expert` (gemv_routed.hip's rule): ids are compared,
//     never used to form an address.  Ids outside [0, num_experts) match no expert; the slice-0 workgroups of expert 0 write the
//     rows of such pairs as zeros.  A workgroup whose expert has no pair exits before it touches anything else;
//   * the pairs of the expert go through gemv_1x16_packed_body at batch 1, one pass each, on the pair's own x row, y row and
//     accumulator cells (two pairs of one expert must not meet in a cell): every row is bit-identical to
//     aqlm_hip_gemv_1x16_packed of that expert on that row, whatever the other pairs are (the cells add fixed-point integers, so the
//     order in which the slice workgroups arrive cannot change a bit);
//   * block size and dynamic LDS are launch-wide: the largest wave count of the table (the body idles waves >= p.NW) and the row
//     tables of the common rows-per-group (all entries share out_features and the uniform 256-stream geometry).
// No chain prefetch, no publish (NPW = 0, pub = nullptr).  4-byte entries, uniform geometry, descriptors with a codebook range.

namespace aqlm {
namespace PK_NS {

struct RoutedPackedArgs {
  const aqlm_hip_routed_packed_entry* table;  // device, [nexp][nseg]
  const void* ids;                            // device, [npairs] int64 or int32
  const uint16_t* x;
  uint16_t* y;                                // [npairs][nseg][M]
  unsigned long long* cells;                  // [npairs][nseg][M], zero at rest
  long xs;
  int ids_int64, npairs, top_k, x_per_pair, nexp, nseg;
  int M, in_groups, RG, nwb, fill_rotate;
};

template <class T_, int PD, uint32_t XWIN>
__global__ __launch_bounds__(1024) void gemv_1x16_packed_routed_kernel(const RoutedPackedArgs a) {
  const int e = blockIdx.z, s = blockIdx.y, block = blockIdx.x;
  const int lane = threadIdx.x & 63;
  long id = -1;
  if (lane < a.npairs) id = a.ids_int64 ? reinterpret_cast<const long*>(a.ids)[lane] : (long)reinterpret_cast<const int*>(a.ids)[lane];
  const bool live = lane < a.npairs;
  const uint64_t mine = __builtin_amdgcn_ballot_w64(live && id == (long)e);
  // rows of pairs that match no expert: one writer per (pair, segment, row) -- the slice-0 workgroup of expert 0 that owns the row
  const bool zeroes = e == 0 && (block & (PK_S - 1)) == 0;
  const uint64_t orphans = zeroes ? __builtin_amdgcn_ballot_w64(live && (id < 0 || id >= (long)a.nexp)) : 0;
  if (!mine && !orphans) return;  // wave-uniform and identical in every wave of the workgroup

  const long ps = (long)a.nseg * a.M;  // pair stride of y and of the cells
  if (orphans) {
    const int row0 = (block >> PK_S_LOG) * a.RG;
    const int nrows = std::min(a.RG, a.M - row0);
    for (uint64_t m = orphans; m; m &= m - 1) {
      const int pr = __builtin_ctzll(m);
      for (int r = (int)threadIdx.x; r < nrows; r += a.nwb * 64) a.y[(long)pr * ps + (long)s * a.M + row0 + r] = 0;
    }
  }
  if (!mine) return;

  // the entry through the constant address space: a uniform address, so its fields arrive by s_load and the buffer resource of
  // the entry stream is built from SGPRs (as a global load behind the stores above it would come back in VGPRs)
  typedef const aqlm_hip_routed_packed_entry __attribute__((address_space(4)))* const_entry_ptr;
  const const_entry_ptr ent = (const_entry_ptr)(uintptr_t)(a.table + (e * a.nseg + s));
  // (the pointers it holds are device-global: said through the address space, or every access through them is a FLAT one, which
  // also counts as an LDS operation and would hold the fill barrier's lgkmcnt(0) until scale and bias are back from HBM)
  auto global_ptr = [](uintptr_t v) { return (const void*)(const __attribute__((address_space(1))) void*)v; };
  PackedGemvParams p{};
  p.ent = reinterpret_cast<const uint32_t*>(global_ptr((uintptr_t)ent->entries));
  p.winfo = reinterpret_cast<const uint32_t*>(global_ptr((uintptr_t)ent->wave_info));
  p.rowstart = reinterpret_cast<const uint32_t*>(global_ptr((uintptr_t)ent->row_starts));
  p.codebook = reinterpret_cast<const uint8_t*>(global_ptr((uintptr_t)ent->codebook));
  uintptr_t scales = (uintptr_t)ent->scales, bias = (uintptr_t)ent->bias;
  p.cb_absmax = ent->codebook_absmax;
  p.M = a.M;
  p.in_groups = a.in_groups;
  p.RG = a.RG;
  p.NW = ent->waves;
  p.T = ent->steps;
  p.XC = ent->x_copies;
  p.ent_bytes = ent->entry_stream_bytes;
  p.y_row_stride = a.M;
  p.fill_rotate = a.fill_rotate;

  auto pass = [&](int pr) {
    const int xr = a.x_per_pair ? pr : pr / a.top_k;
    p.x = a.x + (long)xr * a.xs;
    p.y = a.y + (long)pr * ps + (long)s * a.M;
    p.acc = a.cells + (long)pr * ps + (long)s * a.M;
    // The body waits for its LDS fill with a COUNTED vmcnt: the ring loads plus the scale and bias loads it issues behind the last
    // LDS-DMA.  Scale and bias are the same for every pair of the expert; seen as loop-invariant they would be hoisted out of
    // the loop below and the count would let the two youngest DMA requests pass the barrier.  The pointers are laundered per pass.
    asm volatile("" : "+s"(scales), "+s"(bias));
    p.scales = reinterpret_cast<const uint16_t*>(global_ptr(scales));
    p.bias = bias ? reinterpret_cast<const uint16_t*>(global_ptr(bias)) : nullptr;
    // Nothing of an earlier pass (y and cell stores, atomics) or of the zero rows above may be in flight when the body starts
    // (loads and stores return out of order with each other).  The builtin, so that hipcc's wait-count pass sees the drain.
    __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));  // vmcnt(0)
    __builtin_assume(p.acc != nullptr);  // fused finalize only: no partials branch (its store through the null workspace would be a FLAT one)
    gemv_1x16_packed_body<T_, 1, PD, XWIN, 4, false, false, true>(p, block, a.nwb);
  };
  bool first = true;
  for (uint64_t m = mine; m; m &= m - 1) {
    if (!first) __syncthreads();  // the previous pass's epilogue is done with the row tables before the next fill overwrites them
    first = false;
    pass(__builtin_ctzll(m));
  }
}

// ring depth of the launch: the single-layer batch-1 kernel's default (pick_pd; measured best or within 1 % of best on every shape)
static constexpr int kRoutedPackedPD = 3;

static size_t routed_packed_lds(int in_groups, int RG, bool slice_first) {
  return slice_first ? PackedLds<1, 0u>::total(in_groups, RG) : PackedLds<1, PK_XWIN_FULL>::total(in_groups, RG);
}

// what one descriptor must be for the launch: 4-byte entries, uniform geometry, a codebook range (fused finalize)
static bool routed_packed_desc_ok(const aqlm_hip_packed_desc* d, PackedLayout& L, const char** why) {
  if (!desc_layout(d, L)) { *why = "invalid packed descriptor"; return false; }
  if (L.EB != 4) { *why = "3-byte entries (compact) are not instantiated"; return false; }
  if (L.G.vg) { *why = "variable-geometry buffers run on the single-layer kernel only"; return false; }
  if (!packed_fused(d)) { *why = "descriptor without a codebook range (or the fused finalize is switched off)"; return false; }
  return true;
}

}  // namespace PK_NS
}  // namespace aqlm

using namespace aqlm;
using namespace aqlm::PK_NS;

extern "C" PK_API size_t PK_ENTRY(gemv_1x16_routed_packed_lds_bytes)(int out_features, int in_features, int in_group_size) {
  PK_G16_FORWARD_IF(in_group_size == 16, gemv_1x16_routed_packed_lds_bytes, out_features, in_features, in_group_size);
  if (!packed_shape_ok(out_features, in_features, in_group_size)) return 0;
  const int in_groups = in_features / PK_G, RG = (out_features + PK_NG - 1) / PK_NG;
  return routed_packed_lds(in_groups, RG, packed_b1_slice_first(in_groups, RG));
}

extern "C" PK_API int PK_ENTRY(routed_packed_entry_fill)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                         const void* scales, const void* bias, aqlm_hip_routed_packed_entry* entry) {
  PK_G16_FORWARD(desc, routed_packed_entry_fill, desc, packed, codebook, scales, bias, entry);
  static const char* who = "aqlm_hip_routed_packed_entry_fill";
  if (!desc || !packed || !codebook || !scales || !entry) {
    set_last_error("%s: null pointer argument", who);
    return AQLM_HIP_E_INVALID;
  }
  PackedLayout L;
  const char* why = "";
  if (!routed_packed_desc_ok(desc, L, &why)) {
    set_last_error("%s: %s", who, why);
    return desc_layout(desc, L) ? AQLM_HIP_E_UNSUPPORTED : AQLM_HIP_E_INVALID;
  }
  if (!aligned16(packed) || !aligned16(codebook)) {
    set_last_error("%s: packed buffer / codebook must be 16-byte aligned", who);
    return AQLM_HIP_E_INVALID;
  }
  if (L.relabel && !(desc->flags & AQLM_HIP_PACKED_HAS_CODEBOOK)) {
    set_last_error("%s: a relabelled buffer needs its codebook image: call aqlm_hip_packed_set_codebook first", who);
    return AQLM_HIP_E_INVALID;
  }
  const uint8_t* base = (const uint8_t*)packed;
  entry->entries = base + L.off_ent;
  entry->wave_info = base + L.off_winfo;
  entry->row_starts = base + L.off_rowstart;
  entry->codebook = L.relabel ? (const void*)(base + L.off_cb) : codebook;
  entry->scales = scales;
  entry->bias = bias;
  entry->out_features = L.M;
  entry->rows_per_group = L.RG;
  entry->waves = L.NW;
  entry->steps = L.T;
  entry->x_copies = L.XC;
  entry->entry_stream_bytes = (uint32_t)L.ent_bytes;
  entry->codebook_absmax = desc->codebook_absmax;
  entry->reserved = 0;
  return 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_routed_packed_geometry)(const aqlm_hip_packed_desc* const* descs, int n,
                                                                 aqlm_hip_routed_packed_geometry* geom) {
  PK_G16_FORWARD(descs && n >= 1 ? descs[0] : nullptr, gemv_1x16_routed_packed_geometry, descs, n, geom);
  static const char* who = "aqlm_hip_gemv_1x16_routed_packed_geometry";
  if (!descs || n < 1 || n > AQLM_HIP_MAX_ROUTED_EXPERTS * 2 || !geom) {
    set_last_error("%s: 1..%d descriptors and a geometry to fill required (got %d)", who, AQLM_HIP_MAX_ROUTED_EXPERTS * 2, n);
    return AQLM_HIP_E_INVALID;
  }
  aqlm_hip_routed_packed_geometry g{};
  for (int k = 0; k < n; ++k) {
    PackedLayout L;
    const char* why = "";
    if (!descs[k] || !routed_packed_desc_ok(descs[k], L, &why)) {
      set_last_error("%s: descriptor %d: %s", who, k, descs[k] ? why : "null");
      return descs[k] && desc_layout(descs[k], L) ? AQLM_HIP_E_UNSUPPORTED : AQLM_HIP_E_INVALID;
    }
    if (k == 0) {
      g.out_features = descs[k]->out_features;
      g.in_features = descs[k]->in_features;
      g.in_group_size = PK_G;
      g.rows_per_group = L.RG;
    } else if (descs[k]->out_features != g.out_features || descs[k]->in_features != g.in_features || L.RG != g.rows_per_group) {
      set_last_error("%s: descriptor %d is %d -> %d, descriptor 0 is %d -> %d: one table holds one shape", who, k,
                     descs[k]->in_features, descs[k]->out_features, g.in_features, g.out_features);
      return AQLM_HIP_E_INVALID;
    }
    g.max_waves = std::max(g.max_waves, L.NW);
  }
  const int in_groups = g.in_features / PK_G;
  g.slice_first = packed_b1_slice_first(in_groups, g.rows_per_group) ? 1 : 0;
  g.lds_bytes = (uint32_t)routed_packed_lds(in_groups, g.rows_per_group, g.slice_first != 0);
  if (g.lds_bytes > 160u * 1024u) {
    set_last_error("%s: %d -> %d does not fit the LDS image", who, g.in_features, g.out_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  *geom = g;
  return 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_routed_packed_supported)(const aqlm_hip_packed_desc* const* descs, int n) {
  aqlm_hip_routed_packed_geometry g;
  return PK_ENTRY(gemv_1x16_routed_packed_geometry)(descs, n, &g) == 0 ? 1 : 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_routed_packed)(const aqlm_hip_routed_packed_entry* table,
                                                        const aqlm_hip_routed_packed_geometry* geom, int num_experts,
                                                        int num_segments, const void* expert_ids, int ids_int64, int num_pairs,
                                                        int top_k, const void* x, long x_row_stride, int x_per_pair, void* y,
                                                        int dtype, void* cells, size_t cells_bytes, void* stream_) {
  PK_G16_FORWARD_IF(geom && geom->in_group_size == 16, gemv_1x16_routed_packed, table, geom, num_experts, num_segments, expert_ids,
                    ids_int64, num_pairs, top_k, x, x_row_stride, x_per_pair, y, dtype, cells, cells_bytes, stream_);
  static const char* who = "aqlm_hip_gemv_1x16_routed_packed";
  if (int e = check_not_null(who, table && geom && expert_ids && x && y && cells)) return e;
  if (int e = check_aligned(who, "table / expert_ids", aligned8(table) && ids_aligned(expert_ids, ids_int64))) return e;
  if (int e = check_experts(who, num_experts, num_segments)) return e;
  if (int e = check_pairs(who, num_pairs, top_k, AQLM_HIP_MAX_ROUTED_PAIRS)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  const int M = geom->out_features, RG = (M + PK_NG - 1) / PK_NG;
  if (geom->in_group_size != PK_G || !packed_shape_ok(M, geom->in_features, PK_G) || geom->rows_per_group != RG ||
      geom->max_waves < 1 || geom->max_waves > PK_MAX_NW) {
    set_last_error("%s: not a geometry of aqlm_hip_gemv_1x16_routed_packed_geometry", who);
    return AQLM_HIP_E_INVALID;
  }
  const int in_groups = geom->in_features / PK_G;
  const bool slice_first = packed_b1_slice_first(in_groups, RG);
  const size_t lds = routed_packed_lds(in_groups, RG, slice_first);
  if (lds > 160u * 1024u) {
    set_last_error("%s: %d -> %d does not fit the LDS image", who, geom->in_features, M);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (!aligned16(x) || x_row_stride % 8 != 0) {
    set_last_error("%s: x rows must be 16-byte aligned (x stride %ld)", who, x_row_stride);
    return AQLM_HIP_E_INVALID;
  }
  const size_t cells_need = (size_t)num_pairs * num_segments * M * 8;
  if ((reinterpret_cast<uintptr_t>(cells) & 7u) || cells_bytes < cells_need) {
    set_last_error("%s: %zu bytes of 8-byte aligned, zero-filled cells required, got %zu", who, cells_need, cells_bytes);
    return AQLM_HIP_E_INVALID;
  }
  if (!tuning().packed_fused_finalize) {
    set_last_error("%s: the fused finalize is switched off (tuning knob packed_fused_finalize)", who);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  RoutedPackedArgs a{};
  a.table = table;
  a.ids = expert_ids;
  a.x = (const uint16_t*)x;
  a.y = (uint16_t*)y;
  a.cells = (unsigned long long*)cells;
  a.xs = x_row_stride;
  a.ids_int64 = ids_int64 ? 1 : 0;
  a.npairs = num_pairs;
  a.top_k = top_k;
  a.x_per_pair = x_per_pair ? 1 : 0;
  a.nexp = num_experts;
  a.nseg = num_segments;
  a.M = M;
  a.in_groups = in_groups;
  a.RG = RG;
  a.nwb = geom->max_waves;
  a.fill_rotate = tuning().packed_fill_rotate ? 1 : 0;
  hipStream_t stream = (hipStream_t)stream_;
  auto launch = [&](auto kern) -> int {
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, dim3(PK_NST, num_segments, num_experts), dim3(a.nwb * 64), lds, stream, a);
    return check_hip(hipGetLastError(), "gemv_1x16_packed_routed launch");
  };
  constexpr int PD = kRoutedPackedPD;
  if (slice_first)
    return dtype == AQLM_HIP_F16 ? launch(gemv_1x16_packed_routed_kernel<F16, PD, 0u>) : launch(gemv_1x16_packed_routed_kernel<BF16, PD, 0u>);
  return dtype == AQLM_HIP_F16 ? launch(gemv_1x16_packed_routed_kernel<F16, PD, PK_XWIN_FULL>)
                               : launch(gemv_1x16_packed_routed_kernel<BF16, PD, PK_XWIN_FULL>);
}

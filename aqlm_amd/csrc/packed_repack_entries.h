// Part of gemv_packed.hip (after `using namespace aqlm::PK_NS`): the planning steps of the repack (plan_relabel, plan_geometry) and
// the C entries of planning, prepack, codebook image (its kernel reopens the namespace here: it stays behind the matvec kernels
// in the code object), unpack and dequantise.  Needs packed_format.h, packed_repack_kernels.h and packed_launch.h's packed_max_batch.

// ---- planning steps of the repack (host, pure functions) -----------------------------------------------------------------
// Relabelling: deal the 65536 entries to the PK_S slices, heaviest first, each to the lightest slice that still has room
// (longest-processing-time greedy with PK_SLICE_ENTRIES entries per slice): the slices end up with equal code counts unless a
// single entry outweighs a slice's share.  Deterministic (ties: lower label, lower slice).  Within a slice the heaviest entries
// take consecutive slots, i.e. distinct LDS bank groups.  Returns 0 (and leaves new_of_old alone) when the checkpoint's labels
// already load the slices evenly: no permutation, no codebook image, the buffer of format v6.
// `force`: deal even when the slices' TOTAL masses are already even -- label use correlated with the ROW (rows of one block of the
// layer drawing their codes from one slice's labels) leaves every global histogram flat and one stream per row group 14 x the
// mean; the repack asks for it whenever the 16 x 16 layout is not balanced and keeps the result only if the
// longest stream got shorter.  Equal counts fall out round-robin over the slices (stable order, lightest slice first).
static int plan_relabel(const uint32_t* usage, uint16_t* new_of_old, bool force = false) {
  unsigned long long mass0[PK_S] = {}, total = 0;
  for (int c = 0; c < 65536; ++c) mass0[c >> PK_CODE_BITS] += usage[c];
  unsigned long long mx = 0;
  for (int s = 0; s < PK_S; ++s) {
    total += mass0[s];
    mx = std::max(mx, mass0[s]);
  }
  if (total == 0 || (!force && (double)mx * PK_S <= 1.02 * (double)total)) return 0;
  std::vector<uint32_t> order(65536);
  for (uint32_t c = 0; c < 65536; ++c) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return usage[x] > usage[y]; });
  unsigned long long mass[PK_S] = {};
  int cnt[PK_S] = {};
  for (uint32_t i = 0; i < 65536; ++i) {
    const uint32_t c = order[i];
    int best = -1;
    for (int s = 0; s < PK_S; ++s)
      if (cnt[s] < PK_SLICE_ENTRIES && (best < 0 || mass[s] < mass[best])) best = s;
    new_of_old[c] = (uint16_t)(best * PK_SLICE_ENTRIES + cnt[best]);
    ++cnt[best];
    mass[best] += usage[c];
  }
  return 1;
}

// Geometry: deal the PK_NST workgroups to the slices in proportion to their work (lane-steps + a quarter step per row for the
// epilogue's hand-in): start from PK_MIN_GROUPS each, give the next workgroup to the slice whose groups are the longest.
// Uniform unless that shortens the longest stream by more than 6 % (the variable-geometry kernel pays ~0.1 us of scalar
// arithmetic in its prologue and serves single-layer launches only).  Returns 1 when groups[] is not uniform.
static int plan_geometry(const unsigned long long* slice_steps, int M, int in_features, uint8_t* groups) {
  for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)PK_NG;
  if (PK_G != 8 || M < PK_VG_MIN_ROWS || !packed_shape_ok(M, in_features, PK_G)) return 0;
  const int in_groups = in_features / PK_G;
  double w[PK_S], uni = 0.;
  for (int s = 0; s < PK_S; ++s) {
    w[s] = (double)slice_steps[s] + 0.25 * M;
    uni = std::max(uni, w[s] / PK_NG);
  }
  const int mb_uniform = packed_max_batch(in_groups, (M + PK_NG - 1) / PK_NG);
  for (int nmin = PK_MIN_GROUPS; nmin < PK_NG; ++nmin) {
    int n[PK_S], left = PK_NST - nmin * PK_S, mn = PK_NG;
    for (int s = 0; s < PK_S; ++s) n[s] = nmin;
    while (left-- > 0) {
      int best = 0;
      for (int s = 1; s < PK_S; ++s)
        if (w[s] / n[s] > w[best] / n[best]) best = s;
      ++n[best];
    }
    double var = 0.;
    bool uniform = true;
    for (int s = 0; s < PK_S; ++s) {
      var = std::max(var, w[s] / n[s]);
      mn = std::min(mn, n[s]);
      uniform = uniform && n[s] == PK_NG;
      if (n[s] > 255) return 0;
    }
    if (uniform || var > 0.94 * uni) return 0;
    // the bigger row groups of the lightest slices must not cost the layer its multi-row launches (up to 4 rows in one launch; 5
    // and 6 rows may take two): else start from more groups per slice
    if (packed_max_batch(in_groups, (M + mn - 1) / mn) < std::min(mb_uniform, 4)) continue;
    for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)n[s];
    return 1;
  }
  return 0;
}

extern "C" PK_API int PK_ENTRY(packed_plan_relabel)(const uint32_t* usage, int slices_log2, uint16_t* new_of_old) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_relabel, usage, slices_log2, new_of_old);
  if (!usage || !new_of_old || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_relabel: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  return plan_relabel(usage, new_of_old);
}

extern "C" PK_API int PK_ENTRY(packed_plan_relabel_ex)(const uint32_t* usage, int slices_log2, int force, uint16_t* new_of_old) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_relabel_ex, usage, slices_log2, force, new_of_old);
  if (!usage || !new_of_old || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_relabel_ex: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  return plan_relabel(usage, new_of_old, force != 0);
}

extern "C" PK_API int PK_ENTRY(packed_plan_geometry)(const uint64_t* slice_steps, int slices_log2, int out_features, int in_features,
                                                     uint8_t* slice_groups) {
  PK_G16_FORWARD_IF(slices_log2 == 5, packed_plan_geometry, slice_steps, slices_log2, out_features, in_features, slice_groups);
  if (!slice_steps || !slice_groups || slices_log2 != PK_S_LOG) {
    set_last_error("aqlm_hip_packed_plan_geometry: null pointer or slices_log2 not 4 / 5");
    return AQLM_HIP_E_INVALID;
  }
  unsigned long long st[PK_S];
  for (int s = 0; s < PK_S; ++s) st[s] = slice_steps[s];
  return plan_geometry(st, out_features, in_features, slice_groups);
}

// scratch of the repack, kept in the tail of the caller's capacity: usage counts, the relabelling table, lane-steps per
// (slice, row), lane-steps per slice
struct PkScratch {
  size_t off_hist, off_relabel, off_ls, off_steps, bytes;
};
static PkScratch pk_scratch(int M) {
  PkScratch sc;
  sc.off_hist = 0;
  sc.off_relabel = sc.off_hist + (size_t)65536 * 4;
  sc.off_ls = sc.off_relabel + (size_t)65536 * 2;
  sc.off_steps = align_up(sc.off_ls + (size_t)PK_S * M * 2, 256);
  sc.bytes = align_up(sc.off_steps + PK_S * 4, 1024);
  return sc;
}

extern "C" PK_API size_t PK_ENTRY(prepack_1x16_bytes)(int out_features, int in_features, int in_group_size) {
  PK_G16_FORWARD_IF(in_group_size == 16, prepack_1x16_bytes, out_features, in_features, in_group_size);
  if (!packed_shape_ok(out_features, in_features, in_group_size)) return 0;
  // capacity for streams up to 1.5 x the balanced length (the repack balances the slices; what is left is the difference
  // between the rows of one slice), plus the permutation + codebook image of a relabelled buffer and the repack's scratch;
  // the bytes actually used come back in the descriptor and the buffer may be trimmed to them
  const size_t nst = (size_t)PK_NST;
  const size_t M = (size_t)out_features;
  const size_t RG2 = (M + PK_MIN_GROUPS - 1) / PK_MIN_GROUPS;                 // rows per group at most (variable geometry)
  const size_t in_groups = (size_t)in_features / PK_G;
  const size_t fair = (M * in_groups / 4 + (size_t)PK_S * M) / nst;            // lane-steps per stream when all are equal
  const size_t lane_steps = fair * 3 / 2 + RG2 + 64;                           // per stream
  const size_t ent = nst * (lane_steps * 16 + 16 * 1024);
  const size_t meta = 4096 + nst * PK_MAX_NW * 16 + nst * (RG2 + 1) * 4 + (size_t)AQLM_HIP_MAX_GEMV_BATCH * out_features * 8;
  const size_t image = (size_t)65536 * 2 + (size_t)65536 * PK_VB + 2048;
  // 3-byte entries: the repack builds the 4-byte layout in the tail of the buffer and squeezes it to the front
  return align_up(meta + ent + ent * PK_WREG3 / 1024 + image + pk_scratch(out_features).bytes + 4096, 1024);
}

extern "C" PK_API int PK_ENTRY(prepack_1x16_ex)(const void* codes, int out_features, int in_features, int in_group_size,
                                                void* packed, size_t packed_bytes, aqlm_hip_packed_desc* desc, int flags, void* stream_) {
  PK_G16_FORWARD_IF(in_group_size == 16, prepack_1x16_ex, codes, out_features, in_features, in_group_size, packed, packed_bytes, desc, flags, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  if (!codes || !packed || !desc) {
    set_last_error("aqlm_hip_prepack_1x16: null pointer argument");
    return AQLM_HIP_E_INVALID;
  }
  if (!packed_shape_ok(out_features, in_features, in_group_size)) {
    set_last_error("aqlm_hip_prepack_1x16: unsupported shape (needs g=%d, in/g <= %d; got g=%d in=%d out=%d)", PK_G, PK_MAX_GROUPS,
                   in_group_size, in_features, out_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t cap = PK_ENTRY(prepack_1x16_bytes)(out_features, in_features, in_group_size);
  if (packed_bytes < cap || !aligned16(packed)) {
    set_last_error("aqlm_hip_prepack_1x16: packed buffer needs %zu bytes (16-B aligned), got %zu", cap, packed_bytes);
    return AQLM_HIP_E_INVALID;
  }
  const int M = out_features, in_groups = in_features / PK_G;
  const size_t nst = (size_t)PK_NST;
  uint8_t* base = (uint8_t*)packed;
  const PkScratch sc = pk_scratch(M);
  const size_t work_end = (packed_bytes - sc.bytes) / 1024 * 1024;  // the layout (and the 4-byte working copy of 3-byte entries) stay below
  uint8_t* scratch = base + work_end;
  uint32_t* hist_d = (uint32_t*)(scratch + sc.off_hist);
  uint16_t* relabel_d = (uint16_t*)(scratch + sc.off_relabel);
  uint16_t* ls_d = (uint16_t*)(scratch + sc.off_ls);
  uint32_t* steps_d = (uint32_t*)(scratch + sc.off_steps);
  const int row_blocks = (M + 3) / 4;
  uint32_t* maxL_d = (uint32_t*)(base + 128);
  uint8_t groups[32] = {};
  for (int s = 0; s < PK_S; ++s) groups[s] = (uint8_t)PK_NG;
  std::vector<uint16_t> new_of_old, old_of_new;
  bool relabel = false;
  uint32_t steps_h[PK_S];
  uint32_t maxL = 0;
  // wave-steps a workgroup runs when its longest stream has L lane-steps (what the balancing can change at all: the kernel
  // runs whole steps of whole waves)
  auto capacity = [](uint32_t L) {
    const int nw = choose_waves(L);
    return (uint64_t)nw * ((L + 64u * nw - 1) / (64u * nw));
  };
  // counts lane-steps per (slice, row) with the given labels, builds the row starts of every stream for `groups` in place (their
  // offset does not depend on the wave count chosen later) and reads back the longest stream
  PackedLayout L0;
  auto count_and_scan = [&](const uint16_t* rl) -> int {
    if (!packed_layout(M, in_features, 1, 1, L0, 1, 4, groups, relabel)) {
      set_last_error("aqlm_hip_prepack_1x16: internal: geometry plan rejected");
      return AQLM_HIP_E_INVALID;
    }
    if (L0.off_ent > work_end) {
      set_last_error("aqlm_hip_prepack_1x16: capacity too small for the row tables");
      return AQLM_HIP_E_INVALID;
    }
    if (int e = check_hip(hipMemsetAsync(base, 0, L0.off_ent, stream), "prepack memset")) return e;
    if (int e = check_hip(hipMemsetAsync(steps_d, 0, PK_S * 4, stream), "prepack memset")) return e;
    hipLaunchKernelGGL(pk_count_kernel, dim3(row_blocks), dim3(256), 0, stream, (const uint16_t*)codes, rl, ls_d, steps_d, M, in_groups);
    hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)nst), dim3(256), 0, stream, ls_d, (uint32_t*)(base + L0.off_rowstart), maxL_d, L0.G);
    if (int e = check_hip(hipMemcpyAsync(steps_h, steps_d, PK_S * 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
    if (int e = check_hip(hipMemcpyAsync(&maxL, maxL_d, 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
    return check_hip(hipStreamSynchronize(stream), "prepack sync");
  };
  // (1) the checkpoint's labels on the 16 x 16 geometry
  if (int e = count_and_scan(nullptr)) return e;
  // Balancing is for the longest stream: when it already runs as few wave-steps as perfectly even streams would (+3.5 %: the
  // noise between the row groups of uniform codes), labels and geometry stay -- no permutation, no codebook image.
  unsigned long long total_steps = 0;
  for (int s = 0; s < PK_S; ++s) total_steps += steps_h[s];
  const uint32_t even = (uint32_t)((total_steps * 1035ull + (unsigned long long)PK_NST * 1000ull - 1ull) / ((unsigned long long)PK_NST * 1000ull));
  const bool balanced = capacity(maxL) <= capacity(even);
  if (!balanced) {
    // (2) usage counts -> relabelling plan -> lane-steps with the new labels
    if (!(flags & AQLM_HIP_PREPACK_NO_RELABEL)) {
      std::vector<uint32_t> usage(65536);
      if (int e = check_hip(hipMemsetAsync(hist_d, 0, (size_t)65536 * 4, stream), "prepack memset")) return e;
      hipLaunchKernelGGL(pk_hist_kernel, dim3(2048), dim3(256), 0, stream, (const uint16_t*)codes, (size_t)M * in_groups, hist_d);
      if (int e = check_hip(hipMemcpyAsync(usage.data(), hist_d, (size_t)65536 * 4, hipMemcpyDeviceToHost, stream), "prepack read-back")) return e;
      if (int e = check_hip(hipStreamSynchronize(stream), "prepack sync")) return e;
      new_of_old.resize(65536);
      // forced: the layout is not balanced although the global masses may be (label use correlated with the row); kept only when
      // the longest stream runs fewer wave-steps with the new labels
      const uint32_t maxL_before = maxL;
      relabel = plan_relabel(usage.data(), new_of_old.data(), /*force=*/true) == 1;
      if (relabel) {
        old_of_new.resize(65536);
        for (uint32_t c = 0; c < 65536; ++c) old_of_new[new_of_old[c]] = (uint16_t)c;
        if (int e = check_hip(hipMemcpyAsync(relabel_d, new_of_old.data(), (size_t)65536 * 2, hipMemcpyHostToDevice, stream), "prepack relabel table")) return e;
        if (int e = count_and_scan(relabel_d)) return e;
        if (capacity(maxL) >= capacity(maxL_before)) {  // the deal did not help (e.g. one row that lives in one slice): labels as they are
          relabel = false;
          if (int e = count_and_scan(nullptr)) return e;
        }
      }
    }
    // (3) an entry that outweighs a slice: deal the workgroups to the slices by their work
    if (!(flags & AQLM_HIP_PREPACK_UNIFORM_ONLY)) {
      unsigned long long steps64[PK_S];
      for (int s = 0; s < PK_S; ++s) steps64[s] = steps_h[s];
      if (plan_geometry(steps64, M, in_features, groups))
        if (int e = count_and_scan(relabel ? relabel_d : nullptr)) return e;
    }
  }
  const uint16_t* rl = relabel ? relabel_d : nullptr;
  const PkGeom G = L0.G;
  uint32_t* a = (uint32_t*)(base + L0.off_rowstart);
  const int NW = choose_waves(maxL);
  const int T = (int)((maxL + 64u * NW - 1) / (64u * NW));
  const bool arrange = tuning().packed_arrange && T <= PK_ARR_MAX_T;
  // rotated copies of x: 1 by default -- with the row pools the x reads are already spread well, and up to 4 copies
  // measured within +-1 % (profiles/r02_mb_packed_variants.log); the knob keeps the mechanism testable
  int XC = 1;
  if (AQLM_PK_XFIRST && PK_G == 8 && arrange && !packed_b1_slice_first(in_groups, G.RG) && tuning().packed_xcopies >= 1 && tuning().packed_xcopies <= 4) XC = std::min(pk_max_x_copies(in_groups), tuning().packed_xcopies);
  // 32-bit entries by default (two operations instead of four to form an entry's addresses); 24-bit entries (-23 % bytes; wave
  // ranges of at most 32 steps) are the compact choice for inference-only deployments.  Re-measured per shape in round 5 (profiles/r05_entry_bytes_3_vs_4.md, A/B/A/B on one box): 24-bit
  // entries cost 5.8 % on 4096 x 4096, 3.3 % on 4096 -> 11008, 3.2 % on 4096 -> 1024, 2.3 % on 8192 x 8192 and 1.3-1.4 % on
  // 4096 <-> 14336; layers of more than 32 steps per wave (the 70B MLP) cannot take them at all.  They also keep a shared-input group
  // off the pipelined kernel (4-byte entries only).  So they stay the opt-in compact form (tuning key 3, `prepack_model(compact=True)`).
  const int EB = (PK_G == 8 && tuning().packed_entry_bytes == 3 && T <= 32 && !G.vg) ? 3 : 4;  // (the 3-byte form exists for 16-B vectors and uniform geometry only)
  PackedLayout L, L4;
  if (!packed_layout(M, in_features, NW, T, L, XC, EB, groups, relabel) || !packed_layout(M, in_features, NW, T, L4, XC, 4, groups, relabel) ||
      L.used + (EB == 3 ? L4.ent_bytes + 1024 : 0) > work_end) {
    set_last_error("aqlm_hip_prepack_1x16: the rows of this layer use the codebook too differently from one another for the packed "
                   "format (longest stream %u lane-steps after balancing, %d steps per wave)", maxL, T);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  uint32_t* winfo = (uint32_t*)(base + L.off_winfo);
  // the 4-byte working layout: in place for 4-byte entries, else in the tail of the capacity
  uint32_t* ent = EB == 4 ? (uint32_t*)(base + L.off_ent) : (uint32_t*)(base + (work_end - L4.ent_bytes) / 1024 * 1024);
  aqlm_hip_packed_desc d{};
  d.magic = PK_MAGIC;
  d.version = PK_VERSION;
  d.out_features = M;
  d.in_features = in_features;
  d.slices_log2 = PK_S_LOG;
  d.waves = NW;
  d.steps = T;
  d.entry_bytes = EB;
  d.used_bytes = L.used;
  d.x_copies = (uint32_t)XC;
  d.codebook_absmax = 0.f;  // unknown: the caller sets it (see include/aqlm_hip.h) to enable the fused finalize
  d.flags = (relabel ? AQLM_HIP_PACKED_RELABELLED : 0u) | (G.vg ? AQLM_HIP_PACKED_VARGEOM : 0u);
  d.rows_per_group = G.RG;
  for (int s = 0; s < PK_S; ++s) d.slice_groups[s] = groups[s];
  if (int e = check_hip(hipMemcpyAsync(base, &d, sizeof(d), hipMemcpyHostToDevice, stream), "prepack header")) return e;
  const uint32_t null_entry = (uint32_t)in_groups << (16 + PK_VSH);
  hipLaunchKernelGGL(pk_fill_kernel, dim3(2048), dim3(256), 0, stream, ent, L4.ent_bytes / 4, null_entry);
  hipLaunchKernelGGL(pk_scatter_kernel, dim3(row_blocks), dim3(256), 0, stream, (const uint16_t*)codes, rl, a, ent, G, in_groups, NW, T);
  if (arrange)
    hipLaunchKernelGGL(pk_arrange_kernel, dim3((unsigned)nst, NW), dim3(64), (size_t)T * 1024 + (size_t)T * 256, stream, a,
                       ent, G, in_groups, NW, T, XC);
  // the local search on the greedy deal (1-3 % faster matvec) takes ~10x the greedy deal's time (27 -> 120 ms for a 29 M-code
  // layer): by default (1) only layers of <= 8 Mi codes get it -- a 70B model then prepacks in ~13 s instead of ~1 min --,
  // 3 = always, 2 = never
  if (arrange && (tuning().packed_arrange == 3 || (tuning().packed_arrange == 1 && (long)M * in_groups <= PK_IMPROVE_MAX_CODES)))
    hipLaunchKernelGGL(pk_improve_kernel, dim3((unsigned)nst, NW), dim3(64), (size_t)T * (1024 + 512 + 256 + 32), stream, a, ent, G,
                       in_groups, NW, T);
  if (PK_PARITY_BITS) hipLaunchKernelGGL(pk_parity_kernel, dim3(2048), dim3(256), 0, stream, ent, L4.ent_bytes / 4);
  hipLaunchKernelGGL(pk_flag_kernel, dim3((G.RG + 255) / 256, (unsigned)nst), dim3(256), 0, stream, a, ent, G, NW, T);
  hipLaunchKernelGGL(pk_column_kernel, dim3((unsigned)nst, NW), dim3(64), 0, stream, a, ent, winfo, G, NW, T);
  if (EB == 3)
    hipLaunchKernelGGL(pk_compress_kernel, dim3((unsigned)nst, NW), dim3(64), 0, stream, ent, base + L.off_ent, winfo, G, NW, T);
  if (int e = check_hip(hipGetLastError(), "prepack launch")) return e;
  if (relabel) {  // the permutation travels with the buffer: unpack and the codebook image are made from it
    if (int e = check_hip(hipMemcpyAsync(base + L.off_perm, old_of_new.data(), (size_t)65536 * 2, hipMemcpyHostToDevice, stream), "prepack permutation")) return e;
  }
  if (int e = check_hip(hipStreamSynchronize(stream), "prepack sync")) return e;  // `d` and the tables live on the host stack / heap
  *desc = d;
  return 0;
}

extern "C" PK_API int PK_ENTRY(prepack_1x16)(const void* codes, int out_features, int in_features, int in_group_size,
                                      void* packed, size_t packed_bytes, aqlm_hip_packed_desc* desc, void* stream_) {
  return PK_ENTRY(prepack_1x16_ex)(codes, out_features, in_features, in_group_size, packed, packed_bytes, desc, 0, stream_);
}

// codebook image of a relabelled buffer: image[new] = codebook[old_of_new[new]], one 16-B piece per thread
namespace aqlm {
namespace PK_NS {
__global__ __launch_bounds__(256) void pk_codebook_image_kernel(const uint16_t* old_of_new, const u32x4* codebook, u32x4* image) {
  constexpr uint32_t PIECES = PK_VB / 16;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // < 65536 * PIECES
  const uint32_t c = i / PIECES, h = i - c * PIECES;
  image[i] = codebook[(uint32_t)old_of_new[c] * PIECES + h];
}
}  // namespace PK_NS
}  // namespace aqlm

extern "C" PK_API int PK_ENTRY(packed_set_codebook)(aqlm_hip_packed_desc* desc, void* packed, const void* codebook, void* stream_) {
  PK_G16_FORWARD(desc, packed_set_codebook, desc, packed, codebook, stream_);
  PackedLayout L;
  if (!packed || !codebook || !desc_layout(desc, L) || !aligned16(packed) || !aligned16(codebook)) {
    set_last_error("aqlm_hip_packed_set_codebook: null / misaligned pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  if (!L.relabel) return 0;  // the kernels read the caller's codebook
  uint8_t* base = (uint8_t*)packed;
  hipLaunchKernelGGL(pk_codebook_image_kernel, dim3(65536u * (PK_VB / 16) / 256u), dim3(256), 0, (hipStream_t)stream_,
                     (const uint16_t*)(base + L.off_perm), (const u32x4*)codebook, (u32x4*)(base + L.off_cb));
  if (int e = check_hip(hipGetLastError(), "codebook image launch")) return e;
  desc->flags |= AQLM_HIP_PACKED_HAS_CODEBOOK;
  return 0;
}

extern "C" PK_API int PK_ENTRY(packed_desc_read)(const void* header_host, size_t header_bytes, aqlm_hip_packed_desc* desc) {
  if (header_host && desc && header_bytes >= sizeof(aqlm_hip_packed_desc)) {
    aqlm_hip_packed_desc h;
    memcpy(&h, header_host, sizeof(h));
    PK_G16_FORWARD(&h, packed_desc_read, header_host, header_bytes, desc);
  }
  if (!header_host || !desc || header_bytes < sizeof(aqlm_hip_packed_desc)) {
    set_last_error("aqlm_hip_packed_desc_read: need the first %zu bytes of the packed buffer", sizeof(aqlm_hip_packed_desc));
    return AQLM_HIP_E_INVALID;
  }
  aqlm_hip_packed_desc d;
  memcpy(&d, header_host, sizeof(d));
  PackedLayout L;
  if (!desc_layout(&d, L)) {
    set_last_error("aqlm_hip_packed_desc_read: not a packed 1x16 buffer of format v6");
    return AQLM_HIP_E_INVALID;
  }
  *desc = d;
  return 0;
}

extern "C" PK_API int PK_ENTRY(unpack_1x16)(const aqlm_hip_packed_desc* desc, const void* packed, void* codes, void* stream_) {
  PK_G16_FORWARD(desc, unpack_1x16, desc, packed, codes, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  if (!packed || !codes || !desc_layout(desc, L)) {
    set_last_error("aqlm_hip_unpack_1x16: null pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint16_t* perm = L.relabel ? (const uint16_t*)(base + L.off_perm) : nullptr;  // relabelled: back to the checkpoint's labels
  if (L.EB == 3)
    hipLaunchKernelGGL(pk_unpack3_kernel, dim3((unsigned)L.nst, L.NW), dim3(64), 0, stream, base + L.off_ent,
                       (const uint32_t*)(base + L.off_winfo), perm, (uint16_t*)codes, L.G, L.in_groups, L.NW, L.T);
  else
    hipLaunchKernelGGL(pk_unpack_kernel, dim3((unsigned)L.nst, L.NW), dim3(64), 0, stream, (const uint32_t*)(base + L.off_ent),
                       (const uint32_t*)(base + L.off_winfo), perm, (uint16_t*)codes, L.G, L.in_groups, L.NW, L.T);
  return check_hip(hipGetLastError(), "unpack launch");
}

// W from the packed buffer (pk_dequant_kernel).  Reads the entries, the permutation stored behind them and the CALLER's codebook:
// never the permuted codebook image, whose flag and the descriptor's codebook range are not looked at.
extern "C" PK_API int PK_ENTRY(dequant_1x16_packed)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                    const void* scales, void* W, int dtype, void* stream_) {
  PK_G16_FORWARD(desc, dequant_1x16_packed, desc, packed, codebook, scales, W, dtype, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  if (!packed || !codebook || !W || !desc_layout(desc, L)) {
    set_last_error("aqlm_hip_dequant_1x16_packed: null pointer or invalid descriptor");
    return AQLM_HIP_E_INVALID;
  }
  if (!aligned16(packed) || !aligned16(codebook) || !aligned16(W)) {
    set_last_error("aqlm_hip_dequant_1x16_packed: packed, codebook and W must be 16-byte aligned");
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("aqlm_hip_dequant_1x16_packed: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)", dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint16_t* perm = L.relabel ? (const uint16_t*)(base + L.off_perm) : nullptr;
  // grid order (measured, profiles/packed_dequant.json): one row group per XCD is 7 % / 4 % faster at 4096 x 4096 / 8192 -> 28672 and 2 %
  // slower at 4096 <-> 14336 for 16-B vectors; with 32-B vectors (a quarter of a line per store) the stream-major grid is 6 % faster
  const int knob = tuning().packed_dequant_by_xcd;
  const int by_xcd = !L.G.vg && (knob == 2 || (knob == 1 && PK_G == 8)) ? 1 : 0;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)(L.nst * L.NW)), dim3(64), 0, stream, base + L.off_ent, (const uint32_t*)(base + L.off_winfo), perm,
                       (const u32x4*)codebook, (const uint16_t*)scales, (uint16_t*)W, L.G, L.in_groups, L.NW, L.T, by_xcd);
    return check_hip(hipGetLastError(), "packed dequant launch");
  };
#define AQLM_PK_DQ(TT, EE) (perm ? go(pk_dequant_kernel<TT, EE, true>) : go(pk_dequant_kernel<TT, EE, false>))
#if AQLM_PK_G == 8
  if (L.EB == 3) return dtype == AQLM_HIP_F16 ? AQLM_PK_DQ(F16, 3) : AQLM_PK_DQ(BF16, 3);
#endif
  return dtype == AQLM_HIP_F16 ? AQLM_PK_DQ(F16, 4) : AQLM_PK_DQ(BF16, 4);
#undef AQLM_PK_DQ
}

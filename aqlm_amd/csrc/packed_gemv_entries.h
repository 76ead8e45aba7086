// Part of gemv_packed.hip (after `using namespace aqlm::PK_NS`), host only: the launch of the matvec kernels (packed_fused,
// packed_launch_main, packed_check_args) and the C entries of the single-layer matvec and of the shared-input (multi) one.
// Needs packed_format.h, the kernels and structs of packed_gemv_kernels.h and packed_pipe_kernel.h, and packed_launch.h.

// The fused finalize needs the layer's codebook range (descriptor field) and can be switched off for A/B runs.
static bool packed_fused(const aqlm_hip_packed_desc* desc) {
  return tuning().packed_fused_finalize != 0 && desc->codebook_absmax > 0.f && desc->codebook_absmax < __builtin_inff();
}

// main kernel of one launch (<= packed_max_batch rows).  With `fused.y` it also finalizes (accumulator cells inside the
// packed buffer, no workspace); without, it leaves fp32 slice partials [16][nb][M] in the workspace.
struct PackedFused {
  const void* scales = nullptr;
  const void* bias = nullptr;
  void* y = nullptr;
  long y_row_stride = 0;
  float cb_absmax = 0.f;
  void* cells = nullptr;  // caller-owned accumulator cells [rows][M] u64, zero at rest (one set per stream); null: the cells inside the packed buffer
  // row-parallel shard: publish the fp32 totals (aqlm_hip_gemv_1x16_packed_publish) instead of writing y
  float* pub = nullptr;
  uint32_t* pub_flag = nullptr;
  uint32_t* pub_epoch = nullptr;
  uint32_t pub_max_elems = 0;
};

// the layer that runs next on the stream (chain prefetch); all null = none
struct PackedNext {
  const uint8_t* ent = nullptr;
  const uint8_t* codebook = nullptr;
  uint32_t block_bytes = 0;
};

// Chain prefetch, the rules the chain entry and its report (aqlm_hip_gemv_1x16_packed_chain_plan) share.
// What the prefetch waves are told about the next layer (chain_hint.h): nothing for a variable-geometry buffer (the hint assumes
// workgroup b of both layers sits on one XCD with the same slice), and nothing where their whole-KiB requests would run past the
// buffer's last byte (3-byte entries that end the buffer).
static chain_hint::Hint packed_chain_hint(const PackedLayout& LN) {
  return chain_hint::decide(LN.off_ent, LN.ent_bytes, (int)LN.nst, LN.used, LN.G.vg != 0);
}
// prefetch waves a launch of L asks for when a next layer is named: the tuning key's count (0 = 2, negative = none), at most 7 and
// at most what 16 waves leave beside the stream's own (the launch drops them all if the image with their dump zones does not fit)
static int packed_chain_waves(const PackedLayout& L) {
  const int want = tuning().packed_prefetch_waves < 0 ? 0 : (tuning().packed_prefetch_waves == 0 ? 2 : tuning().packed_prefetch_waves);
  return std::min(std::min(want, 7), PK_MAX_NW - L.NW);
}

static int packed_launch_main(const PackedLayout& L, const void* packed, const void* codebook, const uint16_t* x, int nb,
                              long x_row_stride, int dtype, void* workspace, size_t workspace_bytes, hipStream_t stream,
                              const char* who, const PackedFused& fused = PackedFused{}, const PackedNext& next = PackedNext{},
                              CaptureRelax* relax = nullptr) {
  const bool finalizes = fused.y || fused.pub;
  const size_t need = finalizes ? 0 : (size_t)PK_S * nb * L.M * sizeof(float);
  if (need && (!workspace || workspace_bytes < need)) {
    set_last_error("%s: workspace of %zu bytes required, got %zu", who, need, workspace_bytes);
    return AQLM_HIP_E_INVALID;
  }
  const uint8_t* base = (const uint8_t*)packed;
  const uint32_t* ent = (const uint32_t*)(base + L.off_ent);
  const uint32_t* rowstart = (const uint32_t*)(base + L.off_rowstart);
  const uint8_t* cb = L.relabel ? base + L.off_cb : (const uint8_t*)codebook;  // relabelled: the permuted image (aqlm_hip_packed_set_codebook)
  // the trailing kernel argument as both launches below pass it; the ordinary one adds the publish and next-layer fields
  PackedGemvRest rest{};
  rest.winfo = (const uint32_t*)(base + L.off_winfo);
  rest.partial = (float*)workspace;
  rest.x_row_stride = x_row_stride;
  if (finalizes) {
    rest.acc = fused.cells ? (unsigned long long*)fused.cells : (unsigned long long*)(const_cast<uint8_t*>(base) + L.off_acc);
    rest.cb_absmax = fused.cb_absmax;
    rest.scales = (const uint16_t*)fused.scales;
    rest.bias = (const uint16_t*)fused.bias;
    rest.y = (uint16_t*)fused.y;
    rest.y_row_stride = fused.y_row_stride;
  }
#ifdef AQLM_PACKED_TRACE
  rest.trace = workspace && workspace_bytes >= need + (size_t)PK_NST * PK_MAX_NW * 8 * 8 ? (unsigned long long*)((uint8_t*)workspace + need) : nullptr;
  rest.dbg = tuning().packed_debug;
#endif
  // chain prefetch: up to `packed_prefetch_waves` extra waves per workgroup (default 2) when a next layer is named
  int npw = 0;
  if (next.ent && next.codebook && next.block_bytes) npw = packed_chain_waves(L);
  const uint32_t rotate = tuning().packed_fill_rotate ? 1u : 0u;
#if AQLM_PK_G == 8
  // Capture overlap, grouped launches (capture_overlap.h): a one-row launch of a compact-window instance that finalizes into y
  // is one grid of 256 workgroups, and gemv_1x16_packed_group_kernel runs up to PK_GROUP_MAX such grids of one instance, block
  // size and LDS image as one.  When the planner lets this launch join a node, the node is rewritten to the grouped kernel
  // with this layer as one more segment and nothing is launched.  `joined` false: launch as usual (begin() has been called).
  // `member` holds the launch as it would be made (capture_member_launch); the grouped forms are added here, and the whole
  // travels with the planner, which may also regroup the launch later ("Regrouping the head").
  static_assert(sizeof(PackedGroupSegment) <= CaptureMember::kSegBytes && sizeof(PackedGroupSegment) % 8 == 0 &&
                    sizeof(PackedGroupParams) == (size_t)capture_overlap::kMaxMerge * sizeof(PackedGroupSegment),
                "capture_build_node lays the segments out as PackedGroupParams");
  auto try_join = [&](bool vg, const PackedGroupSegment& me, unsigned threads, size_t lds, CaptureMember& member, bool& joined) -> int {
    joined = false;
    if (tuning().packed_capture_merge <= 1) {
      if (relax) relax->begin(0, member.func ? &member : nullptr, sizeof member);
      return 0;
    }
    const void* gk = vg ? (dtype == AQLM_HIP_F16 ? (const void*)gemv_1x16_packed_group_kernel<F16, 3, PK_XWIN_COMPACT, 4, true>
                                                 : (const void*)gemv_1x16_packed_group_kernel<BF16, 3, PK_XWIN_COMPACT, 4, true>)
                        : (dtype == AQLM_HIP_F16 ? (const void*)gemv_1x16_packed_group_kernel<F16, 3, PK_XWIN_COMPACT, 4, false>
                                                 : (const void*)gemv_1x16_packed_group_kernel<BF16, 3, PK_XWIN_COMPACT, 4, false>);
    if (int e = ensure_dynamic_lds(gk, lds)) return e;  // on eager launches too: the attribute is in place before a capture needs it
    // the folded form of the node (group_fold.h; ordinary geometry only): same image, same block size, 256 / F workgroups per member
    const void* fk = vg ? nullptr
                        : (dtype == AQLM_HIP_F16 ? (const void*)gemv_1x16_packed_group_fold_kernel<F16, 3, PK_XWIN_COMPACT, 4>
                                                 : (const void*)gemv_1x16_packed_group_fold_kernel<BF16, 3, PK_XWIN_COMPACT, 4>);
    if (fk)
      if (int e = ensure_dynamic_lds(fk, lds)) return e;
    if (!relax) return 0;
    uint64_t key = (uint64_t)reinterpret_cast<uintptr_t>(gk) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)threads << 32) ^ (uint64_t)lds;
    if (key == 0) key = 1;
    // The folded kernel finalizes one row per thread (a second row's loads would stand in front of the next pass's ring): a
    // layer with more rows in a group than the block has threads keeps its node unfolded (capture_build_node).
    member.group_func = gk;
    member.fold_func = fk;
    member.seg_bytes = (unsigned)sizeof me;
    member.rows_per_group = me.RG;
    memcpy(member.seg, &me, sizeof me);
    if (relax->begin(key, &member, sizeof member) > 0) joined = relax->join_members();
    return 0;
  };
#endif
  auto launch = [&](auto kern, auto lds_map) -> int {
    const size_t lds = decltype(lds_map)::total(L.in_groups, L.RG, npw, L.NW);
    if (lds > 160 * 1024) { npw = 0; }
    const size_t lds_final = decltype(lds_map)::total(L.in_groups, L.RG, npw, L.NW);
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_final)) return e;
    PackedGemvRest r = rest;
    r.pub = fused.pub;
    r.pub_flag = fused.pub_flag;
    r.pub_epoch = fused.pub_epoch;
    r.pub_max_elems = fused.pub_max_elems;
    if (npw) {
      r.next_ent = next.ent;
      r.next_codebook = next.codebook;
      r.next_block_bytes = next.block_bytes;
    }
    bool joined = false;
    const uint32_t geom = (uint32_t)L.NW | ((uint32_t)L.XC << 8) | ((uint32_t)npw << 12) | (rotate << 15) | ((uint32_t)L.T << 16);
    // the launch below, for the planner (a launch whose arguments do not fit travels without: it is never moved)
    CaptureMember member{};
    const bool described = relax && relax->capturing() &&
                           capture_member_launch(member, kern, (unsigned)PK_NST, (unsigned)(L.NW + npw) * 64u, lds_final, cb, x, ent, rowstart,
                                                 L.in_groups, geom, L.RG, (uint32_t)L.ent_bytes, L.M, r);
#if AQLM_PK_G == 8
    if (decltype(lds_map)::TIGHT && nb == 1 && npw == 0 && fused.y && !fused.pub) {
      PackedGroupSegment me{};
      me.codebook = cb;
      me.x = x;
      me.ent = ent;
      me.rowstart = rowstart;
      me.in_groups = L.in_groups;
      me.RG = L.RG;
      me.M = L.M;
      me.geom = (uint32_t)L.NW | ((uint32_t)L.XC << 8) | (rotate << 15) | ((uint32_t)L.T << 16);
      me.ent_bytes = (uint32_t)L.ent_bytes;
      me.rest = r;
      if (int e = try_join(false, me, (unsigned)L.NW * 64u, lds_final, member, joined)) return e;
    } else
#endif
    if (relax) relax->begin(0, described ? &member : nullptr, sizeof member);
    if (joined) return 0;
    hipLaunchKernelGGL(kern, dim3(PK_NST), dim3((L.NW + npw) * 64), lds_final, stream, cb, x, ent, rowstart, L.in_groups, geom, L.RG,
                       (uint32_t)L.ent_bytes, L.M, r);
    return check_hip(hipGetLastError(), "gemv_1x16_packed launch");
  };
  const bool sf = nb == 1 && packed_b1_slice_first(L.in_groups, L.RG);
  const bool compact = nb == 1 && packed_b1_compact(L, packed_b1_pd(L));
#if AQLM_PK_G == 8
  if (L.G.vg) {  // variable geometry: its own kernels (4-byte entries, ring depth 3 / 4, no chain prefetch, no publish)
    if (fused.pub != nullptr || L.EB != 4) {
      set_last_error("%s: a variable-geometry buffer runs on the single-layer matvec entries only (repack with "
                     "AQLM_HIP_PREPACK_UNIFORM_ONLY for the publish form)", who);
      return AQLM_HIP_E_UNSUPPORTED;
    }
    uint32_t ns[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < PK_S; ++i) ns[i >> 2] |= (uint32_t)L.G.first[i] << ((i & 3) * 8);  // first stream of every slice (< 256)
    auto launch_vg = [&](auto kern, auto lds_map) -> int {
      const size_t lds = decltype(lds_map)::total(L.in_groups, L.RG, 0, L.NW);
      if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
      bool joined = false;
      const uint32_t geom = (uint32_t)L.NW | ((uint32_t)L.XC << 8) | (rotate << 15) | ((uint32_t)L.T << 16);
      CaptureMember member{};
      const bool described = relax && relax->capturing() &&
                             capture_member_launch(member, kern, (unsigned)PK_NST, (unsigned)L.NW * 64u, lds, cb, x, ent,
                                                   (uint32_t)(L.off_ent - L.off_rowstart), (uint32_t)L.in_groups | ((uint32_t)L.RG << 12), geom, L.M,
                                                   ns[0], ns[1], ns[2], ns[3], rest);
      if (decltype(lds_map)::TIGHT && nb == 1 && fused.y) {
        PackedGroupSegment me{};
        me.codebook = cb;
        me.x = x;
        me.ent = ent;
        me.rowstart = rowstart;
        me.in_groups = L.in_groups;
        me.RG = L.RG;
        me.M = L.M;
        me.geom = (uint32_t)L.NW | ((uint32_t)L.XC << 8) | (rotate << 15) | ((uint32_t)L.T << 16);
        me.ent_bytes = (uint32_t)PK_NST * (uint32_t)L.NW * (uint32_t)L.T * 1024u;  // as the variable-geometry kernel derives it
        for (int i = 0; i < 4; ++i) me.ns[i] = ns[i];
        me.rest = rest;
        if (int e = try_join(true, me, (unsigned)L.NW * 64u, lds, member, joined)) return e;
      } else if (relax) {
        relax->begin(0, described ? &member : nullptr, sizeof member);
      }
      if (joined) return 0;
      hipLaunchKernelGGL(kern, dim3(PK_NST), dim3(L.NW * 64), lds, stream, cb, x, ent, (uint32_t)(L.off_ent - L.off_rowstart),
                         (uint32_t)L.in_groups | ((uint32_t)L.RG << 12), geom, L.M, ns[0], ns[1], ns[2], ns[3], rest);
      return check_hip(hipGetLastError(), "gemv_1x16_packed (variable geometry) launch");
    };
    return dispatch_packed_vg(dtype, nb, sf, compact, launch_vg);
  }
#endif
  if (fused.pub != nullptr) return dispatch_packed<PublishKernels>(dtype, nb, pick_pd(L), L.EB, sf, false, launch);
  return dispatch_packed<SingleKernels>(dtype, nb, pick_pd(L), L.EB, sf, compact, launch);
}

static int packed_check_args(const char* who, const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                             const void* x, int batch, long& x_row_stride, int dtype, PackedLayout& L, int& max_b) {
  if (!packed || !codebook || !x || !desc) {
    set_last_error("%s: null pointer argument", who);
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("%s: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)", who, dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (!desc_layout(desc, L)) {
    set_last_error("%s: invalid packed descriptor", who);
    return AQLM_HIP_E_INVALID;
  }
  if (int e = check_x_row_stride(who, batch, desc->in_features, x_row_stride)) return e;
  if (batch < 1 || batch > AQLM_HIP_MAX_GEMV_BATCH || !aligned16(packed) || !aligned16(codebook) || !aligned16(x) ||
      (batch > 1 && x_row_stride % 8 != 0)) {
    set_last_error("%s: batch must be 1..%d and packed / codebook / x rows 16-B aligned (batch %d)", who,
                   AQLM_HIP_MAX_GEMV_BATCH, batch);
    return AQLM_HIP_E_INVALID;
  }
  if (L.relabel && !(desc->flags & AQLM_HIP_PACKED_HAS_CODEBOOK)) {
    set_last_error("%s: a relabelled buffer needs its codebook image: call aqlm_hip_packed_set_codebook first (and again whenever "
                   "the codebook changes)", who);
    return AQLM_HIP_E_INVALID;
  }
  max_b = packed_max_batch(L.in_groups, L.RG);
  if (max_b == 0) {
    set_last_error("%s: layer does not fit the LDS image (in_features %d)", who, desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return 0;
}

static int gemv_1x16_packed_impl(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                 const void* scales, const void* bias, const void* x, void* y, int batch,
                                 long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                 size_t workspace_bytes, void* stream_, const PackedNext& next, void* cells = nullptr,
                                 size_t cells_bytes = 0) {
  hipStream_t stream = (hipStream_t)stream_;
  PackedLayout L;
  int max_b = 0;
  if (!scales || !y) {
    set_last_error("aqlm_hip_gemv_1x16_packed: null pointer argument");
    return AQLM_HIP_E_INVALID;
  }
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b)) return e;
  const bool fused = packed_fused(desc);
  // On a stream under capture the first kernel of the call waits only for the earlier packed matvecs whose memory it shares
  // (capture_overlap.h); the call's later kernels follow it as issued.  The footprint is everything the call reads or writes.
  CaptureRelax relax(stream);
  if (relax.capturing()) {
    relax.fp.add_rows(x, batch, x_row_stride * 2, (size_t)desc->in_features * 2, false);
    relax.fp.add(packed, L.used, false);
    if (fused && !cells) relax.fp.add((const uint8_t*)packed + L.off_acc, L.off_ent - L.off_acc, true);
    relax.fp.add(codebook, (size_t)65536 * PK_VB, false);
    relax.fp.add(scales, (size_t)L.M * 2, false);
    relax.fp.add(bias, (size_t)L.M * 2, false);
    relax.fp.add_rows(y, batch, y_row_stride * 2, (size_t)L.M * 2, true);
    if (fused && cells) relax.fp.add(cells, (size_t)batch * L.M * 8, true);
    if (!fused) relax.fp.add(workspace, (size_t)PK_S * std::min(batch, max_b) * L.M * sizeof(float), true);
  }  // (packed_launch_main plans the first launch: relax.begin(), or a place in a grouped launch)
  for (int b0 = 0; b0 < batch; b0 += max_b) {  // rows that do not fit one LDS image go in several launches
    const int nb = std::min(max_b, batch - b0);
    uint16_t* yb = (uint16_t*)y + (size_t)b0 * y_row_stride;
    PackedFused fz;  // left empty: partials to the workspace, y by the finalize kernel below (and never a next-layer hint)
    if (fused) {
      fz.cb_absmax = desc->codebook_absmax;
      fz.scales = scales;
      fz.bias = bias;
      fz.y = yb;
      fz.y_row_stride = y_row_stride;
      fz.cells = cells;  // launches of one call are stream-ordered: they share the cells
    }
    if (int e = packed_launch_main(L, packed, codebook, (const uint16_t*)x + (size_t)b0 * x_row_stride, nb, x_row_stride, dtype,
                                   workspace, workspace_bytes, stream, "aqlm_hip_gemv_1x16_packed", fz,
                                   fused && b0 + nb >= batch ? next : PackedNext{}, b0 == 0 ? &relax : nullptr))
      return e;
    if (int e = relax.launched()) return e;
    if (fused) continue;
    if (dtype == AQLM_HIP_F16)
      hipLaunchKernelGGL(gemv_1x16_packed_finalize<F16>, dim3((L.M + 255) / 256), dim3(256), 0, stream, (const float*)workspace,
                         (const uint16_t*)scales, (const uint16_t*)bias, yb, y_row_stride, L.M, nb);
    else
      hipLaunchKernelGGL(gemv_1x16_packed_finalize<BF16>, dim3((L.M + 255) / 256), dim3(256), 0, stream, (const float*)workspace,
                         (const uint16_t*)scales, (const uint16_t*)bias, yb, y_row_stride, L.M, nb);
    if (int e = check_hip(hipGetLastError(), "gemv_1x16_packed_finalize launch")) return e;
  }
  return 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_cells)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                const void* scales, const void* bias, const void* x, void* y, int batch,
                                                long x_row_stride, long y_row_stride, int dtype, void* cells,
                                                size_t cells_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_cells, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, cells, cells_bytes, stream_);
  if (!cells || !desc || !(desc->codebook_absmax > 0.f) || cells_bytes < (size_t)std::min(batch, AQLM_HIP_MAX_GEMV_BATCH) * desc->out_features * 8 ||
      (reinterpret_cast<uintptr_t>(cells) & 7u)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_cells: needs a descriptor with the codebook range and %zu bytes of 8-B aligned, "
                   "zero-filled cells", desc ? (size_t)std::min(batch, AQLM_HIP_MAX_GEMV_BATCH) * desc->out_features * 8 : (size_t)0);
    return AQLM_HIP_E_INVALID;
  }
  if (!tuning().packed_fused_finalize) {
    set_last_error("aqlm_hip_gemv_1x16_packed_cells: the fused finalize is switched off (tuning knob packed_fused_finalize)");
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return gemv_1x16_packed_impl(desc, const_cast<void*>(packed), codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype,
                               nullptr, 0, stream_, PackedNext{}, cells, cells_bytes);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                          const void* scales, const void* bias, const void* x, void* y, int batch,
                                          long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace, workspace_bytes, stream_);
  return gemv_1x16_packed_impl(desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace,
                               workspace_bytes, stream_, PackedNext{});
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_chain)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                                const void* scales, const void* bias, const void* x, void* y, int batch,
                                                long x_row_stride, long y_row_stride, int dtype, void* workspace,
                                                size_t workspace_bytes, const aqlm_hip_packed_desc* next_desc,
                                                const void* next_packed, const void* next_codebook, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_chain, desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace, workspace_bytes, next_desc, next_packed, next_codebook, stream_);
  PackedNext next;
  PackedLayout LN;
  if (next_desc && next_packed && next_codebook) {
    if (!desc_layout(next_desc, LN) || !aligned16(next_packed) || !aligned16(next_codebook)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_chain: invalid descriptor / misaligned buffer of the next layer");
      return AQLM_HIP_E_INVALID;
    }
    const chain_hint::Hint h = packed_chain_hint(LN);  // without a hint the call is the plain entry
    if (h.kept) {
      next.ent = (const uint8_t*)next_packed + h.ent_offset;
      next.codebook = LN.relabel ? (const uint8_t*)next_packed + LN.off_cb : (const uint8_t*)next_codebook;
      next.block_bytes = h.block_bytes;
    }
  }
  return gemv_1x16_packed_impl(desc, packed, codebook, scales, bias, x, y, batch, x_row_stride, y_row_stride, dtype, workspace,
                               workspace_bytes, stream_, next);
}

// What the chain entry does with its hint, read off the rules it runs (packed_chain_hint, packed_chain_waves, packed_fused) and the
// LDS map of the kernel instance its dispatch picks.
extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_chain_plan)(const aqlm_hip_packed_desc* desc, int rows, int dtype,
                                                     const aqlm_hip_packed_desc* next_desc, int* hint_kept, int* prefetch_waves,
                                                     size_t* lds_bytes) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_chain_plan, desc, rows, dtype, next_desc, hint_kept, prefetch_waves, lds_bytes);
  PackedLayout L, LN;
  if (!desc_layout(desc, L) || rows < 1 || rows > AQLM_HIP_MAX_GEMV_BATCH || (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_chain_plan: invalid packed descriptor, rows outside 1..%d or a dtype other than float16 / "
                   "bfloat16", AQLM_HIP_MAX_GEMV_BATCH);
    return AQLM_HIP_E_INVALID;
  }
  if (next_desc && !desc_layout(next_desc, LN)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_chain_plan: invalid descriptor of the next layer");
    return AQLM_HIP_E_INVALID;
  }
  const int max_b = packed_max_batch(L.in_groups, L.RG);
  if (max_b == 0) {
    set_last_error("aqlm_hip_gemv_1x16_packed_chain_plan: layer does not fit the LDS image (in_features %d)", desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int nb = rows - (rows - 1) / max_b * max_b;  // the last launch of the call carries the hint (gemv_1x16_packed_impl)
  // the two-kernel finalize never passes the hint on, and the variable-geometry kernels have no prefetch waves
  const bool kept = next_desc && packed_fused(desc) && !L.G.vg && packed_chain_hint(LN).kept;
  int npw = kept ? packed_chain_waves(L) : 0;
  auto visit = [&](auto kern, auto lds_map) -> int {
    using Map = decltype(lds_map);
    (void)kern;
    if (Map::total(L.in_groups, L.RG, npw, L.NW) > 160 * 1024) npw = 0;  // as the launch decides (packed_launch_main)
    if (lds_bytes) *lds_bytes = Map::total(L.in_groups, L.RG, npw, L.NW);
    return 0;
  };
  const bool sf = nb == 1 && packed_b1_slice_first(L.in_groups, L.RG);
  const bool compact = nb == 1 && packed_b1_compact(L, packed_b1_pd(L));
  int e;
#if AQLM_PK_G == 8
  if (L.G.vg) e = dispatch_packed_vg(dtype, nb, sf, compact, visit);
  else
#endif
    e = dispatch_packed<SingleKernels>(dtype, nb, pick_pd(L), L.EB, sf, compact, visit);
  if (e) return e;
  if (hint_kept) *hint_kept = kept ? 1 : 0;
  if (prefetch_waves) *prefetch_waves = npw;
  return 0;
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_partials)(const aqlm_hip_packed_desc* desc, const void* packed, const void* codebook,
                                                   const void* x, int batch, long x_row_stride, int dtype, void* workspace,
                                                   size_t workspace_bytes, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_partials, desc, packed, codebook, x, batch, x_row_stride, dtype, workspace, workspace_bytes, stream_);
  PackedLayout L;
  int max_b = 0;
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed_partials", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b))
    return e;
  if (batch > max_b) {
    set_last_error("aqlm_hip_gemv_1x16_packed_partials: %d rows do not fit one LDS image (at most %d for in_features %d)", batch,
                   max_b, desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return packed_launch_main(L, packed, codebook, (const uint16_t*)x, batch, x_row_stride, dtype, workspace, workspace_bytes,
                            (hipStream_t)stream_, "aqlm_hip_gemv_1x16_packed_partials");
}

// What packed_launch_main would launch for `rows` rows (ordinary form: no publish, no prefetch waves), read off the kernel
// instance and the LDS map its dispatch picks -- no second copy of the rule.
extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_image)(const aqlm_hip_packed_desc* desc, int rows, int dtype, size_t probe_lds_bytes,
                                                size_t* lds_bytes, uint32_t* x_window, int* blocks_per_cu) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_image, desc, rows, dtype, probe_lds_bytes, lds_bytes, x_window, blocks_per_cu);
  PackedLayout L;
  if (!desc_layout(desc, L) || rows < 1 || rows > AQLM_HIP_MAX_GEMV_BATCH || (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_image: invalid packed descriptor, rows outside 1..%d or a dtype other than float16 / "
                   "bfloat16", AQLM_HIP_MAX_GEMV_BATCH);
    return AQLM_HIP_E_INVALID;
  }
  const int max_b = packed_max_batch(L.in_groups, L.RG);
  if (max_b == 0) {
    set_last_error("aqlm_hip_gemv_1x16_packed_image: layer does not fit the LDS image (in_features %d)", desc->in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int nb = std::min(rows, max_b);
  auto visit = [&](auto kern, auto lds_map) -> int {
    using Map = decltype(lds_map);
    const size_t lds = Map::total(L.in_groups, L.RG, 0, L.NW);
    if (lds_bytes) *lds_bytes = lds;
    if (x_window) *x_window = Map::XFIRST ? Map::SLICE : 0u;
    if (!blocks_per_cu) return 0;
    const size_t ask = probe_lds_bytes ? probe_lds_bytes : lds;
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), ask)) return e;
    return check_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, kern, L.NW * 64, ask),
                     "hipOccupancyMaxActiveBlocksPerMultiprocessor");
  };
  const bool sf = nb == 1 && packed_b1_slice_first(L.in_groups, L.RG);
  const bool compact = nb == 1 && packed_b1_compact(L, packed_b1_pd(L));
#if AQLM_PK_G == 8
  if (L.G.vg) return dispatch_packed_vg(dtype, nb, sf, compact, visit);
#endif
  return dispatch_packed<SingleKernels>(dtype, nb, pick_pd(L), L.EB, sf, compact, visit);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_publish)(const aqlm_hip_packed_desc* desc, void* packed, const void* codebook,
                                                  const void* x, int batch, long x_row_stride, int dtype,
                                                  const aqlm_hip_xgmi* xg, void* pub_own, void* flag_own, void* stream_) {
  PK_G16_FORWARD(desc, gemv_1x16_packed_publish, desc, packed, codebook, x, batch, x_row_stride, dtype, xg, pub_own, flag_own, stream_);
  PackedLayout L;
  int max_b = 0;
  if (int e = packed_check_args("aqlm_hip_gemv_1x16_packed_publish", desc, packed, codebook, x, batch, x_row_stride, dtype, L, max_b))
    return e;
  if (!xg || !xg->epoch || !pub_own || !flag_own || !packed_fused(desc) || batch > max_b ||
      (size_t)batch * desc->out_features > (size_t)xg->max_elems) {
    set_last_error("aqlm_hip_gemv_1x16_packed_publish: needs the one-shot all-reduce state, a descriptor with the codebook range, "
                   "and batch (%d) rows that fit one launch (<= %d) and the state (%d elements)", batch, max_b, xg ? xg->max_elems : 0);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  PackedFused fz;
  fz.cb_absmax = desc->codebook_absmax;
  fz.pub = (float*)pub_own;
  fz.pub_flag = (uint32_t*)flag_own;
  fz.pub_epoch = (uint32_t*)xg->epoch;
  fz.pub_max_elems = (uint32_t)xg->max_elems;
  return packed_launch_main(L, packed, codebook, (const uint16_t*)x, batch, x_row_stride, dtype, nullptr, 0, (hipStream_t)stream_,
                            "aqlm_hip_gemv_1x16_packed_publish", fz);
}

static int gemv_1x16_packed_multi_impl(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                       int num_segments, const void* x, int in_features, int batch, long x_row_stride,
                                       int dtype, void* workspace, size_t workspace_bytes, void* cells, size_t cells_bytes,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!segments || !descs || num_segments < 1 || num_segments > AQLM_HIP_MAX_SEGMENTS || !x) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: 1..%d segments, their descriptors and a non-null x required (got %d)",
                   AQLM_HIP_MAX_SEGMENTS, num_segments);
    return AQLM_HIP_E_INVALID;
  }
  if (dtype != AQLM_HIP_F16 && dtype != AQLM_HIP_BF16) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)",
                   dtype);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = check_x_row_stride("aqlm_hip_gemv_1x16_packed_multi", batch, in_features, x_row_stride)) return e;
  if (batch < 1 || batch > AQLM_HIP_MAX_GEMV_BATCH || !aligned16(x) || (batch > 1 && x_row_stride % 8 != 0)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: batch must be 1..%d with 16-B aligned rows (batch %d)",
                   AQLM_HIP_MAX_GEMV_BATCH, batch);
    return AQLM_HIP_E_INVALID;
  }
  // every segment's layout, once; a null or invalid descriptor is only marked here: the checks below report it in their order
  PackedLayout Ls[AQLM_HIP_MAX_SEGMENTS];
  bool valid[AQLM_HIP_MAX_SEGMENTS], any_vg = false;
  for (int k = 0; k < num_segments; ++k) {
    valid[k] = desc_layout(descs[k], Ls[k]);
    any_vg = any_vg || (valid[k] && Ls[k].G.vg);
  }
  if (any_vg) {  // a variable-geometry segment (format v7) runs on the single-layer kernels only: one launch per segment, same bits
    size_t coff = 0;
    for (int k = 0; k < num_segments; ++k) {
      const aqlm_hip_segment& sg = segments[k];
      if (!descs[k] || descs[k]->in_features != in_features || descs[k]->out_features != sg.out_features) {
        set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: descriptor does not match in_features %d / out_features %d", k,
                       in_features, sg.out_features);
        return AQLM_HIP_E_INVALID;
      }
      const size_t cneed = (size_t)batch * sg.out_features * 8;
      if (cells && coff + cneed > cells_bytes) {
        set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: %zu bytes of cells required, got %zu", coff + cneed, cells_bytes);
        return AQLM_HIP_E_INVALID;
      }
      if (int e = gemv_1x16_packed_impl(descs[k], const_cast<void*>(sg.codes), sg.codebook, sg.scales, sg.bias, x, sg.y, batch, x_row_stride,
                                        sg.y_row_stride, dtype, workspace, workspace_bytes, stream_, PackedNext{},
                                        cells ? (uint8_t*)cells + coff : nullptr, cells ? cneed : 0))
        return e;
      coff += cneed;
    }
    return 0;
  }
  PackedMultiParams mp{};
  PackedFinalizeMultiParams fm{};
  mp.x = (const uint16_t*)x;
  mp.x_row_stride = x_row_stride;
  mp.nseg = fm.nseg = num_segments;
  size_t need = 0;
  int fblocks = 0, max_rg = 0, nw = 0, pd = 4, eb = 0;
  bool fused = true;  // every segment must know its codebook range
  for (int k = 0; k < num_segments; ++k) fused = fused && descs[k] && packed_fused(descs[k]);
  size_t cells_need = 0;
  if (cells) {  // caller-owned accumulator cells: [segment][batch][M] u64
    if (!fused) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: every descriptor must carry the codebook range");
      return AQLM_HIP_E_INVALID;
    }
    for (int k = 0; k < num_segments; ++k) cells_need += (size_t)batch * segments[k].out_features * 8;
    if (cells_bytes < cells_need) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: %zu bytes of cells required, got %zu", cells_need, cells_bytes);
      return AQLM_HIP_E_INVALID;
    }
  }
  size_t cells_off = 0;
  for (int k = 0; k < num_segments; ++k) {
    const aqlm_hip_segment& sg = segments[k];
    if (!sg.codes || !sg.codebook || !sg.scales || !sg.y) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: null pointer in segment %d", k);
      return AQLM_HIP_E_INVALID;
    }
    const PackedLayout& L = Ls[k];
    if (!valid[k] || descs[k]->in_features != in_features || descs[k]->out_features != sg.out_features ||
        !aligned16(sg.codes) || !aligned16(sg.codebook)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: invalid descriptor, or it does not match in_features "
                     "%d / out_features %d", k, in_features, sg.out_features);
      return AQLM_HIP_E_INVALID;
    }
    const uint8_t* base = (const uint8_t*)sg.codes;
    PackedSegment& ps = mp.seg[k];
    ps.ent = (const uint32_t*)(base + L.off_ent);
    ps.winfo = (const uint32_t*)(base + L.off_winfo);
    ps.rowstart = (const uint32_t*)(base + L.off_rowstart);
    if (L.relabel && !(descs[k]->flags & AQLM_HIP_PACKED_HAS_CODEBOOK)) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segment %d: a relabelled buffer needs its codebook image "
                     "(aqlm_hip_packed_set_codebook)", k);
      return AQLM_HIP_E_INVALID;
    }
    ps.codebook = L.relabel ? base + L.off_cb : (const uint8_t*)sg.codebook;
    ps.partial = fused ? nullptr : (float*)((uint8_t*)workspace + need);
    if (fused) {
      ps.acc = cells ? (unsigned long long*)((uint8_t*)cells + cells_off) : (unsigned long long*)(const_cast<uint8_t*>(base) + L.off_acc);
      cells_off += (size_t)batch * sg.out_features * 8;
      ps.scales = (const uint16_t*)sg.scales;
      ps.bias = (const uint16_t*)sg.bias;
      ps.y = (uint16_t*)sg.y;
      ps.y_row_stride = sg.y_row_stride;
      ps.cb_absmax = descs[k]->codebook_absmax;
    }
    ps.M = L.M;
    ps.RG = L.RG;
    ps.NW = L.NW;
    ps.T = L.T;
    ps.XC = L.XC;
    ps.ent_bytes = (uint32_t)L.ent_bytes;
    mp.in_groups = L.in_groups;
    if (eb && eb != L.EB) {
      set_last_error("aqlm_hip_gemv_1x16_packed_multi: segments mix 3- and 4-byte entry formats");
      return AQLM_HIP_E_UNSUPPORTED;
    }
    eb = L.EB;
    max_rg = std::max(max_rg, L.RG);
    nw = std::max(nw, L.NW);
    pd = std::max(pd, pick_pd(L));
    PackedFinalizeSegment& fs = fm.seg[k];
    fs.f.partial = ps.partial;
    fs.f.scales = (const uint16_t*)sg.scales;
    fs.f.bias = (const uint16_t*)sg.bias;
    fs.f.y = (uint16_t*)sg.y;
    fs.f.y_row_stride = sg.y_row_stride;
    fs.f.M = sg.out_features;
    fs.f.B = batch;
    fs.block_begin = fblocks;
    fblocks += (sg.out_features + 255) / 256;
    need += (size_t)PK_S * batch * sg.out_features * sizeof(float);
  }
  if (!fused && (!workspace || workspace_bytes < need)) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: workspace of %zu bytes required, got %zu", need, workspace_bytes);
    return AQLM_HIP_E_INVALID;
  }
  if (packed_max_batch(mp.in_groups, max_rg) < batch) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi: %d rows of %d features do not fit the LDS image", batch, in_features);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  // under capture: the first kernel below is ordered by the memory of all segments (as in gemv_1x16_packed_impl)
  CaptureRelax relax(stream);
  if (relax.capturing()) {
    relax.fp.add_rows(x, batch, x_row_stride * 2, (size_t)in_features * 2, false);
    for (int k = 0; k < num_segments; ++k) {
      const aqlm_hip_segment& sg = segments[k];
      relax.fp.add(sg.codes, Ls[k].used, false);
      if (fused && !cells) relax.fp.add((const uint8_t*)sg.codes + Ls[k].off_acc, Ls[k].off_ent - Ls[k].off_acc, true);
      relax.fp.add(sg.codebook, (size_t)65536 * PK_VB, false);
      relax.fp.add(sg.scales, (size_t)sg.out_features * 2, false);
      relax.fp.add(sg.bias, (size_t)sg.out_features * 2, false);
      relax.fp.add_rows(sg.y, batch, sg.y_row_stride * 2, (size_t)sg.out_features * 2, true);
    }
    if (fused && cells) relax.fp.add(cells, cells_need, true);
    if (!fused) relax.fp.add(workspace, need, true);
    relax.begin();
  }
  // batch 1 with the single-kernel finalize: one workgroup per CU walks all segments, slices double-buffered (pipe kernel)
  if (fused && batch == 1 && tuning().packed_pipe) {
    int prg = 0, nwc = 0, dmaw = 0;
    uint32_t xwin = PP_XWIN;
    bool oneb = false;
    if (pipe_eligible(Ls, num_segments, mp.in_groups, prg, nwc, dmaw, xwin, oneb)) {
      PipeParams pp{};
      pp.x = mp.x;
      pp.in_groups = mp.in_groups;
      pp.nseg = num_segments;
      pp.max_rg = prg;
      pp.nwc = nwc;
      pp.dma_waves = dmaw;
      pp.defer = tuning().packed_pipe == 4 ? 0 : 1;
      for (int k = 0; k < num_segments; ++k) pp.seg[k] = mp.seg[k];
      const size_t lds = pipe_lds(prg, xwin, oneb).total;
      auto go = [&](auto kern) -> int {
        if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
        hipLaunchKernelGGL(kern, dim3(PK_NST), dim3((nwc + dmaw) * 64), lds, stream, pp);
        if (int e = check_hip(hipGetLastError(), "gemv_1x16_packed_pipe launch")) return e;
        return relax.launched();
      };
#define AQLM_PP_GO(SELF, XWV, OB) \
  (dtype == AQLM_HIP_F16 ? go(gemv_1x16_packed_pipe_kernel<F16, SELF, XWV, OB>) : go(gemv_1x16_packed_pipe_kernel<BF16, SELF, XWV, OB>))
      if (xwin == PP_XWIN_SMALL) {
        if (dmaw == 0) return AQLM_PP_GO(true, PP_XWIN_SMALL, false);
        return oneb ? AQLM_PP_GO(false, PP_XWIN_SMALL, true) : AQLM_PP_GO(false, PP_XWIN_SMALL, false);
      }
      if (dmaw == 0) return AQLM_PP_GO(true, PP_XWIN, false);
      return oneb ? AQLM_PP_GO(false, PP_XWIN, true) : AQLM_PP_GO(false, PP_XWIN, false);
#undef AQLM_PP_GO
    }
  }
  auto launch = [&](auto kern, auto lds_map) -> int {
    const size_t lds = decltype(lds_map)::total(mp.in_groups, max_rg);
    if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, dim3(PK_NST * num_segments), dim3(nw * 64), lds, stream, mp);
    if (int e = check_hip(hipGetLastError(), "gemv_1x16_packed_multi launch")) return e;
    return relax.launched();
  };
  if (int e = dispatch_packed<MultiKernels>(dtype, batch, pd, eb, batch == 1 && packed_b1_slice_first(mp.in_groups, max_rg), false, launch)) return e;
  if (fused) return 0;
  if (dtype == AQLM_HIP_F16)
    hipLaunchKernelGGL(gemv_1x16_packed_finalize_multi<F16>, dim3(fblocks), dim3(256), 0, stream, fm);
  else
    hipLaunchKernelGGL(gemv_1x16_packed_finalize_multi<BF16>, dim3(fblocks), dim3(256), 0, stream, fm);
  return check_hip(hipGetLastError(), "gemv_1x16_packed_finalize_multi launch");
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_multi)(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                                int num_segments, const void* x, int in_features, int batch,
                                                long x_row_stride, int dtype, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
  PK_G16_FORWARD(descs && num_segments >= 1 ? descs[0] : nullptr, gemv_1x16_packed_multi, segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, workspace, workspace_bytes, stream_);
  return gemv_1x16_packed_multi_impl(segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, workspace,
                                     workspace_bytes, nullptr, 0, stream_);
}

extern "C" PK_API int PK_ENTRY(gemv_1x16_packed_multi_cells)(const aqlm_hip_segment* segments, const aqlm_hip_packed_desc* const* descs,
                                                      int num_segments, const void* x, int in_features, int batch,
                                                      long x_row_stride, int dtype, void* cells, size_t cells_bytes,
                                                      void* stream_) {
  PK_G16_FORWARD(descs && num_segments >= 1 ? descs[0] : nullptr, gemv_1x16_packed_multi_cells, segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, cells, cells_bytes, stream_);
  if (!cells || (reinterpret_cast<uintptr_t>(cells) & 7u) || !tuning().packed_fused_finalize) {
    set_last_error("aqlm_hip_gemv_1x16_packed_multi_cells: needs 8-B aligned, zero-filled cells and the fused finalize switched on");
    return AQLM_HIP_E_INVALID;
  }
  return gemv_1x16_packed_multi_impl(segments, descs, num_segments, x, in_features, batch, x_row_stride, dtype, nullptr, 0,
                                     cells, cells_bytes, stream_);
}

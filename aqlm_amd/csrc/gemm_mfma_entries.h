// Part of gemm_mfma.hip (read there, last): the workspace size of every op that takes one, the shared-input launch of the X-resident
// K x 8 kernel, and the C entries of the fused K x 8 and 1x16 ops -- argument checks in the order they report, then one launch path
// per route.

namespace aqlm {
size_t gemv_8x8_lut_workspace(int out_features, int in_features, int in_group_size);
}

extern "C" size_t aqlm_hip_workspace_bytes(int op, int batch, int out_features, int in_features) {
  if (op == AQLM_HIP_OP_GEMV_8X8_LUT && batch > 0 && out_features > 0 && in_features > 0 && in_features % batch == 0)
    return aqlm::gemv_8x8_lut_workspace(out_features, in_features, /*in_group_size=*/batch);
  if (batch <= 0 || out_features <= 0 || in_features <= 0) return 0;
  if (op == AQLM_HIP_OP_GEMV_1X16_PACKED || op == AQLM_HIP_OP_GEMV_1X16_G16_PACKED)  // fp32 partials [slices][rows of x][out]
    return (size_t)(op == AQLM_HIP_OP_GEMV_1X16_PACKED ? 16 : 32) * std::min(batch, AQLM_HIP_MAX_GEMV_BATCH) * out_features * sizeof(float);
  if (op == AQLM_HIP_OP_GEMM_KX8_MFMA)  // fp32 partials of the K-split form (64+ rows); 0 below: the op then needs no workspace
    return batch >= 49 ? (size_t)KX_MAX_KSPLIT * std::min(batch, 128) * out_features * sizeof(float) : 0;
  if (op != AQLM_HIP_OP_GEMM_1X16_MFMA) return 0;
  // covers both kernels of the op (the LDS-DMA pipeline and the register-staged one behind the `gemm_variant` knob)
  const GemmPlan g = plan_gemm(batch, out_features, in_features);
  size_t need = (size_t)g.ksplit * out_features * g.Bpad * sizeof(float);
  GldsPlan q;
  if (plan_glds(std::min(batch, 128), out_features, in_features, q) && q.ksplit > 1)
    need = std::max(need, (size_t)q.ksplit * std::min(batch, 128) * out_features * sizeof(float));
  need = std::max(need, scan::workspace_bytes(batch, out_features, in_features));  // the slice-scan kernel's planes (gemm_variant 0 / 4)
  return need;
}

namespace aqlm {
// Shared-input launches of the fused K x 8 op at <= 16 rows (called by aqlm_hip_gemv_kx8_multi; arguments validated there):
// AQLM_HIP_E_UNSUPPORTED when the layers' codebooks + X do not fit the LDS together (the caller launches the layers one by one).
int gemm_kx8_xres_multi(const aqlm_hip_segment* segments, int num_segments, const void* X, int in_features, int K, int batch, long xs,
                        int dtype, hipStream_t stream) {
  if (num_segments < 2 || num_segments > KR_MAX_SEG || !tuning().kx8_xres || (K != 1 && K != 2)) return AQLM_HIP_E_UNSUPPORTED;
  if (!xres_fits(K, batch, in_features, xs, num_segments) || !aligned16(X) || xs % 8 != 0) return AQLM_HIP_E_UNSUPPORTED;
  KrParams<KR_MAX_SEG> p{};
  int tiles = 0;
  for (int k = 0; k < num_segments; ++k) {
    const aqlm_hip_segment& sg = segments[k];
    if (!aligned16(sg.codebook)) return AQLM_HIP_E_UNSUPPORTED;
    p.seg[k] = kr_seg(sg.codes, sg.codebook, sg.scales, sg.bias, sg.y, sg.y_row_stride, sg.out_features, tiles);
    tiles += (sg.out_features + 15) / 16;
  }
  for (int k = num_segments; k < KR_MAX_SEG; ++k) {
    p.seg[k] = p.seg[0];
    p.seg[k].tile0 = 0x7fffffff;  // never reached
  }
  p.X = (const uint16_t*)X;
  p.xs = xs;
  p.B = batch;
  p.in_groups = in_features / 8;
  p.ntiles = tiles;
  p.nseg = num_segments;
  return dispatch_dtype_k(dtype, K, [&](auto t, auto k) { return launch_kx8_xres<decltype(t), decltype(k)::value, KR_MAX_SEG>(p, in_features, stream); });
}
}  // namespace aqlm

extern "C" int aqlm_hip_gemm_kx8_mfma(const void* codes, const void* codebooks, const void* scales, const void* bias, const void* X,
                                      void* Y, int batch, int out_features, int in_features, int num_codebooks, int in_group_size,
                                      long xs, long ys, int dtype, void* stream_) {
  return aqlm_hip_gemm_kx8_mfma_ws(codes, codebooks, scales, bias, X, Y, batch, out_features, in_features, num_codebooks, in_group_size, xs,
                                   ys, dtype, nullptr, 0, stream_);
}

extern "C" int aqlm_hip_gemm_kx8_mfma_ws(const void* codes, const void* codebooks, const void* scales, const void* bias, const void* X,
                                         void* Y, int batch, int out_features, int in_features, int num_codebooks, int in_group_size,
                                         long xs, long ys, int dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "aqlm_hip_gemm_kx8_mfma";
  if (int e = check_not_null(who, codes && codebooks && scales && X && Y)) return e;
  if (int e = check_positive(who, batch, out_features, in_features)) return e;
  if ((num_codebooks != 1 && num_codebooks != 2) || in_group_size != 8) {
    set_last_error("aqlm_hip_gemm_kx8_mfma: 1 or 2 codebooks of 256 x 8 only, got %d codebooks, group %d", num_codebooks, in_group_size);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_x_row_stride(who, batch, in_features, xs)) return e;
  KxPlan probe{};
  if (!plan_kx8(std::min(batch, 128), out_features, in_features, probe) || !aligned16(codebooks) || !aligned16(X) || xs % 8 != 0) {
    set_last_error("aqlm_hip_gemm_kx8_mfma: needs in_features %% 128 == 0, >= 384, and 16-B aligned codebooks / X rows");
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const int ntiles = (out_features + 15) / 16, in_groups = in_features / 8;
  // layers of more tiles than CUs at 7+ rows: the phased form first -- every workgroup holds its 2..4 tiles' accumulators and the K shares
  // meet once (measured, 2x8 g8 4096 -> 11008: 11.5 / 11.9 / 12.2 us at 8 / 12 / 16 rows on the single-phase kernel, 10.3 / 10.8 / 11.0 phased;
  // at 4 rows 9.3 vs 10.1, and with one tile per CU the single-phase kernel is ahead: profiles/r05_gemm_kx8_phase_geometry.log)
  const bool phased_first = (batch >= 7 && ntiles > device_cus() && ntiles <= 4 * device_cus()) || tuning().kx8_phase_tpb != 0;
  auto try_phased = [&]() -> int {  // the X-resident kernel in phases: images that do not fit the LDS at once, 17 .. 32 rows, multi-round layers
    if (!(batch <= (tuning().kx8_xres_phased == 2 ? 16 : 32) && tuning().kx8_xres && tuning().kx8_xres_phased && in_features % 128 == 0 && xs > 0 &&
          xs < (1l << 21)))
      return AQLM_HIP_E_UNSUPPORTED;
    KpParams kp{};
    kp.codes = (const uint8_t*)codes;
    kp.codebooks = (const uint8_t*)codebooks;
    kp.X = (const uint16_t*)X;
    kp.scales = (const uint16_t*)scales;
    kp.bias = (const uint16_t*)bias;
    kp.Y = (uint16_t*)Y;
    kp.xs = xs;
    kp.ys = ys;
    kp.M = out_features;
    kp.B = batch;
    kp.in_groups = in_groups;
    kp.ntiles = ntiles;
    return dispatch_dtype_k(dtype, num_codebooks, [&](auto t, auto k) { return launch_kx8_xres_phased<decltype(t), decltype(k)::value>(kp, in_features, stream); });
  };
  if (phased_first) {
    const int e = try_phased();
    if (e != AQLM_HIP_E_UNSUPPORTED) return e;
  }
  if (batch <= 16 && tuning().kx8_xres && xres_fits(num_codebooks, batch, in_features, xs)) {
    // <= 16 rows: X resident in LDS, no per-step synchronisation (round 5)
    KrParams<1> kr{};
    kr.seg[0] = kr_seg(codes, codebooks, scales, bias, Y, ys, out_features, 0);
    kr.X = (const uint16_t*)X;
    kr.xs = xs;
    kr.B = batch;
    kr.in_groups = in_groups;
    kr.ntiles = ntiles;
    kr.nseg = 1;
    return dispatch_dtype_k(dtype, num_codebooks, [&](auto t, auto k) { return launch_kx8_xres<decltype(t), decltype(k)::value, 1>(kr, in_features, stream); });
  }
  if (!phased_first) {
    const int e = try_phased();
    if (e != AQLM_HIP_E_UNSUPPORTED) return e;
  }
  // fp32 partials of the K-split form: [<= KX_MAX_KSPLIT][rows of the slab][out_features]; a workspace too small for a slab's plan
  // simply keeps that slab on the no-split form
  auto can_split = [&](int nb) {
    return workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 &&
           workspace_bytes >= (size_t)KX_MAX_KSPLIT * nb * out_features * sizeof(float);
  };
  for (int b0 = 0; b0 < batch; b0 += 128) {  // every slab is planned before anything is launched (a tail slab plans differently from the probe)
    KxPlan r{};
    if (!plan_kx8(std::min(128, batch - b0), out_features, in_features, r, can_split(std::min(128, batch - b0)))) {
      set_last_error("aqlm_hip_gemm_kx8_mfma: a slab of %d rows at in_features %d is outside the kernel's plans", std::min(128, batch - b0), in_features);
      return AQLM_HIP_E_UNSUPPORTED;
    }
  }
  KxParams kp{};
  kp.codes = (const uint8_t*)codes;
  kp.codebooks = (const uint8_t*)codebooks;
  kp.scales = (const uint16_t*)scales;
  kp.bias = (const uint16_t*)bias;
  kp.xs = xs;
  kp.ys = ys;
  kp.M = out_features;
  kp.in_groups = in_groups;
  kp.partial = (float*)workspace;
  for (int b0 = 0; b0 < batch; b0 += 128) {  // slabs of 128 rows (the codes are re-read per slab: they are 2 bits per weight)
    const int nb = std::min(128, batch - b0);
    KxPlan r{};
    plan_kx8(nb, out_features, in_features, r, can_split(nb));
    kp.X = (const uint16_t*)X + (long)b0 * xs;
    kp.Y = (uint16_t*)Y + (long)b0 * ys;
    kp.B = nb;
    kp.nsteps = r.nsteps;
    kp.ksplit = r.ksplit;
    kp.row_blocks = (out_features + 16 * r.rt - 1) / (16 * r.rt);
    if (int e = dispatch_dtype_k(dtype, num_codebooks, [&](auto t, auto k) { return launch_kx8<decltype(t), decltype(k)::value>(kp, r, stream); })) return e;
    if (r.ksplit > 1)  // the slices meet: sum in slice order, scale, bias, one rounding (the 1x16 pipeline's finalize kernel)
      if (int e = launch_glds_finalize(dtype, workspace, scales, bias, kp.Y, ys, out_features, nb, r.ksplit, stream, "gemm_kx8 finalize launch")) return e;
  }
  return 0;
}

extern "C" int aqlm_hip_gemm_1x16_mfma(const void* codes, const void* codebook, const void* scales, const void* bias,
                                       const void* X, void* Y, int batch, int out_features, int in_features,
                                       int in_group_size, long xs, long ys, int dtype, void* workspace,
                                       size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "aqlm_hip_gemm_1x16_mfma";
  if (int e = check_not_null(who, codes && codebook && scales && X && Y)) return e;
  if (int e = check_positive(who, batch, out_features, in_features)) return e;
  if (int e = check_group_size(who, in_group_size)) return e;
  if (int e = check_dtype(who, dtype)) return e;
  if (int e = check_x_row_stride(who, batch, in_features, xs)) return e;
  if (in_features % BK != 0 || !aligned16(codes) || !aligned16(codebook) || !aligned16(X) || xs % 8 != 0) {
    set_last_error("aqlm_hip_gemm_1x16_mfma: needs in_features %% 64 == 0 and 16-B aligned codes/codebook/X rows");
    return AQLM_HIP_E_UNSUPPORTED;
  }
  const size_t need = aqlm_hip_workspace_bytes(AQLM_HIP_OP_GEMM_1X16_MFMA, batch, out_features, in_features);
  if (!workspace || workspace_bytes < need) {
    set_last_error("aqlm_hip_gemm_1x16_mfma: workspace of %zu bytes required, got %zu", need, workspace_bytes);
    return AQLM_HIP_E_INVALID;
  }
  // gemm_variant: 0 = the slice-scan kernel (gemm_1x16_scan.hip, round 6: codebook slices in LDS, no L2 gathers) up to scan_max_rows
  // where it applies, else round 5's routing (5): 16-row blocks where they pay, else the K-split pipeline; 1 = register-staged kernel of
  // round 1, 2 = 16-row blocks wherever they apply, 3 = K-split pipeline only, 4 = slice-scan kernel at any row count
  int variant = tuning().gemm_variant;
  if ((variant == 4 || (variant == 0 && batch <= tuning().scan_max_rows)) && in_group_size == 8 &&
      scan::workspace_bytes(batch, out_features, in_features) != 0 && aligned16(workspace)) {
    return scan::run(codes, codebook, scales, bias, X, Y, batch, out_features, in_features, xs, ys, dtype, workspace, stream);
  }
  if (variant == 4 || variant == 5) variant = 0;
  const bool use_glds = variant != 1;
  const int in_groups = in_features / in_group_size;
  // what a slab does not change, per route: the 16-row kernel, the K-split pipeline, the register-staged kernel and its finalize
  R16Params rp{};
  rp.codes = (const uint8_t*)codes;
  rp.codebook = (const uint8_t*)codebook;
  rp.scales = (const uint16_t*)scales;
  rp.bias = (const uint16_t*)bias;
  rp.xs = xs;
  rp.ys = ys;
  rp.M = out_features;
  rp.in_groups = in_groups;
  GldsParams gp{};
  gp.codes = (const uint8_t*)codes;
  gp.codebook = (const uint8_t*)codebook;
  gp.partial = (float*)workspace;
  gp.scales = (const uint16_t*)scales;
  gp.bias = (const uint16_t*)bias;
  gp.xs = xs;
  gp.ys = ys;
  gp.M = out_features;
  gp.in_groups = in_groups;
  gp.store_nt = tuning().gemm_store_nt;
  gp.dbg = tuning().gemm_debug;
  GemmParams p{};
  p.codes = (const uint8_t*)codes;
  p.codebook = (const uint8_t*)codebook;
  p.partial = (float*)workspace;
  p.M = out_features;
  p.K = in_features;
  p.in_groups = in_groups;
  p.xs = xs;
  p.cb_bytes = 65536 * in_group_size * 2;
  FinalizeParams f{};
  f.partial = (const float*)workspace;
  f.scales = (const uint16_t*)scales;
  f.bias = (const uint16_t*)bias;
  f.M = out_features;
  f.ys = ys;
  // batch > 128 is processed in slabs of 128 columns (codes re-gathered per slab)
  for (int b0 = 0; b0 < batch; b0 += 128) {
    const int nb = std::min(128, batch - b0);
    const uint16_t* Xs = (const uint16_t*)X + (long)b0 * xs;
    uint16_t* Ys = (uint16_t*)Y + (long)b0 * ys;
    R16Plan r16{};
    const bool r16_pays = nb <= R16_ROWS_ANY || (nb <= R16_ROWS_SMALL && (long)out_features * in_features <= R16_SMALL_LAYER);
    if ((variant == 2 || (variant == 0 && r16_pays)) && plan_rows16(nb, in_features, in_group_size, r16)) {
      rp.X = Xs;
      rp.Y = Ys;
      rp.B = nb;
      rp.nsteps = r16.nsteps;
      if (int e = dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) { return launch_rows16<decltype(t), decltype(g)::value>(rp, r16, stream); })) return e;
      continue;
    }
    GldsPlan q;
    if (use_glds && plan_glds(nb, out_features, in_features, q)) {
      gp.X = Xs;
      gp.Y = Ys;
      gp.B = nb;
      gp.row_blocks = q.row_blocks;
      gp.ksplit = q.ksplit;
      gp.chunks_base = q.chunks_base;
      gp.chunks_rem = q.chunks_rem;
      if (int e = dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto g) { return launch_glds<decltype(t), decltype(g)::value>(gp, q, stream); })) return e;
      if (q.ksplit > 1)
        if (int e = launch_glds_finalize(dtype, workspace, scales, bias, Ys, ys, out_features, nb, q.ksplit, stream, "gemm_glds_finalize launch")) return e;
      continue;
    }
    // The register-staged kernel forms a row's X offset in 32 bits behind a bounds-checked descriptor of x_bytes.  A slab whose extent
    // ((rows - 1) * xs + in_features) * 2 passes 2^32 (xs above ~2^24 at 128 rows) is cut into sub-slabs whose extent fits, down to
    // single rows, X and Y rebased per sub-slab.  The extent stays <= 0xfffffff0: the kernel reads zeros for k past its slice at
    // offset 0xfffffff0, which the descriptor range-checks dword by dword, so a larger extent would let those loads see memory.
    // The K split is the plan's whatever the rows (plan_gemm takes it from M and K), so a row's bits do not depend on the cut; at
    // ordinary strides there is one sub-slab and the launch is what it always was.
    const long sub_max = xs > 0 ? std::max<long>(1, ((0xfffffff0L / 2 - in_features) / xs) + 1) : nb;
    for (int s0 = 0; s0 < nb; s0 += (int)std::min<long>(sub_max, nb)) {
      const int ns = (int)std::min<long>(sub_max, nb - s0);
      const GemmPlan g = plan_gemm(ns, out_features, in_features);
      p.X = Xs + (long)s0 * xs;
      p.B = ns;
      p.Bpad = g.Bpad;
      p.kslice = g.kslice;
      p.ksplit = g.ksplit;
      p.x_bytes = (uint32_t)std::min<long>(((long)(ns - 1) * xs + in_features) * 2, 0xffffffffL);
      if (int e = dispatch_dtype_group(dtype, in_group_size, [&](auto t, auto gs) { return launch_gemm<decltype(t), decltype(gs)::value>(p, g.nbt, stream); })) return e;
      f.Y = Ys + (long)s0 * ys;
      f.B = ns;
      f.Bpad = g.Bpad;
      f.ksplit = g.ksplit;
      dim3 grid((out_features + 31) / 32, g.nbt);
      if (dtype == AQLM_HIP_F16) hipLaunchKernelGGL(gemm_finalize_kernel<F16>, grid, dim3(256), 0, stream, f);
      else hipLaunchKernelGGL(gemm_finalize_kernel<BF16>, grid, dim3(256), 0, stream, f);
      if (int e2 = check_hip(hipGetLastError(), "gemm_finalize launch")) return e2;
    }
  }
  return 0;
}

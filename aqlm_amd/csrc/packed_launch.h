// Part of gemv_packed.hip (inside namespace aqlm::PK_NS), host only: ring depth (pick_pd), the (dtype, batch, ring depth, entry bytes)
// dispatch over the kernel instantiations (dispatch_packed and its *Kernels selectors) and the LDS budget (packed_lds_need,
// packed_max_batch, packed_b1_slice_first).  Needs PackedLayout (packed_format.h) and the matvec kernels and PackedLds
// of packed_gemv_kernels.h.

static int pick_pd(const PackedLayout& L) {
  const int t = tuning().packed_prefetch;
  if (t == 3 || t == 4 || t == 8) return t;
  // measured (profiles/r02_mb_packed_variants.log): 3 steps in flight per wave are best or within 1 % of best on every
  // shape; 8 are 5-10 % slower (the bigger burst of the prologue delays the codebook slice, which gates the loop)
  return 3;
}

// Instantiations: (dtype, B, PD, entry bytes).  Only the batch-1 kernels come with the deeper ring (PD = 8): with more
// rows the loop is LDS-bound and 4 steps in flight cover the stream.
// slice_first: the one-row image with the slice in front (no 64 KiB x window): for layers whose row tables do not fit
// behind the window (packed_b1_slice_first).
// compact: the one-row image with the compact x window (packed_b1_compact; ring depth 3, 4-byte entries, and only the
// selectors that carry such instances: KP::COMPACT).
template <class KP, class Launch>
static int dispatch_packed(int dtype, int batch, int pd, int eb, bool slice_first, bool compact, Launch&& launch) {
#define AQLM_PK_GO(TT, BB, PP, EE) launch(KP::template get<TT, BB, PP, EE, PK_XWIN_FULL>(), PackedLds<BB, PK_XWIN_FULL>{})
#define AQLM_PK_GO0(TT, PP, EE) launch(KP::template get<TT, 1, PP, EE, 0u>(), PackedLds<1, 0u>{})
#define AQLM_PK_GOC(TT) launch(KP::template get<TT, 1, 3, 4, PK_XWIN_COMPACT>(), PackedLds<1, PK_XWIN_COMPACT>{})
#define AQLM_PK_CASE(BB)                                                                                      \
  case BB:                                                                                                    \
    if (dtype == AQLM_HIP_F16) return eb == 3 ? AQLM_PK_GO(F16, BB, 4, 3) : AQLM_PK_GO(F16, BB, 4, 4);          \
    return eb == 3 ? AQLM_PK_GO(BF16, BB, 4, 3) : AQLM_PK_GO(BF16, BB, 4, 4);
  switch (batch) {
    case 1:
#define AQLM_PK_B1(TT, EE) (pd == 8 ? AQLM_PK_GO(TT, 1, 8, EE) : (pd == 4 ? AQLM_PK_GO(TT, 1, 4, EE) : AQLM_PK_GO(TT, 1, 3, EE)))
      if (slice_first) {  // (ring depth 3, the default, only)
        if (dtype == AQLM_HIP_F16) return eb == 3 ? AQLM_PK_GO0(F16, 3, 3) : AQLM_PK_GO0(F16, 3, 4);
        return eb == 3 ? AQLM_PK_GO0(BF16, 3, 3) : AQLM_PK_GO0(BF16, 3, 4);
      }
      if constexpr (KP::COMPACT) {
        if (compact && pd == 3 && eb == 4) return dtype == AQLM_HIP_F16 ? AQLM_PK_GOC(F16) : AQLM_PK_GOC(BF16);
      }
      if (dtype == AQLM_HIP_F16) return eb == 3 ? AQLM_PK_B1(F16, 3) : AQLM_PK_B1(F16, 4);
      return eb == 3 ? AQLM_PK_B1(BF16, 3) : AQLM_PK_B1(BF16, 4);
#undef AQLM_PK_B1
    AQLM_PK_CASE(2)
    AQLM_PK_CASE(3)
    AQLM_PK_CASE(4)
    AQLM_PK_CASE(5)
    AQLM_PK_CASE(6)
    AQLM_PK_CASE(7)
    AQLM_PK_CASE(8)
  }
#undef AQLM_PK_CASE
#undef AQLM_PK_GO
#undef AQLM_PK_GO0
#undef AQLM_PK_GOC
  return AQLM_HIP_E_INVALID;
}

#if AQLM_PK_G == 8
// ... and over the variable-geometry kernels (4-byte entries; ring depth 3 at one row, 4 above; no chain prefetch, no publish)
template <class Launch>
static int dispatch_packed_vg(int dtype, int batch, bool slice_first, bool compact, Launch&& launch) {
#define AQLM_PK_VG(TT, BB, PP, XW) launch(gemv_1x16_packed_vg_kernel<TT, BB, PP, XW>, PackedLds<BB, XW>{})
#define AQLM_PK_VG_CASE(BB) \
  case BB:                  \
    return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, BB, 4, PK_XWIN_FULL) : AQLM_PK_VG(BF16, BB, 4, PK_XWIN_FULL);
  switch (batch) {
    case 1:
      if (slice_first) return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, 1, 3, 0u) : AQLM_PK_VG(BF16, 1, 3, 0u);
      if (compact) return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, 1, 3, PK_XWIN_COMPACT) : AQLM_PK_VG(BF16, 1, 3, PK_XWIN_COMPACT);
      return dtype == AQLM_HIP_F16 ? AQLM_PK_VG(F16, 1, 3, PK_XWIN_FULL) : AQLM_PK_VG(BF16, 1, 3, PK_XWIN_FULL);
    AQLM_PK_VG_CASE(2)
    AQLM_PK_VG_CASE(3)
    AQLM_PK_VG_CASE(4)
    AQLM_PK_VG_CASE(5)
    AQLM_PK_VG_CASE(6)
    AQLM_PK_VG_CASE(7)
    AQLM_PK_VG_CASE(8)
  }
#undef AQLM_PK_VG_CASE
#undef AQLM_PK_VG
  return AQLM_HIP_E_INVALID;
}
#endif

struct SingleKernels {
  static constexpr bool COMPACT = AQLM_PK_XFIRST && PK_G == 8;  // the decode path's instances; the 16-element build keeps the full window
  template <class T_, int B, int PD, int EB, uint32_t XW>
  static auto get() { return gemv_1x16_packed_kernel<T_, B, PD, XW, EB>; }
};
struct PublishKernels {  // row-parallel shards (aqlm_hip_gemv_1x16_packed_publish)
  static constexpr bool COMPACT = false;
  template <class T_, int B, int PD, int EB, uint32_t XW>
  static auto get() { return gemv_1x16_packed_kernel<T_, B, PD, XW, EB, true>; }
};
struct MultiKernels {
  static constexpr bool COMPACT = false;
  template <class T_, int B, int PD, int EB, uint32_t XW>
  static auto get() { return gemv_1x16_packed_multi_kernel<T_, B, PD, XW, EB>; }
};

// largest batch whose LDS image fits the CU
template <int BB>
static size_t packed_lds_total(int in_groups, int RG) { return PackedLds<BB, PK_XWIN_FULL>::total(in_groups, RG); }
// one row: x first (a 64 KiB window, both reads without an address add) where that fits, else slice first
static bool packed_b1_slice_first(int in_groups, int RG) { return packed_lds_total<1>(in_groups, RG) > 160 * 1024; }
static int packed_b1_pd(const PackedLayout& L) { return L.G.vg ? 3 : pick_pd(L); }  // ring depth of the one-row launch (variable geometry: always 3)
// ... and of the x-first layers those whose x image (all its copies) fits the compact window take it: the image then leaves
// room on the CU for a workgroup of another layer (tuning key packed_compact_window: 1 = always the full window).
// Ring depth 3 and 4-byte entries only -- the decode path; everything else has no compact instance.
static bool packed_b1_compact(const PackedLayout& L, int pd) {
  return SingleKernels::COMPACT && tuning().packed_compact_window != 1 && pd == 3 && L.EB == 4 &&
         !packed_b1_slice_first(L.in_groups, L.RG) && pk_x_image_bytes(L.in_groups, L.XC) <= PK_XWIN_COMPACT;
}
static size_t packed_lds_need(int b, int in_groups, int RG) {
  switch (b) {
    case 1: return std::min(packed_lds_total<1>(in_groups, RG), PackedLds<1, 0u>::total(in_groups, RG));
    case 2: return packed_lds_total<2>(in_groups, RG);
    case 3: return packed_lds_total<3>(in_groups, RG);
    case 4: return packed_lds_total<4>(in_groups, RG);
    case 5: return packed_lds_total<5>(in_groups, RG);
    case 6: return packed_lds_total<6>(in_groups, RG);
    case 7: return packed_lds_total<7>(in_groups, RG);
    default: return packed_lds_total<8>(in_groups, RG);
  }
}
static int packed_max_batch(int in_groups, int RG) {
  // (the single-row image is not always the smallest: x first keeps a 64 KiB window in front of the slice)
  if (packed_lds_need(1, in_groups, RG) > 160 * 1024) return 0;
  int b = AQLM_HIP_MAX_GEMV_BATCH;
  while (b > 1 && packed_lds_need(b, in_groups, RG) > 160 * 1024) --b;
  return packed_lds_need(b, in_groups, RG) <= 160 * 1024 ? b : 0;
}

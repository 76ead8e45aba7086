// Shared device/host helpers for the gfx950 AQLM kernels.  wave64 everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/aqlm_hip.h"
#include "capture_overlap.h"
#include "group_fold.h"

namespace aqlm {

constexpr int WAVE = 64;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// buffer cache-policy bits of gfx940+ raw buffer loads (cdna_hip_programming.md T8 / G16)
constexpr int AUX_DEFAULT = 0;
constexpr int AUX_SC0 = 1;
constexpr int AUX_NT = 2;
constexpr int AUX_SC1 = 16;

// ---------------------------------------------------------------------------------------------
// element-type traits: fp16 and bf16 share every kernel; arithmetic is v_dot2c_f32_{f16,bf16}
// with fp32 accumulation (the reference CUDA kernels accumulate each group in half precision,
// cuda_kernel.cu:69-75; we do not reproduce that rounding).
// ---------------------------------------------------------------------------------------------
struct F16 {
  static constexpr int id = AQLM_HIP_F16;
  static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c, false);
  }
  static __device__ __forceinline__ float to_float(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
  static __device__ __forceinline__ uint16_t from_float(float f) {
    return __builtin_bit_cast(uint16_t, (_Float16)f);  // v_cvt_f16_f32, round-to-nearest-even
  }
  // packed add of two f16 pairs (used by dequant to sum codebooks like embedding_bag does in storage dtype)
  static __device__ __forceinline__ float lo(uint32_t a) { return to_float((uint16_t)(a & 0xffffu)); }
  static __device__ __forceinline__ float hi(uint32_t a) { return to_float((uint16_t)(a >> 16)); }
};

struct BF16 {
  static constexpr int id = AQLM_HIP_BF16;
  static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
  }
  static __device__ __forceinline__ float to_float(uint16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
  static __device__ __forceinline__ uint16_t from_float(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                               // round-to-nearest-even
    return (uint16_t)(u >> 16);
  }
  static __device__ __forceinline__ float lo(uint32_t a) { return __uint_as_float(a << 16); }
  static __device__ __forceinline__ float hi(uint32_t a) { return __uint_as_float(a & 0xffff0000u); }
};

// <8 halfs, 8 halfs> accumulated into fp32
template <class T>
__device__ __forceinline__ float dot8(const u32x4& w, const u32x4& x, float acc) {
  acc = T::dot2(w.x, x.x, acc);
  acc = T::dot2(w.y, x.y, acc);
  acc = T::dot2(w.z, x.z, acc);
  acc = T::dot2(w.w, x.w, acc);
  return acc;
}

// Reductions on the VALU (DPP): __shfl_xor compiles to ds_bpermute_b32, i.e. every step of a shuffle tree is an LDS
// instruction with LDS latency -- in the gather kernels that is 4-6 extra LDS round trips per output row on the unit
// that is already the bottleneck.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15); every lane of the row receives the total
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f32<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f32<0x141>(v);  // row_half_mirror: the other quad of each group of 8
  v += dpp_f32<0x140>(v);  // row_mirror: the other half of the row
  return v;
}

// sum over aligned groups of 4 lanes; every lane of the group receives the total
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  return v;
}

// sum over aligned groups of 8 lanes; every lane of the group receives the total
__device__ __forceinline__ float oct_sum(float v) {
  v = quad_sum(v);
  v += dpp_f32<0x141>(v);  // row_half_mirror
  return v;
}

// sum over the wave; every lane receives the total
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

// maximum over the wave of an unsigned value (DPP within the rows, scalar across them); wave-uniform result
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  uint32_t o;
  o = dpp_u32<0xB1>(v);  v = o > v ? o : v;
  o = dpp_u32<0x4E>(v);  v = o > v ? o : v;
  o = dpp_u32<0x141>(v); v = o > v ? o : v;
  o = dpp_u32<0x140>(v); v = o > v ? o : v;
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  const uint32_t a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
  return a > b ? a : b;
}

// compile-time extraction of code #idx from the dwords of one code word
template <int CODE_BYTES, int N>
__device__ __forceinline__ uint32_t code_at(const uint32_t (&cw)[N], int idx) {
  if constexpr (CODE_BYTES == 2) {
    return (cw[idx >> 1] >> ((idx & 1) * 16)) & 0xffffu;
  } else {
    return (cw[idx >> 2] >> ((idx & 3) * 8)) & 0xffu;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
void set_last_error(const char* fmt, ...);
int check_hip(hipError_t e, const char* what);
// Raise a kernel's dynamic-LDS limit (needed above the 64 KiB default) once per (kernel, device): a process may drive
// several GPUs (device_map="auto"), and the attribute is per device.  Returns 0 or an error code.
int ensure_dynamic_lds(const void* kernel, size_t bytes);

struct Tuning {
  int gemv_rows_per_wave = 0;    // 0 = heuristic
  int gemv1x16_aux = AUX_DEFAULT;  // cache policy of the codebook gathers: 0 default, 1 sc0, 2 nt, 16 sc1
  int gemv1x16_prefetch_cb = 0;  // 1: each block touches a slice of the codebook first (warms its XCD's L2)
  int kx8_replicas = 1;          // K x 8 g8 batch-1: 1 = replicated-LDS kernel for >= 4096 rows, 0 = never, 2 = always
  int gemm_variant = 0;          // large-batch 1x16 op: 0 = slice-scan kernel (round 6) up to scan_max_rows (default 0: never) where it applies (g 8, in_features % 256 == 0), else as 5; 1 = register-staged split-K kernel (round 1), 2 = 16-row L2-gather kernel wherever it applies, 3 = K-split L2-gather pipeline only, 4 = slice-scan kernel at any row count, 5 = round 5's routing (16-row kernel <= 64 rows, pipeline above)
  int scan_max_rows = 0;         // rows up to which variant 0 takes the slice-scan kernel (0: never -- measured slower than round 5's routes, gemm_1x16_scan.hip)
  int scan_prefetch = 4;         // slice-scan kernel: tiles of code words in flight per wave (2 / 4)
  int kx8_xres = 1;              // fused K x 8 MFMA op at <= 16 rows: 1 = X resident in LDS (round 5), 0 = the streaming 16-row kernel (A/B runs)
  int kx8_xres_phased = 1;       // ... whose X image does not fit the LDS at once: 1 = the X-resident kernel in phases (round 5; also 17 .. 32 rows), 2 = up to 16 rows only, 0 = the streaming 16-row kernel
  int kx8_phase_tpb = 0;         // experiments: 1..3 = every <= 32-row call on the phased kernel with this many tiles per workgroup (0 = off)
  int kx8_phase_quads = 0;       // experiments: cap on the quads per phase (smaller image -> more workgroups per CU)
  int kx8_mfma_min_rows = 2;     // rows from which aqlm_hip_gemv_kx8[_multi] hands 1x8 / 2x8 g8 calls to the fused MFMA kernel (0 = never; 3 in round 4, 2 since the X-resident kernel)
  int kx8_multi_xres_min_rows = 2;  // shared-input launches of 1x8 / 2x8 g8: rows from which all layers run in ONE launch of the X-resident MFMA kernel (0 = never; 1 = batch 1 too)
  int kx8_ksplit = 0;            // fused K x 8 MFMA op with a workspace at >= 49 rows: 0 = K slices by the plan (<= 4), 1 = never split, 2 / 4 = force
  int kx8_rt = 0;                // ... 16-row tiles per block: 0 = by the plan, 1 / 2 = force (A/B runs)
  int gemm_debug = 0;            // LDS-DMA pipeline: knock-out switches for timing experiments (never set in production: results are wrong)
  int gemm_store_nt = 0;         // LDS-DMA pipeline: fp32 partials stored with the non-temporal hint
  int force_generic = 0;         // 1: route every gemv through the generic kernel (testing)
  int packed_fused_finalize = 1;  // 0 = two-kernel finalize even when the descriptor carries the codebook range (A/B runs)
  int packed_waves = 0;          // prepack: waves per workgroup of the packed 1x16 kernel (4 / 8 / 16); 0 = heuristic
  int packed_arrange = 1;        // prepack: bank-aware order of the entries: 1 = greedy deal + local search for layers of <= 8 Mi codes, greedy deal alone above; 3 = local search always; 2 = greedy deal only; 0 = ascending j
  int packed_xcopies = 0;        // prepack: rotated copies of x the batch-1 kernel keeps in LDS (1..4, capped by what fits); 0 = 1
  int packed_entry_bytes = 0;    // prepack: 0 / 4 = 32-bit entries; 3 = 24-bit entries (wave ranges of <= 32 steps)
  int packed_debug = 0;          // profiling builds (-DAQLM_PACKED_TRACE) only: 1 = no LDS reads / dots, 2 = no entry stream
  int packed_prefetch = 0;       // packed 1x16 kernel: steps of the entry stream in flight per wave (4 / 8); 0 = heuristic
  int packed_pipe = 1;           // shared-input launches of batch 1: 1 = one workgroup per CU walks the segments with double-buffered slices
  int packed_fill_rotate = 1;    // packed 1x16 kernel: 1 = the workgroups that share a codebook slice start their LDS fill at different pieces
  int packed_compact_window = 0; // packed 1x16 kernel, one-row launches whose x fits 8208 bytes (<= 4096 features): 0 = the compact x window (two layers' workgroups share a CU), 1 = always the 64 KiB window (A/B runs)
  int lut_waves = 0;             // 8 x 8 look-up-table matvec: waves per workgroup (8 / 16); 0 = default
  int packed_prefetch_waves = 0; // chain prefetch: extra waves per workgroup that pull the next layer towards L2 (0 = 2, -1 = off)
  int packed_capture_window = capture_overlap::kDefaultWindow;  // packed 1x16 matvecs captured into a graph: consecutive launches that share no memory and may run side by side (1..8; capture_overlap.h); 1 = every launch after the previous one
  int packed_capture_min_run = capture_overlap::kDefaultMinRun;  // ... launches an uninterrupted run of them must hold before any is relaxed (a graph with branches costs host time per node: capture_overlap.h); 1 = from the second launch on
  int packed_capture_merge = capture_overlap::kDefaultMerge;  // ... launches of one kernel instance that may share a graph node, run by the grouped kernel (1..8; capture_overlap.h, "Grouped launches"); 1 = every launch a node of its own
  int packed_capture_head = 1;   // ... once a run holds packed_capture_min_run launches, its first launches -- a chain of single launches until then -- are regrouped in place into grouped / folded nodes (capture_overlap.h, "Regrouping the head"): 1 = on, 0 = they stay single launches
  int packed_group_fold = 0;     // ... workgroups of such a node that keep their codebook slice and x in LDS and walk F row groups of their (layer, slice) in turn (group_fold.h): 0 = default (4), 1 = off, 2, 4; a node of fewer than F launches is not folded
  int packed_dequant_by_xcd = 1; // aqlm_hip_dequant_1x16_packed, grid order: 1 = by the measured rule (16-B vectors: the streams that run together on an XCD are the slices of one row group, so their partial-line stores meet in one L2; 32-B vectors: stream-major like the unpack kernel), 0 = always stream-major, 2 = always by XCD (A/B runs)
};
Tuning& tuning();

// What a captured packed matvec leaves with the planner (the payload of capture_overlap.h): enough to build the graph node of
// any group it is a member of, also inside a call of another kernel instance -- the call that regroups a run's head may have
// the other shape.  A node of one member launches `func` as the member's own call did; a node of several launches the grouped
// form of their kernel instance (`group_func`; its only argument is their segments, kMaxMerge of `seg_bytes` each) or, by
// group_fold::choose and while no member has more rows per group than the block has threads, the folded form (`fold_func`,
// null: none; second argument the fold factor).
struct CaptureMember {
  static constexpr unsigned kMaxArgs = 12, kArgBytes = 320, kSegBytes = 256;
  const void* func;  // the launch as issued: kernel, geometry, arguments
  unsigned grid, threads, lds, nargs;
  uint16_t arg_off[kMaxArgs];  // into args
  const void* group_func;  // null: the launch shares no node
  const void* fold_func;
  unsigned seg_bytes;
  int rows_per_group;
  alignas(8) unsigned char args[kArgBytes];
  alignas(8) unsigned char seg[kSegBytes];
};
// the launch half: parameter types from the kernel's own signature, values converted as a launch converts them
template <class... P, class... A>
inline bool capture_member_launch(CaptureMember& m, void (*kern)(P...), unsigned grid, unsigned threads, size_t lds, const A&... a) {
  static_assert(sizeof...(P) == sizeof...(A) && sizeof...(P) <= CaptureMember::kMaxArgs, "one value per kernel parameter");
  m.func = reinterpret_cast<const void*>(kern);
  m.grid = grid;
  m.threads = threads;
  m.lds = (unsigned)lds;
  m.nargs = 0;
  size_t at = 0;
  bool fits = true;
  auto put = [&](const auto& v) {
    static_assert(alignof(decltype(v)) <= 8, "arguments are packed at 8-byte boundaries");
    at = (at + 7) & ~(size_t)7;
    if (at + sizeof v > CaptureMember::kArgBytes) {
      fits = false;
      return;
    }
    memcpy(m.args + at, &v, sizeof v);
    m.arg_off[m.nargs++] = (uint16_t)at;
    at += sizeof v;
  };
  (put(static_cast<std::remove_cv_t<P>>(a)), ...);
  return fits;
}
// The node of the `n` members at `members` (n x sizeof(CaptureMember) bytes, 1 <= n <= kMaxMerge) under the tuning value
// packed_group_fold: try_join and the head regrouping build every node through this.  False: the members cannot share a node.
struct CaptureNode {
  hipKernelNodeParams params;
  int fold = 1;  // > 1: the folded form
  void* args[CaptureMember::kMaxArgs];
  std::vector<unsigned char> store;  // what args point into (the runtime copies it when the node is set)
};
bool capture_build_node(const unsigned char* members, int n, CaptureNode& out);

// The first kernel of a packed matvec call on a stream that is being captured: ordered by the memory the call touches, not
// by the order of issue (capture_overlap.h has the rule, api.hip the state shared by both builds of the packed entries).
//   CaptureRelax relax(stream);
//   if (relax.capturing()) { relax.fp.add(...); ...; relax.begin(); }
//   <launch>;  relax.launched();
// Outside a capture it costs the one status query.  A call that returns without launched() leaves the stream as it found it.
class CaptureRelax {
 public:
  explicit CaptureRelax(hipStream_t stream);
  ~CaptureRelax();
  CaptureRelax(const CaptureRelax&) = delete;
  CaptureRelax& operator=(const CaptureRelax&) = delete;
  bool capturing() const { return active_; }
  capture_overlap::Footprint fp;
  // `key` != 0: the launch is one grid of a kernel whose grouped form can run several such launches as one (capture_overlap.h,
  // "Grouped launches"); the key names the kernel instance, block size and LDS bytes, `member` is the launch's CaptureMember
  // (kept with the planner also at key 0: the head of a run may be regrouped later).  When begin() returns n > 0 the launch
  // may join a node that holds n launches already: group() is their members in order, and join_members() builds the node
  // for n + 1 and hands it to join().  join() false: the runtime refused the rewrite (counted, not an error); the stream is
  // set up for an ordinary launch and the caller makes one.
  int begin(uint64_t key = 0, const void* member = nullptr, size_t member_bytes = 0);
  const std::vector<unsigned char>& group() const { return plan_.payload; }
  // (null: the caller cannot build the node; `folded_delta`: +1 when this rewrite turns the node into its folded form
  // (group_fold.h), -1 when it turns it back -- added to the count of folded nodes when the rewrite holds)
  bool join(const hipKernelNodeParams* node, int folded_delta = 0);
  // (the same from the members: builds the node of group() plus this launch's member through capture_build_node)
  bool join_members();
  // After the launch (later launches of the call: no effect; nor after a join()).  0, or the error when the stream could not
  // be made to wait for the launches that ran beside this one: the capture would be wrong, so the call fails.
  int launched();

 private:
  void fail(const char* what, hipError_t e);
  void apply_plan();
  void regroup_head(capture_overlap::Run& run, std::vector<capture_overlap::NodeId>& now);  // after the commit of launched(); caller holds the mutex
  hipStream_t stream_;
  bool active_ = false, begun_ = false, done_ = false, changed_ = false, head_touched_ = false;
  uint64_t key_ = 0;
  std::vector<unsigned char> member_;
  unsigned long long id_ = 0;
  std::vector<capture_overlap::NodeId> before_;  // the stream's dependency set as the call found it
  capture_overlap::Plan plan_;
};

// slice-scan MFMA kernel of the 1x16 g8 scheme at 2+ rows (gemm_1x16_scan.hip); aqlm_hip_gemm_1x16_mfma (gemm_mfma_entries.h) routes to it
namespace scan {
size_t workspace_bytes(int B, int M, int K);  // 0: no plan (in_features % 256 != 0)
int run(const void* codes, const void* codebook, const void* scales, const void* bias, const void* X, void* Y, int batch, int out_features,
        int in_features, long xs, long ys, int dtype, void* workspace, hipStream_t stream);
}  // namespace scan

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned2(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }
// an id array (int64 or int32) is aligned to its element
inline bool ids_aligned(const void* ids, int ids_int64) { return (reinterpret_cast<uintptr_t>(ids) & (ids_int64 ? 7u : 3u)) == 0; }
// the reference of the code searches (fp16, bf16 or fp32) is aligned to its element; element `idx` of it as fp32
inline bool ref_aligned(const void* p, int dtype) { return dtype == AQLM_HIP_F32 ? aligned4(p) : aligned2(p); }
__device__ __forceinline__ float load_ref(const void* p, size_t idx, int dtype) {
  if (dtype == AQLM_HIP_F32) return reinterpret_cast<const float*>(p)[idx];
  const uint16_t u = reinterpret_cast<const uint16_t*>(p)[idx];
  return dtype == AQLM_HIP_BF16 ? BF16::to_float(u) : F16::to_float(u);
}
// dW and the outputs of the gradient kernels: fp16, bf16 or fp32 (the tag of the third beside F16 / BF16)
struct F32 {
  static constexpr int id = AQLM_HIP_F32;
};
inline bool dw_dtype_ok(int dtype) { return dtype == AQLM_HIP_F16 || dtype == AQLM_HIP_BF16 || dtype == AQLM_HIP_F32; }
inline size_t dtype_bytes(int dtype) { return dtype == AQLM_HIP_F32 ? 4 : 2; }
// the 16 bits of an fp16 / bf16 scale as fp32, for kernels that are not instantiated per scale dtype
__device__ __forceinline__ float half_bits_to_float(uint32_t u16, int is_bf16) {
  return is_bf16 ? __uint_as_float(u16 << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)u16);
}

// ---------------------------------------------------------------------------------------------
// Argument checks that the indexed entry points (routed, routed packed, bucket, grouped, transposed, LoRA) and the dense MFMA GEMM
// entries share.  Each sets the message and returns the code when its condition is violated, else 0; an entry point calls them in
// the order in which it reports: `if (int e = check_...(who, ...)) return e;`
// ---------------------------------------------------------------------------------------------
inline int check_not_null(const char* who, bool all_set) {
  if (all_set) return 0;
  set_last_error("%s: null pointer argument", who);
  return AQLM_HIP_E_INVALID;
}
// `what` names the arguments, e.g. "table / bucket"
inline int check_aligned(const char* who, const char* what, bool ok) {
  if (ok) return 0;
  set_last_error("%s: %s misaligned", who, what);
  return AQLM_HIP_E_INVALID;
}
inline int check_experts(const char* who, int num_experts, int num_segments) {
  if (num_experts >= 1 && num_experts <= AQLM_HIP_MAX_ROUTED_EXPERTS && num_segments >= 1 && num_segments <= 2) return 0;
  set_last_error("%s: %d experts x %d segments (1..%d x 1..2 supported)", who, num_experts, num_segments, AQLM_HIP_MAX_ROUTED_EXPERTS);
  return AQLM_HIP_E_INVALID;
}
inline int check_pairs(const char* who, int num_pairs, int top_k, int max_pairs) {
  if (num_pairs >= 1 && num_pairs <= max_pairs && top_k >= 1 && num_pairs % top_k == 0) return 0;
  set_last_error("%s: %d pairs with top_k %d (1..%d pairs, a multiple of top_k)", who, num_pairs, top_k, max_pairs);
  return AQLM_HIP_E_INVALID;
}
inline int check_sizes(const char* who, int out_features, int in_features, int in_group_size) {
  if (out_features > 0 && in_features > 0 && in_group_size > 0 && in_features % in_group_size == 0) return 0;
  set_last_error("%s: bad sizes (out=%d in=%d g=%d)", who, out_features, in_features, in_group_size);
  return AQLM_HIP_E_INVALID;
}
// the three sizes of a dense forward entry
inline int check_positive(const char* who, int batch, int out_features, int in_features) {
  if (batch > 0 && out_features > 0 && in_features > 0) return 0;
  set_last_error("%s: sizes must be positive", who);
  return AQLM_HIP_E_INVALID;
}
inline int check_dtype(const char* who, int dtype) {
  if (dtype == AQLM_HIP_F16 || dtype == AQLM_HIP_BF16) return 0;
  set_last_error("%s: AQLM HIP kernels only support float16 and bfloat16 (dtype id %d)", who, dtype);
  return AQLM_HIP_E_UNSUPPORTED;
}
inline int check_group_size(const char* who, int in_group_size) {
  if (in_group_size == 8 || in_group_size == 16) return 0;
  set_last_error("%s: only codebooks with 8 or 16 features are supported, got %d", who, in_group_size);
  return AQLM_HIP_E_UNSUPPORTED;
}
// x_row_stride of the dense forward entries (include/aqlm_hip.h, "input of the dense forward entries"), the one place that looks at its
// sign.  One row has no stride: the argument is not read there and becomes in_features, so that it passes every later check and
// selects no kernel.  At 2+ rows a negative stride is refused for every entry alike; 0 and overlapping rows are legal.
inline int check_x_row_stride(const char* who, int batch, int in_features, long& x_row_stride) {
  if (batch <= 1) {
    x_row_stride = in_features;
    return 0;
  }
  if (x_row_stride >= 0) return 0;
  set_last_error("%s: negative x_row_stride %ld (rows of x)", who, x_row_stride);
  return AQLM_HIP_E_INVALID;
}

template <int V>
struct GroupSize {
  static constexpr int value = V;
};
// the tail of an entry point with checked arguments: f(F16{} or BF16{}, GroupSize<8>{} or GroupSize<16>{})
template <class F>
inline int dispatch_dtype_group(int dtype, int in_group_size, F&& f) {
  if (dtype == AQLM_HIP_F16) return in_group_size == 8 ? f(F16{}, GroupSize<8>{}) : f(F16{}, GroupSize<16>{});
  return in_group_size == 8 ? f(BF16{}, GroupSize<8>{}) : f(BF16{}, GroupSize<16>{});
}
template <int V>
struct Codebooks {
  static constexpr int value = V;
};
// its sibling for the 1x8 / 2x8 entries (num_codebooks checked to be 1 or 2): f(F16{} or BF16{}, Codebooks<1>{} or Codebooks<2>{})
template <class F>
inline int dispatch_dtype_k(int dtype, int num_codebooks, F&& f) {
  if (dtype == AQLM_HIP_F16) return num_codebooks == 2 ? f(F16{}, Codebooks<2>{}) : f(F16{}, Codebooks<1>{});
  return num_codebooks == 2 ? f(BF16{}, Codebooks<2>{}) : f(BF16{}, Codebooks<1>{});
}

}  // namespace aqlm

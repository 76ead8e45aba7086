// Host-side glue shared by every entry point of libaqlm_hip.so: error reporting, ABI version, tuning knobs.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

#include "aqlm_common.h"

namespace aqlm {

static thread_local char g_err[512] = "";

void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  set_last_error("%s: %s (%d)", what, hipGetErrorString(e), (int)e);
  return (int)e;
}

int ensure_dynamic_lds(const void* kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return 0;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> granted;
  int dev = 0;
  if (int e = check_hip(hipGetDevice(&dev), "hipGetDevice")) return e;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[{kernel, dev}];
  if (have >= bytes) return 0;
  if (int e = check_hip(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes),
                        "hipFuncSetAttribute(MaxDynamicSharedMemorySize)"))
    return e;
  have = bytes;
  return 0;
}

Tuning& tuning() {
  static Tuning t;
  return t;
}

static int* tuning_slot(const char* key) {
  Tuning& t = tuning();
  if (!key) return nullptr;
  if (!strcmp(key, "gemv_rows_per_wave")) return &t.gemv_rows_per_wave;
  if (!strcmp(key, "gemv1x16_aux")) return &t.gemv1x16_aux;
  if (!strcmp(key, "gemv1x16_prefetch_cb")) return &t.gemv1x16_prefetch_cb;
  if (!strcmp(key, "kx8_replicas")) return &t.kx8_replicas;
  if (!strcmp(key, "gemm_variant")) return &t.gemm_variant;
  if (!strcmp(key, "kx8_mfma_min_rows")) return &t.kx8_mfma_min_rows;
  if (!strcmp(key, "kx8_xres")) return &t.kx8_xres;
  if (!strcmp(key, "kx8_xres_phased")) return &t.kx8_xres_phased;
  if (!strcmp(key, "kx8_phase_tpb")) return &t.kx8_phase_tpb;
  if (!strcmp(key, "kx8_phase_quads")) return &t.kx8_phase_quads;
  if (!strcmp(key, "kx8_multi_xres_min_rows")) return &t.kx8_multi_xres_min_rows;
  if (!strcmp(key, "kx8_ksplit")) return &t.kx8_ksplit;
  if (!strcmp(key, "kx8_rt")) return &t.kx8_rt;
  if (!strcmp(key, "scan_max_rows")) return &t.scan_max_rows;
  if (!strcmp(key, "scan_prefetch")) return &t.scan_prefetch;
  if (!strcmp(key, "gemm_debug")) return &t.gemm_debug;
  if (!strcmp(key, "gemm_store_nt")) return &t.gemm_store_nt;
  if (!strcmp(key, "force_generic")) return &t.force_generic;
  if (!strcmp(key, "packed_waves")) return &t.packed_waves;
  if (!strcmp(key, "packed_fused_finalize")) return &t.packed_fused_finalize;
  if (!strcmp(key, "packed_prefetch")) return &t.packed_prefetch;
  if (!strcmp(key, "packed_arrange")) return &t.packed_arrange;
  if (!strcmp(key, "packed_xcopies")) return &t.packed_xcopies;
  if (!strcmp(key, "packed_entry_bytes")) return &t.packed_entry_bytes;
  if (!strcmp(key, "packed_debug")) return &t.packed_debug;
  if (!strcmp(key, "packed_fill_rotate")) return &t.packed_fill_rotate;
  if (!strcmp(key, "packed_compact_window")) return &t.packed_compact_window;
  if (!strcmp(key, "packed_capture_window")) return &t.packed_capture_window;
  if (!strcmp(key, "packed_capture_min_run")) return &t.packed_capture_min_run;
  if (!strcmp(key, "packed_capture_merge")) return &t.packed_capture_merge;
  if (!strcmp(key, "packed_capture_head")) return &t.packed_capture_head;
  if (!strcmp(key, "packed_group_fold")) return &t.packed_group_fold;
  if (!strcmp(key, "packed_pipe")) return &t.packed_pipe;
  if (!strcmp(key, "packed_prefetch_waves")) return &t.packed_prefetch_waves;
  if (!strcmp(key, "packed_dequant_by_xcd")) return &t.packed_dequant_by_xcd;
  if (!strcmp(key, "lut_waves")) return &t.lut_waves;
  return nullptr;
}

// ---------------------------------------------------------------------------------------------
// Capture overlap: the HIP side of capture_overlap.h.  One planner for the process (both builds of the packed entries launch
// through it), behind one mutex that is never held across a launch.
// ---------------------------------------------------------------------------------------------
namespace {
struct CaptureOverlapState {
  std::mutex mu;
  capture_overlap::Planner planner;
  // seen, relaxed, kept for a conflict, kept for the window, runs broken, API failures; then: launches that joined a node
  // (also counted as kept for the window), rewrites of a node the runtime refused, launches that added a node of their own,
  // nodes that went over to the folded grouped kernel (group_fold.h); then: runs whose head was regrouped, head launches that
  // gave up a node of their own, head scripts that stopped early (capture_overlap.h, "Regrouping the head")
  static constexpr int kStats = 13;
  uint64_t stats[kStats] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool off = false;                        // a capture call failed once: every launch as issued from then on
  bool head_off = false;                   // a head script stopped early once: no head is regrouped from then on
};
CaptureOverlapState& capture_state() {
  static CaptureOverlapState s;
  return s;
}
hipError_t set_capture_deps(hipStream_t stream, const std::vector<capture_overlap::NodeId>& nodes) {
  static_assert(sizeof(hipGraphNode_t) == sizeof(capture_overlap::NodeId), "a graph node handle is carried as a 64-bit id");
  std::vector<hipGraphNode_t> d;
  for (capture_overlap::NodeId n : nodes) d.push_back(reinterpret_cast<hipGraphNode_t>(static_cast<uintptr_t>(n)));
  return hipStreamUpdateCaptureDependencies(stream, d.empty() ? nullptr : d.data(), d.size(), hipStreamSetCaptureDependencies);
}
bool same_nodes(const std::vector<capture_overlap::NodeId>& a, const std::vector<capture_overlap::NodeId>& b) {
  return a.size() == b.size() && std::is_permutation(a.begin(), a.end(), b.begin());
}
// the stream's capture status; false (and the error) when the query itself failed
bool read_capture(hipStream_t stream, bool& capturing, unsigned long long& id, std::vector<capture_overlap::NodeId>& deps, hipError_t& err) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipGraphNode_t* d = nullptr;
  size_t n = 0;
  hipGraph_t graph = nullptr;
  err = hipStreamGetCaptureInfo_v2(stream, &st, &id, &graph, &d, &n);
  if (err != hipSuccess) return false;
  capturing = st == hipStreamCaptureStatusActive;
  deps.clear();
  if (capturing)
    for (size_t i = 0; i < n; ++i) deps.push_back(static_cast<capture_overlap::NodeId>(reinterpret_cast<uintptr_t>(d[i])));
  return true;
}
}  // namespace

bool capture_build_node(const unsigned char* members, int n, CaptureNode& out) {
  if (!members || n < 1 || n > capture_overlap::kMaxMerge) return false;
  CaptureMember m0;
  memcpy(&m0, members, sizeof m0);
  out.params = hipKernelNodeParams{};
  out.params.blockDim = dim3(m0.threads);
  out.params.sharedMemBytes = m0.lds;
  out.params.kernelParams = out.args;
  out.params.extra = nullptr;
  out.fold = 1;
  if (n == 1) {  // the launch as its call made it
    if (!m0.func || m0.nargs == 0 || m0.nargs > CaptureMember::kMaxArgs) return false;
    out.store.assign(m0.args, m0.args + CaptureMember::kArgBytes);
    for (unsigned i = 0; i < m0.nargs; ++i) {
      if (m0.arg_off[i] >= CaptureMember::kArgBytes) return false;
      out.args[i] = out.store.data() + m0.arg_off[i];
    }
    out.params.func = const_cast<void*>(m0.func);
    out.params.gridDim = dim3(m0.grid);
    return true;
  }
  if (!m0.group_func || m0.seg_bytes == 0 || m0.seg_bytes > CaptureMember::kSegBytes || m0.seg_bytes % 8 != 0) return false;
  const size_t segs = (size_t)capture_overlap::kMaxMerge * m0.seg_bytes;  // the grouped kernels' first argument, whole
  out.store.assign(segs + sizeof(int), 0);
  bool one_row = m0.fold_func != nullptr;  // the folded kernel finalizes one row per thread
  for (int i = 0; i < n; ++i) {
    CaptureMember m;
    memcpy(&m, members + (size_t)i * sizeof m, sizeof m);
    if (m.group_func != m0.group_func || m.fold_func != m0.fold_func || m.threads != m0.threads || m.lds != m0.lds || m.seg_bytes != m0.seg_bytes)
      return false;
    memcpy(out.store.data() + (size_t)i * m0.seg_bytes, m.seg, m0.seg_bytes);
    one_row = one_row && m.rows_per_group <= (int)m0.threads;
  }
  out.fold = one_row ? group_fold::choose(tuning().packed_group_fold, n) : 1;
  memcpy(out.store.data() + segs, &out.fold, sizeof(int));
  out.args[0] = out.store.data();
  out.args[1] = out.store.data() + segs;  // (the unfolded kernel takes the first only)
  out.params.func = const_cast<void*>(out.fold > 1 ? m0.fold_func : m0.group_func);
  out.params.gridDim = dim3(group_fold::grid(n, out.fold));
  return true;
}

void CaptureRelax::fail(const char* what, hipError_t e) {
  (void)hipGetLastError();  // the launch that follows checks the sticky error: this one is ours
  CaptureOverlapState& s = capture_state();
  s.off = true;
  ++s.stats[5];
  set_last_error("capture overlap switched off for this process: %s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

CaptureRelax::CaptureRelax(hipStream_t stream) : stream_(stream) {
  if (!stream) return;  // the null stream cannot be captured
  CaptureOverlapState& s = capture_state();
  {
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.off) return;
  }
  bool capturing = false;
  hipError_t err = hipSuccess;
  if (!read_capture(stream, capturing, id_, before_, err)) {
    std::lock_guard<std::mutex> lock(s.mu);
    fail("hipStreamGetCaptureInfo_v2", err);
    return;
  }
  if (!capturing) return;
  const int window = tuning().packed_capture_window;
  std::lock_guard<std::mutex> lock(s.mu);
  ++s.stats[0];
  ++s.stats[8];  // (a launch that joins a node takes it back)
  if (window <= 1 && tuning().packed_capture_merge <= 1) ++s.stats[3];  // exactly the graph as issued: nothing to plan
  else active_ = true;
}

// counts the plan and makes the stream wait for what it names (an ordinary launch follows); caller holds the mutex
void CaptureRelax::apply_plan() {
  CaptureOverlapState& s = capture_state();
  ++s.stats[plan_.kind == capture_overlap::kBroken ? 4 : (int)plan_.kind];
  if (plan_.kind == capture_overlap::kBroken || same_nodes(plan_.deps, before_)) return;
  const hipError_t e = set_capture_deps(stream_, plan_.deps);
  if (e == hipSuccess) {
    changed_ = true;
    return;
  }
  // the stream still waits for everything it did: launch as issued
  fail("hipStreamUpdateCaptureDependencies", e);
  s.planner.run(id_).reset();
  active_ = false;
}

int CaptureRelax::begin(uint64_t key, const void* member, size_t member_bytes) {
  if (!active_ || begun_) return 0;
  begun_ = true;
  const int merge = std::min(std::max(tuning().packed_capture_merge, 1), capture_overlap::kMaxMerge);
  if (member) member_.assign(static_cast<const unsigned char*>(member), static_cast<const unsigned char*>(member) + member_bytes);
  if (merge > 1 && key != 0 && member) key_ = key;
  CaptureOverlapState& s = capture_state();
  std::lock_guard<std::mutex> lock(s.mu);
  plan_ = s.planner.run(id_).plan(before_.data(), before_.size(), fp, tuning().packed_capture_window, tuning().packed_capture_min_run,
                                  key_, merge);
  if (plan_.merge) return plan_.member;  // counted by join()
  apply_plan();
  return 0;
}

bool CaptureRelax::join(const hipKernelNodeParams* node, int folded_delta) {
  if (!active_ || !begun_ || done_ || !plan_.merge) return false;
  CaptureOverlapState& s = capture_state();
  std::lock_guard<std::mutex> lock(s.mu);
  capture_overlap::Run& run = s.planner.run(id_);
  // The node has no dependents (it is in the tail) and stays where it is in the graph: only what it launches changes, and
  // the runtime copies the arguments.  The stream's dependency set is the tail before and after.
  // (A plan that another launch of this capture has overtaken is not acted on: the node is only touched when the commit holds.)
  const hipError_t e = node && run.latest(plan_)
                           ? hipGraphKernelNodeSetParams(reinterpret_cast<hipGraphNode_t>(static_cast<uintptr_t>(plan_.target)), node)
                           : hipErrorInvalidValue;
  if (e == hipSuccess && run.commit(plan_, plan_.target, fp, member_.data(), member_.size())) {
    ++s.stats[3];
    ++s.stats[6];
    --s.stats[8];
    s.stats[9] += (uint64_t)(int64_t)folded_delta;
    done_ = true;
    return true;
  }
  // refused (the node is as it was: the call changes it or fails), or the plan went stale: today's edge instead
  (void)hipGetLastError();
  ++s.stats[7];
  plan_ = run.plan(before_.data(), before_.size(), fp, tuning().packed_capture_window, tuning().packed_capture_min_run, key_, 1);
  apply_plan();
  return false;
}

bool CaptureRelax::join_members() {
  const size_t n = plan_.merge ? (size_t)plan_.member : 0;
  if (n == 0 || n >= (size_t)capture_overlap::kMaxMerge || plan_.payload.size() != n * sizeof(CaptureMember) || member_.size() != sizeof(CaptureMember))
    return join(nullptr);
  std::vector<unsigned char> all(plan_.payload);
  all.insert(all.end(), member_.begin(), member_.end());
  // The node is rewritten on every join, so the choice of its form follows the member count: folded from F members on (the grid
  // never drops under 256 workgroups), the unfolded kernel below that.  The planner's key is the unfolded instance's either way.
  CaptureNode before, after;
  if (!capture_build_node(all.data(), (int)n + 1, after)) return join(nullptr);
  const bool was_folded = capture_build_node(plan_.payload.data(), (int)n, before) && before.fold > 1;
  return join(&after.params, (after.fold > 1 ? 1 : 0) - (was_folded ? 1 : 0));
}

// "Regrouping the head" (capture_overlap.h): the run has just reached packed_capture_min_run launches.  Every node is built
// before the graph is touched; then the script step by step, and the planner is told how far it got.  `now`: the stream's
// dependency set, kept current.
void CaptureRelax::regroup_head(capture_overlap::Run& run, std::vector<capture_overlap::NodeId>& now) {
  CaptureOverlapState& s = capture_state();
  if (s.head_off || tuning().packed_capture_head == 0) return;
  const int merge = std::min(std::max(tuning().packed_capture_merge, 1), capture_overlap::kMaxMerge);
  const capture_overlap::HeadScript script = run.regroup_head(tuning().packed_capture_min_run, merge);
  if (script.empty()) return;
  using capture_overlap::HeadStep;
  std::vector<CaptureNode> nodes(script.steps.size());
  uint64_t folded = 0;
  for (size_t k = 0; k < script.steps.size(); ++k) {
    const HeadStep& st = script.steps[k];
    if (st.op != HeadStep::kRewrite) continue;
    if (st.payload.size() != st.members.size() * sizeof(CaptureMember) ||
        !capture_build_node(st.payload.data(), (int)st.members.size(), nodes[k])) {
      run.head_applied(0);  // a group that cannot be built: the graph stays as issued
      ++s.stats[12];
      return;
    }
    folded += nodes[k].fold > 1;
  }
  size_t done = 0;
  hipError_t e = hipSuccess;
  const char* what = "";
  for (; done < script.steps.size(); ++done) {
    const HeadStep& st = script.steps[done];
    const hipGraphNode_t node = reinterpret_cast<hipGraphNode_t>(static_cast<uintptr_t>(st.node));
    if (st.op == HeadStep::kRewrite) {
      what = "hipGraphKernelNodeSetParams";
      e = hipGraphKernelNodeSetParams(node, &nodes[done].params);
    } else if (st.op == HeadStep::kSetStreamDeps) {
      what = "hipStreamUpdateCaptureDependencies";
      e = set_capture_deps(stream_, {st.node});
      if (e == hipSuccess) now.assign(1, st.node);
    } else {
      what = "hipGraphDestroyNode";
      e = hipGraphDestroyNode(node);
    }
    if (e != hipSuccess) break;
    head_touched_ = true;
  }
  run.head_applied(done);
  if (done == script.steps.size()) {
    ++s.stats[10];
    s.stats[11] += script.moved;
    s.stats[9] += folded;
    return;
  }
  // every prefix of the script is a correct graph: the capture goes on from what is left, and no head is regrouped again
  (void)hipGetLastError();
  ++s.stats[12];
  s.head_off = true;
  set_last_error("capture overlap: regrouping of run heads switched off for this process: %s: %s (%d) at step %zu of %zu", what,
                 hipGetErrorString(e), (int)e, done, script.steps.size());
}

int CaptureRelax::launched() {
  if (!active_ || !begun_ || done_) return 0;
  done_ = true;
  CaptureOverlapState& s = capture_state();
  std::lock_guard<std::mutex> lock(s.mu);
  capture_overlap::Run& run = s.planner.run(id_);
  bool capturing = false;
  unsigned long long id = 0;
  std::vector<capture_overlap::NodeId> now;
  hipError_t err = hipSuccess;
  const bool read = read_capture(stream_, capturing, id, now, err);
  std::vector<capture_overlap::NodeId> want;
  if (read && capturing && id == id_ && now.size() == 1 && run.commit(plan_, now[0], std::move(fp), member_.data(), member_.size())) {
    if (plan_.head) regroup_head(run, now);
    want = run.tail();
  } else {
    // the new node is not known: everything the call found, and whatever the stream names now
    if (!read) fail("hipStreamGetCaptureInfo_v2", err);
    run.reset();
    if (!changed_) return 0;  // the launch was chained as issued
    want = before_;
    for (capture_overlap::NodeId n : now)
      if (std::find(want.begin(), want.end(), n) == want.end()) want.push_back(n);
    if (!read || !capturing) {
      set_last_error("capture overlap: the stream's capture state was lost after a launch that had been moved");
      return AQLM_HIP_E_INVALID;
    }
  }
  if (same_nodes(want, now)) return 0;
  const hipError_t e = set_capture_deps(stream_, want);
  if (e == hipSuccess) return 0;
  run.reset();
  const bool moved = changed_ || head_touched_ || want.size() > 1;
  fail("hipStreamUpdateCaptureDependencies", e);
  return moved ? (int)e : 0;
}

CaptureRelax::~CaptureRelax() {
  if (!active_ || !begun_ || done_) return;
  // the call ends without its launch: the stream waits for what it waited for before
  CaptureOverlapState& s = capture_state();
  std::lock_guard<std::mutex> lock(s.mu);
  s.planner.run(id_).reset();
  if (!changed_) return;
  const hipError_t e = set_capture_deps(stream_, before_);
  if (e != hipSuccess) fail("hipStreamUpdateCaptureDependencies", e);
}

// position-sensitive checksum (include/aqlm_hip.h): per-thread partial sums, wave reduction through the atomics' return path is
// not needed -- 64-bit atomic adds commute, so the result does not depend on the order the waves arrive in
__global__ __launch_bounds__(256) void checksum_kernel(const uint8_t* data, size_t bytes, unsigned long long* out) {
  const size_t nwords = (bytes + 3) / 4;
  const bool aligned = (reinterpret_cast<uintptr_t>(data) & 3u) == 0;
  unsigned long long a = 0, b = 0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) {
    uint32_t w = 0;
    if (aligned && i * 4 + 4 <= bytes) w = reinterpret_cast<const uint32_t*>(data)[i];
    else
      for (size_t k = 0; k < 4 && i * 4 + k < bytes; ++k) w |= (uint32_t)data[i * 4 + k] << (8 * k);
    a += w;
    b += (unsigned long long)w * (((unsigned long long)i * 0x9E3779B97F4A7C15ull) | 1ull);
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, WAVE);
    b += __shfl_xor(b, o, WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[0], a);
    atomicAdd(&out[1], b);
  }
}

}  // namespace aqlm

extern "C" int aqlm_hip_checksum(const void* data, size_t bytes, void* out_u64x2, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out_u64x2 || (!data && bytes) || (reinterpret_cast<uintptr_t>(out_u64x2) & 7u)) {
    aqlm::set_last_error("aqlm_hip_checksum: null pointer argument or misaligned output");
    return AQLM_HIP_E_INVALID;
  }
  if (int e = aqlm::check_hip(hipMemsetAsync(out_u64x2, 0, 16, stream), "checksum memset")) return e;
  if (bytes == 0) return 0;
  const size_t nwords = (bytes + 3) / 4;
  const unsigned blocks = (unsigned)std::min<size_t>(2048, (nwords + 255) / 256);
  hipLaunchKernelGGL(aqlm::checksum_kernel, dim3(blocks), dim3(256), 0, stream, (const uint8_t*)data, bytes, (unsigned long long*)out_u64x2);
  return aqlm::check_hip(hipGetLastError(), "checksum launch");
}

static int capture_overlap_stats(uint64_t* out, int n) {
  aqlm::CaptureOverlapState& s = aqlm::capture_state();
  std::lock_guard<std::mutex> lock(s.mu);
  for (int i = 0; i < aqlm::CaptureOverlapState::kStats; ++i) {
    if (!out) s.stats[i] = 0;
    else if (i < n) out[i] = s.stats[i];
  }
  return 0;
}

extern "C" int aqlm_hip_capture_overlap_stats(uint64_t out[6]) { return capture_overlap_stats(out, 6); }

extern "C" int aqlm_hip_capture_overlap_stats_ex(uint64_t* out, int count) {
  if (out && (count < 0 || count > aqlm::CaptureOverlapState::kStats)) {
    aqlm::set_last_error("aqlm_hip_capture_overlap_stats_ex: count must be 0..13 (got %d)", count);
    return AQLM_HIP_E_INVALID;
  }
  return capture_overlap_stats(out, count);
}

extern "C" int aqlm_hip_abi_version(void) { return AQLM_HIP_ABI_VERSION; }

extern "C" const char* aqlm_hip_last_error(void) { return aqlm::g_err; }

extern "C" int aqlm_hip_set_tuning(const char* key, int value) {
  int* s = aqlm::tuning_slot(key);
  if (!s) {
    aqlm::set_last_error("aqlm_hip_set_tuning: unknown key '%s'", key ? key : "(null)");
    return AQLM_HIP_E_INVALID;
  }
  *s = value;
  return 0;
}

extern "C" int aqlm_hip_get_tuning(const char* key, int* value) {
  int* s = aqlm::tuning_slot(key);
  if (!s || !value) {
    aqlm::set_last_error("aqlm_hip_get_tuning: unknown key '%s'", key ? key : "(null)");
    return AQLM_HIP_E_INVALID;
  }
  *value = *s;
  return 0;
}

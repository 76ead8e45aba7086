// Capture overlap: which earlier launches a launch captured into a graph really has to wait for.  Plain C++17, no HIP: the
// launch side (aqlm_common.h: CaptureRelax, api.hip) hands in opaque node ids and byte ranges and installs what comes back;
// tests/capture_overlap_host.cpp drives the same code on the CPU.
//
// A stream under capture only describes a dependency graph, and whoever adds a node may choose its dependencies.  The library
// knows the memory every packed matvec reads and writes, so consecutive launches that share none of it need no edge between
// them: the next layer's workgroups start on CUs as the previous layer's leave them, instead of after its last one.
//
// Per capture id the planner keeps the RUN of library launches it has added: the dependency set the run started from (base)
// and a TAIL of at most W launches that nothing captured so far waits for, each with its footprint.  For a new launch, given
// the stream's current dependency set D:
//   1. D is not exactly the tail (a foreign node, an event wait, another capture, the first launch): the run is broken;
//      base := D, the launch depends on D, tail := {launch}.
//   2. otherwise it depends on every tail launch whose footprint overlaps its own with a write on either side (RAW, WAR, WAW);
//      with no such launch and a full tail, on the oldest tail launch (W chains, never more than W launches in flight); with
//      neither, on base alone.  Every tail launch is ordered after base, so base is named only when no tail launch is.
//      The tail launches it depends on leave the tail, the new launch joins it -- and answers for them from then on: a tail
//      entry's footprint is its launch's own plus those of the launches that left the tail through it, because a later launch
//      that touches the memory of one of those can only be ordered after it by waiting for the entry.  (Comparing with the
//      launch's own footprint alone loses exactly that hazard: A, B in the tail; C waits for A; D touches A's memory but not
//      C's.)  A footprint that would outgrow kMaxRanges is handled like a broken run: the launch waits for the whole tail.
//   3. after the launch the caller sets the stream's dependency set to the tail: whatever is captured next, by anyone, waits
//      for every launch it could observe.
//
// Grouped launches.  Every node of a replayed graph pays a dependent-launch boundary, and the next node of a chain starts only
// when the last workgroup of the previous one has left; inside one launch the dispatcher backfills a CU the moment a workgroup
// leaves it.  So a launch may JOIN the node of a tail entry instead of adding one, when the caller can run both as one grid: it
// hands in a KEY (kernel instance, block size, LDS bytes; 0 = launches alone) and only equal keys share a node, at most
// `merge_max` launches each.  Where step 2 would answer "no hazard, tail full: wait for the oldest entry", the oldest entry
// with the launch's key and room left takes the launch in: no node is added, the entry's footprint absorbs the launch's (it
// has been checked against every tail entry's footprint, that entry's included, so it may run beside all of them and after
// everything the entry's node waits for), and the entry becomes the youngest of the tail, so that the next launch of another
// key finds its own partner first.  The caller rewrites the node (Plan::target, Plan::member); the members' launch parameters
// travel with the entry as an opaque payload.  A full group, another key, a footprint that would outgrow kMaxRanges: the
// answers of step 2 as they were.  The stream's dependency set after a joined launch is the tail, the same nodes as before.
//
// Regrouping the head.  A run relaxes and joins nothing until it holds `min_run` launches (kDefaultMinRun has the reason), so
// the first `min_run` launches of a long run -- its HEAD -- are a chain of single launches, each waiting for the one before:
// only at the last of them does the planner learn that the run is long.  Until then it keeps, per head launch, the node, the
// launch's own footprint, key and payload, and whether any of them was planned kConflict or restarted the run (kMaxRanges).
// If none was, the head launches are pairwise free of hazards (each was checked against the union of those before it), and
// after the commit that brings the run to `min_run` launches Run::regroup_head() regroups them in place: walking the head in
// issue order, a launch of key k joins the earliest group of key k with room (merge_max), else it opens one; keyless launches
// are groups of one; groups are ordered by their first member; group i takes the i-th node of the chain, whatever that node
// launched before, and the nodes left over -- a suffix of the chain -- go.  The head stays ONE chain in stream order and the
// run's base, length and later planning are untouched: launch min_run + 1 is still the first relaxed one.  What comes back is
// an edit script for the caller to apply in order,
//   Rewrite(node_i, members of group i)          for every group whose node launches something else now,
//   SetStreamDeps({predecessor}), Destroy(node)  for every surplus node, last to first,
// every prefix of which leaves a correct graph: after the rewrites alone a launch may run twice, each copy in a node of its
// own of the one chain (a repeated launch writes the same bits); every destroy removes a node nothing depends on.  The caller
// reports how far it got (head_applied): after the whole script the tail is the last group's node with that group's key,
// member count and payload, so that later launches may join it; after a script that stopped, the newest node that is left,
// with key 0.  Either way the entry keeps the footprint of the whole head.  Runs shorter than `min_run` see none of this.
#ifndef AQLM_CAPTURE_OVERLAP_H_
#define AQLM_CAPTURE_OVERLAP_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace aqlm {
namespace capture_overlap {

using NodeId = uint64_t;

constexpr int kMaxWindow = 8;
// Every branch of a replayed graph wants a hardware queue of its own, and a process opens 4 by default, which the capturing
// stream and every other stream share.  Measured on the 64-layer decode step (profiles/capture_overlap.json): 2 branches
// 391-396 us in every placement of the streams tried; 3 and 4 branches 397-411 us, or 450-455 us (stream order: 470) when two
// branches land on one queue, which depends on how many streams the process created before.  Two is faster and does not
// depend on that.
constexpr int kDefaultWindow = 2;
// A graph with branches leaves the runtime's single-stream replay and pays about 2 us of host time per node, for EVERY node of
// the graph (64 nodes: 20 -> 157 us of enqueue per replay).  Where the library's launches are the graph, as in a stack of
// linears, the kernels are longer than that and the overlap wins; in a decoder's graph of thousands of short framework nodes
// the replay becomes host-bound (Llama-3-8B decode loop: 5.84 -> 7.90 ms per token with q/k/v relaxed).  Nothing the planner
// sees tells the two apart except how long the library's launches go uninterrupted: a run relaxes nothing until it is this
// long, which q/k/v, gate/up and the like never are.
constexpr int kDefaultMinRun = 8;
constexpr int kMaxMerge = 8;  // launches that may share one node (the grouped kernel's segments)
// Measured on the 64-layer decode step at a window of 2 (profiles/capture_merge.json): 1 launch per node 357-359 us, 2: 377,
// 3: 361, 4: 345, 5: 336, 6: 334, 8: 338.  Small groups lose: two workgroups of the SAME launch may share a CU where before a
// workgroup of the other chain sat, and the longer chain waits for its place; from 4 on the saved boundaries and tails win.
// With folded nodes (group_fold.h) the best group size moved: four launches per node at four passes per workgroup, 292 us against
// 329 / 306 for six / eight (fold 2: 327 / 310 / 307; unfolded as above).
constexpr int kDefaultMerge = 4;
constexpr size_t kMaxRanges = 256;  // of one tail entry's footprint (a packed matvec brings 6 to 9)

struct Range {
  uintptr_t begin, end;  // [begin, end) in bytes
  bool writes;
};

struct Footprint {
  std::vector<Range> ranges;
  void add(const void* p, size_t bytes, bool writes) {
    if (!p || !bytes) return;
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    ranges.push_back(Range{b, b + bytes, writes});
  }
  // `rows` rows of `row_bytes` each, `stride_bytes` apart (any sign): one range when they touch, else one per row
  void add_rows(const void* p, int rows, long stride_bytes, size_t row_bytes, bool writes) {
    if (rows > 1 && stride_bytes == (long)row_bytes) return add(p, (size_t)rows * row_bytes, writes);
    for (int r = 0; r < rows; ++r) add(reinterpret_cast<const char*>(p) + (ptrdiff_t)r * stride_bytes, row_bytes, writes);
  }
};

inline bool hazard(const Footprint& a, const Footprint& b) {
  for (const Range& x : a.ranges)
    for (const Range& y : b.ranges)
      if ((x.writes || y.writes) && x.begin < y.end && y.begin < x.end) return true;
  return false;
}

enum Kind { kBroken = 0, kRelaxed = 1, kConflict = 2, kWindow = 3 };

struct Plan {
  Kind kind = kBroken;
  std::vector<NodeId> deps;   // what the launch depends on
  std::vector<size_t> leave;  // ascending tail positions of the launches among them
  bool restart = false;       // the launch starts a run: base := deps, tail := {launch}
  uint64_t generation = 0;    // of the run when it was planned: commit() takes only the latest plan
  uint64_t key = 0;           // of the launch (0: it shares no node)
  // the launch joins the node of a tail entry (kind stays kWindow; deps / leave are empty: no node is added)
  bool merge = false;
  size_t merge_pos = 0;                // tail position of that entry
  NodeId target = 0;                   // its node
  int member = 0;                      // the launch's index among the node's launches (>= 1)
  std::vector<unsigned char> payload;  // what the entry's launches left with commit(), in order
  bool head = false;                   // the launch is among the run's first `min_run` ("Regrouping the head")
};

// One step of the edit script that regroups a run's head.
struct HeadStep {
  enum Op { kRewrite = 0, kSetStreamDeps = 1, kDestroy = 2 };
  Op op = kRewrite;
  NodeId node = 0;                     // kRewrite: the node to rewrite; kSetStreamDeps: the node the stream is to wait for; kDestroy: the node
  uint64_t key = 0;                    // kRewrite: of the group
  std::vector<size_t> members;         // kRewrite: the group's launches, as positions in the head
  std::vector<unsigned char> payload;  // kRewrite: their payloads, in order
};
struct HeadScript {
  std::vector<HeadStep> steps;
  size_t groups = 0;  // nodes the head keeps
  size_t moved = 0;   // launches that gave up a node of their own (= nodes destroyed by the whole script)
  bool empty() const { return steps.empty(); }
};

class Run {
 public:
  uint64_t capture_id = 0;

  // Steps 1 and 2 for a launch with footprint `fp`; `deps` / `num_deps` = D.  Nothing is recorded until commit().
  // A run relaxes nothing until it holds `min_run` launches: until then every launch waits for the whole tail, as issued.
  // `key` / `merge_max`: the launch may join a tail entry of the same non-zero key that holds fewer than `merge_max` launches.
  Plan plan(const NodeId* deps, size_t num_deps, const Footprint& fp, int window, int min_run = 1, uint64_t key = 0,
            int merge_max = 1) {
    window = std::min(std::max(window, 1), kMaxWindow);
    merge_max = std::min(merge_max, kMaxMerge);
    Plan p;
    p.key = key;
    p.generation = ++generation_;
    p.head = true;  // (a launch that starts a run is its first)
    if (!is_tail(deps, num_deps)) {
      p.kind = kBroken;
      p.restart = true;
      p.deps.assign(deps, deps + num_deps);
      return p;
    }
    p.head = length_ < (size_t)std::max(min_run, 1);
    for (size_t i = 0; i < tail_.size(); ++i)
      if (hazard(tail_[i].fp, fp)) p.leave.push_back(i);
    if (!p.leave.empty()) {
      p.kind = kConflict;
    } else if (length_ < (size_t)std::max(min_run, 1)) {
      p.kind = kWindow;
      for (size_t i = 0; i < tail_.size(); ++i) p.leave.push_back(i);
    } else if ((int)tail_.size() >= window) {
      p.kind = kWindow;
      for (size_t i = 0; key != 0 && i < tail_.size(); ++i) {
        if (tail_[i].key != key || tail_[i].members >= merge_max) continue;
        if (fp.ranges.size() + tail_[i].fp.ranges.size() > kMaxRanges) {  // too much for one entry: wait for the whole tail
          p.restart = true;
          p.head = true;
          p.deps.assign(deps, deps + num_deps);
          return p;
        }
        p.merge = true;
        p.merge_pos = i;
        p.target = tail_[i].node;
        p.member = tail_[i].members;
        p.payload = tail_[i].payload;
        return p;
      }
      p.leave.push_back(0);  // the oldest
    } else {
      p.kind = kRelaxed;
      p.deps = base_;
      return p;
    }
    size_t ranges = fp.ranges.size();
    for (size_t i : p.leave) ranges += tail_[i].fp.ranges.size();
    if (ranges > kMaxRanges) {  // too much to answer for: wait for the whole tail (= D) and start over from there
      p.restart = true;
      p.head = true;
      p.leave.clear();
      p.deps.assign(deps, deps + num_deps);
      return p;
    }
    for (size_t i : p.leave) p.deps.push_back(tail_[i].node);
    return p;
  }

  // The launch of plan `p` became `node`: step 2's bookkeeping, after which tail() is what step 3 installs.  False (and
  // nothing recorded) when `p` is not the run's latest plan.
  // `payload`: the launch's parameters, opaque here; a later launch that joins the node gets them back (Plan::payload).
  bool commit(const Plan& p, NodeId node, Footprint fp, const void* payload = nullptr, size_t payload_bytes = 0) {
    if (p.generation != generation_) return false;
    const unsigned char* pb = static_cast<const unsigned char*>(payload);
    if (p.merge) {  // `node` is the entry's node (the caller rewrote it, or replaced it by a node with the same dependencies)
      Entry e = std::move(tail_[p.merge_pos]);
      tail_.erase(tail_.begin() + (ptrdiff_t)p.merge_pos);
      e.node = node;
      e.fp.ranges.insert(e.fp.ranges.end(), fp.ranges.begin(), fp.ranges.end());
      if (pb) e.payload.insert(e.payload.end(), pb, pb + payload_bytes);
      ++e.members;
      ++generation_;
      ++length_;
      tail_.push_back(std::move(e));  // the youngest now
      head_.clear();
      return true;
    }
    Footprint own;
    if (p.head && head_.size() == (p.restart ? 0 : length_)) own = fp;
    if (p.restart) {
      base_ = p.deps;
      tail_.clear();
      length_ = 0;
      head_.clear();
      head_ok_ = p.kind == kBroken;  // (a restart inside a run, kMaxRanges: its launches are not regrouped)
    } else {
      for (size_t k = p.leave.size(); k-- > 0;) {
        const Footprint& gone = tail_[p.leave[k]].fp;
        fp.ranges.insert(fp.ranges.end(), gone.ranges.begin(), gone.ranges.end());
        tail_.erase(tail_.begin() + (ptrdiff_t)p.leave[k]);
      }
    }
    // the head: every launch since the run began, while none is relaxed or joined
    if (p.head && head_.size() == length_) {
      if (p.kind == kConflict) head_ok_ = false;
      head_.push_back(HeadLaunch{node, own, p.key, std::vector<unsigned char>(pb, pb + (pb ? payload_bytes : 0))});
    } else {
      head_.clear();
    }
    ++generation_;
    ++length_;
    tail_.push_back(Entry{node, std::move(fp), p.key, 1, std::vector<unsigned char>(pb, pb + (pb ? payload_bytes : 0))});
    return true;
  }

  // "Regrouping the head": to be called after the commit that brought the run to `min_run` launches (any other time: an empty
  // script).  An empty script also when a head launch was planned kConflict or restarted the run, when no two head launches
  // share a non-zero key (or merge_max <= 1), and when a launch that would have to change nodes left no payload to build it
  // from.  A script that is not empty must be answered by head_applied() before the run plans again.
  HeadScript regroup_head(int min_run, int merge_max) {
    HeadScript s;
    merge_max = std::min(merge_max, kMaxMerge);
    const size_t n = head_.size();
    if (length_ < (size_t)std::max(min_run, 1)) return s;  // not yet
    if (!head_ok_ || merge_max <= 1 || n < 2 || n != length_ || n != (size_t)std::max(min_run, 1) || tail_.size() != 1 ||
        tail_[0].node != head_[n - 1].node) {
      head_.clear();
      return s;
    }
    std::vector<std::vector<size_t>> groups;
    for (size_t i = 0; i < n; ++i) {
      size_t g = groups.size();
      for (size_t k = 0; head_[i].key != 0 && k < groups.size() && g == groups.size(); ++k)
        if (head_[groups[k][0]].key == head_[i].key && groups[k].size() < (size_t)merge_max) g = k;
      if (g == groups.size()) groups.emplace_back();
      groups[g].push_back(i);
    }
    bool possible = groups.size() < n;
    for (size_t g = 0; g < groups.size(); ++g)
      for (size_t i : groups[g])
        if (i != g && head_[i].payload.empty()) possible = false;  // cannot be built in another node
    if (!possible) {
      head_.clear();
      return s;
    }
    for (size_t g = 0; g < groups.size(); ++g) {
      if (groups[g].size() == 1 && groups[g][0] == g) continue;  // the node launches exactly that already
      HeadStep st;
      st.op = HeadStep::kRewrite;
      st.node = head_[g].node;
      st.key = head_[groups[g][0]].key;
      st.members = groups[g];
      for (size_t i : groups[g]) st.payload.insert(st.payload.end(), head_[i].payload.begin(), head_[i].payload.end());
      s.steps.push_back(std::move(st));
    }
    for (size_t j = n; j-- > groups.size();) {
      HeadStep dep, gone;
      dep.op = HeadStep::kSetStreamDeps;
      dep.node = head_[j - 1].node;
      gone.op = HeadStep::kDestroy;
      gone.node = head_[j].node;
      s.steps.push_back(std::move(dep));
      s.steps.push_back(std::move(gone));
    }
    s.groups = groups.size();
    s.moved = n - groups.size();
    pending_ = s;
    pending_last_ = std::move(groups.back());
    ++generation_;  // nothing planned before the script holds afterwards
    return s;
  }

  // The caller applied the first `steps_done` steps of the script regroup_head() returned (all of them: the head is
  // regrouped; fewer: the script stopped there and the run keeps what is still true).  tail() is what the stream is to wait for.
  void head_applied(size_t steps_done) {
    if (pending_.empty() || tail_.size() != 1 || head_.empty()) return;
    ++generation_;
    Entry& e = tail_[0];
    if (steps_done >= pending_.steps.size()) {
      e.node = head_[pending_.groups - 1].node;
      e.key = head_[pending_last_[0]].key;
      e.members = (int)pending_last_.size();
      e.payload.clear();
      for (size_t i : pending_last_) e.payload.insert(e.payload.end(), head_[i].payload.begin(), head_[i].payload.end());
    } else {
      size_t destroyed = 0;
      for (size_t k = 0; k < steps_done; ++k) destroyed += pending_.steps[k].op == HeadStep::kDestroy;
      e.node = head_[head_.size() - 1 - destroyed].node;  // the newest node that is left; what it launches now is not tracked
      e.key = 0;
      e.members = 1;
      e.payload.clear();
    }
    pending_ = HeadScript{};
    pending_last_.clear();
    head_.clear();
  }

  bool latest(const Plan& p) const { return p.generation == generation_; }

  // Forget the run (its launch failed, or the new node could not be read): the next launch starts a new one.
  void reset() {
    ++generation_;
    base_.clear();
    tail_.clear();
    length_ = 0;
    head_.clear();
    head_ok_ = false;
    pending_ = HeadScript{};
    pending_last_.clear();
  }

  std::vector<NodeId> tail() const {
    std::vector<NodeId> t;
    for (const Entry& e : tail_) t.push_back(e.node);
    return t;
  }
  const std::vector<NodeId>& base() const { return base_; }

 private:
  struct Entry {
    NodeId node;
    Footprint fp;
    uint64_t key;  // of its launches (0: nothing joins it)
    int members;   // launches that share the node
    std::vector<unsigned char> payload;
  };
  bool is_tail(const NodeId* deps, size_t n) const {
    if (tail_.empty() || n != tail_.size()) return false;
    for (size_t i = 0; i < n; ++i) {
      bool found = false;
      for (const Entry& e : tail_) found = found || e.node == deps[i];
      if (!found) return false;
      for (size_t j = 0; j < i; ++j)
        if (deps[j] == deps[i]) return false;
    }
    return true;
  }
  struct HeadLaunch {
    NodeId node;
    Footprint fp;  // its own
    uint64_t key;
    std::vector<unsigned char> payload;
  };
  std::vector<NodeId> base_;
  std::vector<Entry> tail_;  // oldest first
  std::vector<HeadLaunch> head_;  // the run's launches so far, while there are at most `min_run` of them
  bool head_ok_ = false;          // none of them was planned kConflict or restarted the run after its first launch
  HeadScript pending_;            // the script regroup_head() handed out, until head_applied()
  std::vector<size_t> pending_last_;  // its last group
  size_t length_ = 0;        // launches of the run so far
  uint64_t generation_ = 0;
};

// The runs of the captures in progress: a few at most (one per capturing stream), the least recently used one makes room.
class Planner {
 public:
  Run& run(uint64_t capture_id) {
    ++clock_;
    size_t lru = 0;
    for (size_t i = 0; i < kSlots; ++i) {
      if (used_[i] && runs_[i].capture_id == capture_id) {
        used_[i] = clock_;
        return runs_[i];
      }
      if (used_[i] < used_[lru]) lru = i;
    }
    runs_[lru].reset();
    runs_[lru].capture_id = capture_id;
    used_[lru] = clock_;
    return runs_[lru];
  }

 private:
  static constexpr size_t kSlots = 4;
  Run runs_[kSlots];
  uint64_t used_[kSlots] = {0, 0, 0, 0};
  uint64_t clock_ = 0;
};

}  // namespace capture_overlap
}  // namespace aqlm
#endif  // AQLM_CAPTURE_OVERLAP_H_

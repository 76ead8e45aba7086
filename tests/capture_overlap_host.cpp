// Stand-alone check of aqlm_amd/csrc/capture_overlap.h (built and run by tests/test_capture_overlap_host.py with the address and
// undefined-behaviour sanitizers).  A tiny model of a stream under capture: its dependency set, launches of the library that go
// through the planner, and foreign nodes that take the set as it is.  Prints one line per case; exit status 0 = all passed.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../aqlm_amd/csrc/capture_overlap.h"

using namespace aqlm::capture_overlap;

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

struct Node {
  std::vector<NodeId> deps;
  Footprint fp;
  bool foreign;
};

// the capturing stream and the graph it has built so far; node ids are 100, 101, ...
struct Stream {
  uint64_t capture_id = 1;
  std::vector<Node> nodes;
  std::vector<NodeId> D;  // the stream's dependency set
  Planner planner;
  int window = 4;  // the cases state their graphs for a window of 4 and runs that relax from the second launch on;
  int min_run = 1;  // the library's defaults are kDefaultWindow and kDefaultMinRun
  Kind last = kBroken;

  static size_t idx(NodeId n) { return (size_t)(n - 100); }
  NodeId add(std::vector<NodeId> deps, Footprint fp, bool foreign) {
    nodes.push_back(Node{std::move(deps), std::move(fp), foreign});
    return 100 + nodes.size() - 1;
  }
  // what the launch side does: plan, install, launch, read the node back, set the tail
  NodeId launch(const Footprint& fp) {
    Run& run = planner.run(capture_id);
    Plan p = run.plan(D.data(), D.size(), fp, window, min_run);
    last = p.kind;
    const NodeId n = add(p.deps, fp, false);
    CHECK(run.commit(p, n, fp));
    D = run.tail();
    return n;
  }
  NodeId foreign_node() {  // anyone else's kernel: after the whole dependency set, then alone in it
    const NodeId n = add(D, Footprint{}, true);
    D = {n};
    return n;
  }
  bool reaches(NodeId from, NodeId to) const {  // `from` is ordered after `to`
    if (from == to) return true;
    std::vector<NodeId> todo{from};
    std::set<NodeId> seen;
    while (!todo.empty()) {
      const NodeId n = todo.back();
      todo.pop_back();
      for (NodeId d : nodes[idx(n)].deps) {
        if (d == to) return true;
        if (seen.insert(d).second) todo.push_back(d);
      }
    }
    return false;
  }
  std::set<NodeId> deps_of(NodeId n) const { return std::set<NodeId>(nodes[idx(n)].deps.begin(), nodes[idx(n)].deps.end()); }
};

static char g_mem[64 * 1024];
// a launch that reads buffer r and writes buffer w (4 KiB each)
static Footprint rw(int r, int w) {
  Footprint f;
  f.add(g_mem + 4096 * r, 4096, false);
  f.add(g_mem + 4096 * w, 4096, true);
  return f;
}
using S = std::set<NodeId>;

static void first_launch() {
  Stream s;
  const NodeId f = s.foreign_node();
  const NodeId a = s.launch(rw(0, 1));
  CHECK(s.last == kBroken);
  CHECK(s.deps_of(a) == S{f});
  CHECK(s.D == std::vector<NodeId>{a});
  Stream e;  // nothing captured yet
  const NodeId b = e.launch(rw(0, 1));
  CHECK(e.last == kBroken && e.deps_of(b).empty() && e.D == std::vector<NodeId>{b});
}

static void independent_pair() {
  Stream s;
  const NodeId f = s.foreign_node();
  const NodeId a = s.launch(rw(0, 1)), b = s.launch(rw(2, 3));
  CHECK(s.last == kRelaxed);
  CHECK(s.deps_of(b) == S{f});
  CHECK((S(s.D.begin(), s.D.end()) == S{a, b}));
  // two reads of one buffer are no hazard
  const NodeId c = s.launch(rw(0, 4));
  CHECK(s.last == kRelaxed && s.deps_of(c) == S{f});
}

static void hazards() {
  struct Case {
    const char* name;
    Footprint first, second;
  } cases[] = {{"RAW", rw(0, 1), rw(1, 2)}, {"WAR", rw(0, 1), rw(2, 0)}, {"WAW", rw(0, 1), rw(2, 1)}};
  for (Case& c : cases) {
    Stream s;
    s.foreign_node();
    const NodeId a = s.launch(c.first), b = s.launch(c.second);
    CHECK(s.last == kConflict);
    CHECK(s.deps_of(b) == S{a});
    CHECK(s.D == std::vector<NodeId>{b});
    // ranges that only meet at a boundary do not overlap
    Footprint next;
    next.add(g_mem + 4096 * 8, 4096, true);
    Footprint after;
    after.add(g_mem + 4096 * 9, 4096, true);
    Stream t;
    t.launch(next);
    t.launch(after);
    CHECK(t.last == kRelaxed);
  }
}

static void conflict_with_second_of_three() {
  Stream s;
  const NodeId f = s.foreign_node();
  const NodeId a = s.launch(rw(0, 1)), b = s.launch(rw(2, 3)), c = s.launch(rw(4, 5));
  const NodeId d = s.launch(rw(3, 6));  // reads what b writes
  CHECK(s.last == kConflict);
  CHECK(s.deps_of(d) == S{b});
  CHECK((S(s.D.begin(), s.D.end()) == S{a, c, d}));
  CHECK(s.reaches(d, f));
  // b has left the tail through d: a launch that touches b's memory (and not d's own) must wait for d
  const NodeId e = s.launch(rw(7, 2));  // writes what b reads
  CHECK(s.last == kConflict);
  CHECK(s.deps_of(e) == S{d});
  CHECK(s.reaches(e, b));
}

static void full_window() {
  Stream s;
  const NodeId f = s.foreign_node();
  NodeId n[6];
  for (int i = 0; i < 4; ++i) {
    n[i] = s.launch(rw(2 * i, 2 * i + 1));
    CHECK(i == 0 ? s.last == kBroken : s.last == kRelaxed);
    CHECK(s.deps_of(n[i]) == S{f});
  }
  n[4] = s.launch(rw(8, 9));
  CHECK(s.last == kWindow);
  CHECK(s.deps_of(n[4]) == S{n[0]});  // the first, and nothing else beyond the base (which n[0] carries)
  CHECK(s.reaches(n[4], f));
  CHECK((S(s.D.begin(), s.D.end()) == S{n[1], n[2], n[3], n[4]}));
  n[5] = s.launch(rw(10, 11));
  CHECK(s.last == kWindow && s.deps_of(n[5]) == S{n[1]});
  CHECK(s.D.size() == 4);
  // a long run: the entries' footprints are bounded (a launch that would outgrow the bound waits for the whole tail), the
  // window holds, the first launch stays ordered before a late one that touches its memory, and everything reaches the tail
  Stream l;
  l.window = 2;
  const NodeId first = l.launch(rw(0, 1));
  int joins = 0;
  for (int i = 0; i < 400; ++i) {
    Footprint f;  // all read buffer 2, each writes 64 bytes of its own
    f.add(g_mem + 4096 * 2, 4096, false);
    f.add(g_mem + 4096 * 4 + 64 * i, 64, true);
    const NodeId n = l.launch(f);
    joins += l.deps_of(n).size() == 2;
    CHECK(l.D.size() <= 2);
  }
  CHECK(joins >= 1);
  const NodeId late = l.launch(rw(1, 15));  // reads what the first launch wrote
  CHECK(l.reaches(late, first));
  for (size_t i = 0; i < l.nodes.size(); ++i) {
    bool seen = false;
    for (NodeId d : l.D) seen = seen || l.reaches(d, 100 + i);
    CHECK(seen);
  }
}

static void foreign_dependency_set() {
  Stream s;
  const NodeId a = s.launch(rw(0, 1)), b = s.launch(rw(2, 3));
  const NodeId f = s.foreign_node();
  CHECK((s.deps_of(f) == S{a, b}));
  const NodeId c = s.launch(rw(4, 5));
  CHECK(s.last == kBroken && s.deps_of(c) == S{f});
  const NodeId d = s.launch(rw(6, 7));
  CHECK(s.last == kRelaxed && s.deps_of(d) == S{f});
  // an event wait adds a node to the set without removing the tail: not exactly the tail either
  const NodeId other = s.add({}, Footprint{}, true);
  s.D.push_back(other);
  const NodeId e = s.launch(rw(8, 9));
  CHECK(s.last == kBroken);
  CHECK((s.deps_of(e) == S{c, d, other}));
  // a subset of the tail (the caller dropped a dependency) is not the tail
  const NodeId g = s.launch(rw(10, 11));
  CHECK(s.last == kRelaxed);
  s.D = {g};
  const NodeId h = s.launch(rw(12, 13));
  CHECK(s.last == kBroken && s.deps_of(h) == S{g});
}

static void changed_capture_id() {
  Stream s;
  const NodeId a = s.launch(rw(0, 1));
  s.launch(rw(2, 3));
  // another capture reuses the node handles of the first one: its first launch must not be taken for a continuation
  s.capture_id = 2;
  s.D = {a};
  const NodeId c = s.launch(rw(4, 5));
  CHECK(s.last == kBroken && s.deps_of(c) == S{a});
  // more captures than the planner keeps runs for: the oldest run is forgotten, which only costs a broken run
  Planner p;
  for (uint64_t id = 1; id <= 9; ++id) {
    Run& r = p.run(id);
    Plan pl = r.plan(nullptr, 0, rw(0, 1), 4);
    CHECK(pl.kind == kBroken && r.commit(pl, 100 + id, rw(0, 1)));
  }
  const NodeId d1 = 101;
  CHECK(p.run(1).plan(&d1, 1, rw(2, 3), 4).kind == kBroken);
  const NodeId d9 = 109;
  CHECK(p.run(9).plan(&d9, 1, rw(2, 3), 4).kind == kRelaxed);
  // a plan that is not the run's latest is not committed
  Run r;
  Plan p1 = r.plan(nullptr, 0, rw(0, 1), 4), p2 = r.plan(nullptr, 0, rw(0, 1), 4);
  CHECK(!r.commit(p1, 100, rw(0, 1)) && r.commit(p2, 101, rw(0, 1)) && r.tail() == std::vector<NodeId>{101});
}

static void window_of_one_is_a_chain() {
  static_assert(kDefaultWindow >= 1 && kDefaultWindow <= kMaxWindow, "the default window is one the planner takes");
  Stream s;
  s.window = 1;
  NodeId prev = s.foreign_node();
  for (int i = 0; i < 6; ++i) {
    const NodeId n = s.launch(rw(2 * i, 2 * i + 1));
    CHECK(s.deps_of(n) == S{prev});
    CHECK(s.last != kRelaxed);
    CHECK(s.D == std::vector<NodeId>{n});
    prev = n;
  }
}

// a run relaxes nothing until it holds min_run launches: until then the graph is the one stream order gives
static void short_runs_stay_chained() {
  static_assert(kDefaultMinRun >= 1, "the default run length is one the planner takes");
  Stream s;
  s.window = 2;
  s.min_run = 3;
  NodeId prev = s.foreign_node();
  for (int round = 0; round < 2; ++round) {
    for (int i = 0; i < 3; ++i) {  // q / k / v: independent, and never three launches before them
      const NodeId n = s.launch(rw(0, 1 + i));
      CHECK(s.deps_of(n) == S{prev});
      CHECK(s.last != kRelaxed);
      prev = n;
    }
    prev = s.foreign_node();
  }
  // a longer run: the fourth launch is the first one relaxed, and it still answers to the base
  const NodeId base = prev;
  NodeId n[6];
  for (int i = 0; i < 6; ++i) n[i] = s.launch(rw(0, 1 + i));
  CHECK(s.deps_of(n[1]) == S{n[0]} && s.deps_of(n[2]) == S{n[1]});
  CHECK(s.deps_of(n[3]) == S{base});
  CHECK(s.deps_of(n[4]) == S{n[2]});  // window of 2: waits for the older of {n[2], n[3]}
  CHECK(s.deps_of(n[5]) == S{n[3]});
  // a launch that touches the memory of one inside the chained part waits for the entry that answers for it
  const NodeId late = s.launch(rw(1, 9));  // reads what n[0] wrote; n[0] left through n[1], n[2], n[4]
  CHECK(s.reaches(late, n[0]));
}

// 200 random sequences over 6 buffers against the brute-force statement of what the graph must guarantee
static void random_sequences() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&](uint32_t n) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)((rng >> 11) % n);
  };
  int relaxed = 0, launches = 0;
  for (int seq = 0; seq < 200; ++seq) {
    Stream s;
    s.window = 1 + (int)next(kMaxWindow);
    s.min_run = 1 + (int)next(4);
    const int len = 5 + (int)next(40);
    for (int i = 0; i < len; ++i) {
      const uint32_t what = next(12);
      if (what == 0) {
        s.foreign_node();
        continue;
      }
      Footprint f;
      const int nr = 1 + (int)next(3);
      for (int k = 0; k < nr; ++k) f.add(g_mem + 4096 * next(6) + 512 * next(4), 512 + 512 * next(6), next(3) == 0);
      s.launch(f);
      ++launches;
      relaxed += s.last == kRelaxed;
      CHECK((int)s.D.size() <= s.window);
    }
    // every pair with a hazard (a foreign node: with everything) is connected by a path ...
    for (size_t j = 0; j < s.nodes.size(); ++j)
      for (size_t i = 0; i < j; ++i)
        if (s.nodes[i].foreign || s.nodes[j].foreign || hazard(s.nodes[i].fp, s.nodes[j].fp)) CHECK(s.reaches(100 + j, 100 + i));
    // ... and whatever is captured next waits for every launch: each one reaches the final dependency set
    for (size_t i = 0; i < s.nodes.size(); ++i) {
      bool seen = false;
      for (NodeId d : s.D) seen = seen || s.reaches(d, 100 + i);
      CHECK(seen);
    }
  }
  printf("  %d launches, %d relaxed\n", launches, relaxed);
  CHECK(relaxed > launches / 10);
}

int main() {
  struct {
    const char* name;
    void (*fn)();
  } cases[] = {{"first launch", first_launch},
               {"independent pair", independent_pair},
               {"RAW / WAR / WAW", hazards},
               {"conflict with the second of three", conflict_with_second_of_three},
               {"full window", full_window},
               {"foreign dependency set", foreign_dependency_set},
               {"changed capture id", changed_capture_id},
               {"window of one", window_of_one_is_a_chain},
               {"short runs stay chained", short_runs_stay_chained},
               {"random sequences", random_sequences}};
  for (auto& c : cases) {
    const int before = g_failed;
    c.fn();
    printf("%s: %s\n", c.name, g_failed == before ? "ok" : "FAILED");
  }
  return g_failed ? 1 : 0;
}

// Stand-alone check of the grouped launches of aqlm_amd/csrc/capture_overlap.h (built and run by tests/test_capture_merge_host.py
// with the address and undefined-behaviour sanitizers).  A model of a stream under capture whose library nodes hold SETS of
// launches: a launch either adds a node or joins one, as the planner says.  Random sequences are checked against the brute-force
// statement of what the graph must guarantee; with merge_max = 1 the planner must answer exactly like the rule it had before
// launches could share nodes, which is restated here (Before) and driven in lockstep.  Exit status 0 = all passed.
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../aqlm_amd/csrc/capture_overlap.h"

using namespace aqlm::capture_overlap;

static int g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                \
    }                                                            \
  } while (0)

// The planner before grouped launches: steps 1 to 3 of capture_overlap.h, one launch per node.
struct Before {
  struct Entry {
    NodeId node;
    Footprint fp;
  };
  std::vector<NodeId> base;
  std::vector<Entry> tail;
  size_t length = 0;
  // -> the dependencies of the launch; `node` is the id it gets
  std::vector<NodeId> launch(const std::vector<NodeId>& D, const Footprint& fp, int window, int min_run, NodeId node, Kind& kind) {
    std::set<NodeId> t, d(D.begin(), D.end());
    for (const Entry& e : tail) t.insert(e.node);
    std::vector<NodeId> deps;
    std::vector<size_t> leave;
    bool restart = false;
    if (tail.empty() || d != t || D.size() != tail.size()) {
      kind = kBroken;
      restart = true;
      deps = D;
    } else {
      for (size_t i = 0; i < tail.size(); ++i)
        if (hazard(tail[i].fp, fp)) leave.push_back(i);
      if (!leave.empty()) {
        kind = kConflict;
      } else if (length < (size_t)min_run) {
        kind = kWindow;
        for (size_t i = 0; i < tail.size(); ++i) leave.push_back(i);
      } else if ((int)tail.size() >= window) {
        kind = kWindow;
        leave.push_back(0);
      } else {
        kind = kRelaxed;
        deps = base;
      }
      size_t ranges = fp.ranges.size();
      for (size_t i : leave) ranges += tail[i].fp.ranges.size();
      if (kind != kRelaxed && ranges > kMaxRanges) {
        restart = true;
        leave.clear();
        deps = D;
      } else {
        for (size_t i : leave) deps.push_back(tail[i].node);
      }
    }
    Footprint mine = fp;
    if (restart) {
      base = deps;
      tail.clear();
      length = 0;
    } else {
      for (size_t k = leave.size(); k-- > 0;) {
        const Footprint& gone = tail[leave[k]].fp;
        mine.ranges.insert(mine.ranges.end(), gone.ranges.begin(), gone.ranges.end());
        tail.erase(tail.begin() + (ptrdiff_t)leave[k]);
      }
    }
    ++length;
    tail.push_back(Entry{node, mine});
    return deps;
  }
};

struct Launch {
  Footprint fp;
  uint64_t key;
  size_t node;  // index of the node that runs it
};
struct Node {
  std::vector<NodeId> deps;
  std::vector<uint32_t> members;  // launches (empty: a foreign node)
};

struct Stream {
  uint64_t capture_id = 1;
  std::vector<Node> nodes;  // ids 100, 101, ...
  std::vector<Launch> launches;
  std::vector<NodeId> D;
  Planner planner;
  int window = 2, min_run = 1, merge_max = 4;
  int refuse_every = 0;  // every n-th join is refused by the "runtime": the launch side plans again without merging
  uint64_t seen = 0, kinds[4] = {0, 0, 0, 0}, merged = 0, refused = 0, joins_tried = 0;
  Plan last;

  static size_t idx(NodeId n) { return (size_t)(n - 100); }
  void launch(const Footprint& fp, uint64_t key) {
    Run& run = planner.run(capture_id);
    const uint32_t me = (uint32_t)launches.size();
    ++seen;
    Plan p = run.plan(D.data(), D.size(), fp, window, min_run, key, merge_max);
    if (p.merge && refuse_every && ++joins_tried % refuse_every == 0) {
      ++refused;
      p = run.plan(D.data(), D.size(), fp, window, min_run, key, 1);
      CHECK(!p.merge);
    }
    last = p;
    ++kinds[p.kind];
    if (p.merge) {
      ++merged;
      CHECK(p.kind == kWindow && p.deps.empty() && p.leave.empty() && !p.restart);
      Node& n = nodes[idx(p.target)];
      CHECK(p.member == (int)n.members.size() && p.member >= 1);
      // the payload is what the node's launches left, in order
      CHECK(p.payload.size() == n.members.size() * sizeof(uint32_t) &&
            (n.members.empty() || !memcmp(p.payload.data(), n.members.data(), p.payload.size())));
      n.members.push_back(me);
      launches.push_back(Launch{fp, key, idx(p.target)});
      const std::vector<NodeId> before = run.tail();
      CHECK(run.commit(p, p.target, fp, &me, sizeof me));
      const std::vector<NodeId> after = run.tail();
      CHECK(std::set<NodeId>(before.begin(), before.end()) == std::set<NodeId>(after.begin(), after.end()));
      CHECK(!after.empty() && after.back() == p.target);  // the youngest now
    } else {
      nodes.push_back(Node{p.deps, {me}});
      launches.push_back(Launch{fp, key, nodes.size() - 1});
      CHECK(run.commit(p, 100 + nodes.size() - 1, fp, &me, sizeof me));
    }
    D = run.tail();
  }
  void foreign_node() {
    nodes.push_back(Node{D, {}});
    D = {100 + nodes.size() - 1};
  }
  bool reaches(size_t from, size_t to) const {  // node `from` is ordered after node `to`
    std::vector<size_t> todo{from};
    std::set<size_t> seen_;
    while (!todo.empty()) {
      const size_t n = todo.back();
      todo.pop_back();
      for (NodeId d : nodes[n].deps) {
        if (idx(d) == to) return true;
        if (seen_.insert(idx(d)).second) todo.push_back(idx(d));
      }
    }
    return false;
  }
  // what every graph must guarantee
  void verify() const {
    for (const Node& n : nodes) {
      CHECK((int)n.members.size() <= std::max(merge_max, 1));
      for (size_t a = 0; a < n.members.size(); ++a) {
        CHECK(launches[n.members[a]].key == launches[n.members[0]].key);  // one key per node
        CHECK(n.members.size() == 1 || launches[n.members[a]].key != 0);
        for (size_t b = 0; b < a; ++b) CHECK(!hazard(launches[n.members[a]].fp, launches[n.members[b]].fp));
      }
    }
    // every pair with a hazard is ordered as issued ...
    for (size_t j = 0; j < launches.size(); ++j)
      for (size_t i = 0; i < j; ++i)
        if (hazard(launches[i].fp, launches[j].fp)) CHECK(launches[i].node != launches[j].node && reaches(launches[j].node, launches[i].node));
    // ... a foreign node with everything around it: issue order of nodes is creation order, except that a launch may have
    // joined an OLDER node -- never across a foreign node
    for (size_t f = 0; f < nodes.size(); ++f) {
      if (!nodes[f].members.empty()) continue;
      for (size_t n = 0; n < nodes.size(); ++n) {
        if (n < f) CHECK(reaches(f, n));
        if (n > f) CHECK(reaches(n, f));
      }
    }
    // ... and whatever is captured next waits for every node
    for (size_t n = 0; n < nodes.size(); ++n) {
      bool ok = false;
      for (NodeId d : D) ok = ok || idx(d) == n || reaches(idx(d), n);
      CHECK(ok);
    }
    uint64_t member_count = 0, lib_nodes = 0;
    for (const Node& n : nodes) {
      member_count += n.members.size();
      lib_nodes += !n.members.empty();
    }
    CHECK(member_count == seen);
    CHECK(seen == kinds[kBroken] + kinds[kRelaxed] + kinds[kConflict] + kinds[kWindow]);
    CHECK(merged <= kinds[kWindow]);
    CHECK(lib_nodes == seen - merged);
  }
};

static char g_mem[64 * 1024];
static Footprint rw(int r, int w) {
  Footprint f;
  f.add(g_mem + 4096 * r, 4096, false);
  f.add(g_mem + 4096 * w, 4096, true);
  return f;
}

// two shapes alternating, as a stack of decoder blocks issues them: two chains of groups, never a mixed node
static void alternating_shapes() {
  for (int merge = 1; merge <= 4; ++merge) {
    Stream s;
    s.window = 2;
    s.merge_max = merge;
    for (int i = 0; i < 32; ++i) s.launch(rw(15, i % 8), 1 + (uint64_t)(i % 2));  // (writes clash 8 launches apart)
    s.verify();
  }
  Stream s;
  s.window = 2;
  s.merge_max = 4;
  Footprint f[16];
  for (int i = 0; i < 16; ++i) {
    f[i].add(g_mem, 4096, false);
    f[i].add(g_mem + 4096 + 64 * i, 64, true);
    s.launch(f[i], 1 + (uint64_t)(i % 2));
  }
  s.verify();
  // A0 B0 | A1..A3, B1..B3 join | A4 B4 start groups that wait for the full ones | ...
  CHECK(s.nodes.size() == 4 && s.merged == 12);
  for (const Node& n : s.nodes) CHECK(n.members.size() == 4);
  CHECK(s.nodes[2].deps == std::vector<NodeId>{100} && s.nodes[3].deps == std::vector<NodeId>{101});
}

static void window_of_one() {
  Stream s;
  s.window = 1;
  s.merge_max = 3;
  for (int i = 0; i < 7; ++i) {
    Footprint f;
    f.add(g_mem + 64 * i, 64, true);
    s.launch(f, 5);
  }
  s.verify();
  CHECK(s.nodes.size() == 3);  // 3 + 3 + 1: a chain of groups, no branches
  CHECK(s.nodes[1].deps == std::vector<NodeId>{100} && s.nodes[2].deps == std::vector<NodeId>{101});
  CHECK(s.kinds[kRelaxed] == 0);
}

static void hazards_and_keys() {
  Stream s;
  s.window = 1;
  s.merge_max = 4;
  s.launch(rw(0, 1), 7);
  s.launch(rw(1, 2), 7);  // reads what the first writes: its own node, after it
  CHECK(!s.last.merge && s.last.kind == kConflict && s.nodes.size() == 2);
  s.launch(rw(3, 4), 7);  // joins the second
  CHECK(s.last.merge && s.last.target == 101);
  s.launch(rw(5, 6), 8);  // another key
  CHECK(!s.last.merge && s.nodes.size() == 3);
  s.launch(rw(5, 7), 0);  // not eligible
  CHECK(!s.last.merge && s.nodes.size() == 4);
  s.launch(rw(5, 8), 0);  // nothing joins a node without a key
  CHECK(!s.last.merge && s.nodes.size() == 5);
  s.foreign_node();
  s.launch(rw(9, 10), 7);  // a broken run: nothing from before it is joined
  CHECK(!s.last.merge && s.last.kind == kBroken);
  s.launch(rw(9, 11), 7);
  CHECK(s.last.merge && s.last.target == 100 + s.nodes.size() - 1);
  // a launch that touches the memory of a JOINED launch waits for the node
  s.launch(rw(11, 12), 7);
  CHECK(!s.last.merge && s.last.kind == kConflict);
  s.verify();
  // short runs: nothing joins before the run holds min_run launches
  Stream t;
  t.window = 2;
  t.min_run = 4;
  for (int i = 0; i < 4; ++i) {
    t.launch(rw(0, 1 + i), 7);
    CHECK(!t.last.merge);
  }
  t.verify();
  CHECK(t.nodes.size() == 4);
  // a footprint that would outgrow the bound: no join, the launch waits for the whole tail
  Stream u;
  u.window = 1;
  u.merge_max = 4;
  Footprint big;
  for (size_t i = 0; i < kMaxRanges - 1; ++i) big.add(g_mem + 8 * i, 4, true);
  u.launch(big, 7);
  u.launch(rw(9, 10), 7);
  CHECK(!u.last.merge && u.last.restart && u.nodes[1].deps == std::vector<NodeId>{100});
  u.verify();
}

static void random_sequences() {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&](uint32_t n) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)((rng >> 11) % n);
  };
  uint64_t launches = 0, merged = 0, refused = 0;
  for (int seq = 0; seq < 400; ++seq) {
    Stream s;
    s.window = 1 + (int)next(4);
    s.merge_max = 1 + (int)next(4);
    s.min_run = 1 + (int)next(3);
    s.refuse_every = seq % 4 == 3 ? 1 + (int)next(3) : 0;
    const uint32_t nbuf = 6 + next(20), nkeys = 1 + next(3);
    Before before;
    const int len = 5 + (int)next(60);
    for (int i = 0; i < len; ++i) {
      if (next(16) == 0) {
        s.foreign_node();
        continue;
      }
      Footprint f;
      const int nr = 1 + (int)next(3);
      for (int k = 0; k < nr; ++k) f.add(g_mem + 2048 * next(nbuf) + 512 * next(4), 512 + 512 * next(3), next(3) == 0);
      const std::vector<NodeId> D = s.D;
      s.launch(f, next(5) == 0 ? 0 : 1 + next(nkeys));
      CHECK((int)s.D.size() <= s.window);  // never more than `window` nodes that nothing waits for
      if (s.merge_max == 1) {              // node for node what the planner answered before
        Kind kind = kBroken;
        const std::vector<NodeId> deps = before.launch(D, f, s.window, s.min_run, 100 + s.nodes.size() - 1, kind);
        CHECK(!s.last.merge && kind == s.last.kind && deps == s.nodes.back().deps);
        std::vector<NodeId> tail;
        for (const Before::Entry& e : before.tail) tail.push_back(e.node);
        CHECK(tail == s.D);
      }
    }
    s.verify();
    launches += s.seen;
    merged += s.merged;
    refused += s.refused;
  }
  printf("  %llu launches, %llu joined a node, %llu joins refused\n", (unsigned long long)launches, (unsigned long long)merged,
         (unsigned long long)refused);
  CHECK(merged > launches / 20 && refused > 0);
}

int main() {
  struct {
    const char* name;
    void (*fn)();
  } cases[] = {{"alternating shapes", alternating_shapes},
               {"window of one", window_of_one},
               {"hazards, keys and broken runs", hazards_and_keys},
               {"random sequences", random_sequences}};
  for (auto& c : cases) {
    const int before = g_failed;
    c.fn();
    printf("%s: %s\n", c.name, g_failed == before ? "ok" : "FAILED");
  }
  return g_failed ? 1 : 0;
}

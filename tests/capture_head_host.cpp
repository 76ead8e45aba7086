// Stand-alone check of "Regrouping the head" in aqlm_amd/csrc/capture_overlap.h (built and run by tests/test_capture_head_host.py
// with the address and undefined-behaviour sanitizers).  A model of a stream under capture: a DAG whose library nodes hold
// member lists.  Launches are planned and committed as the launch side does it; when the planner hands out an edit script, the
// script is applied step by step and EVERY prefix is checked against the brute-force statement of what the graph must
// guarantee.  Exit status 0 = all passed.
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

struct Launch {
  Footprint fp;
  uint64_t key;
};
struct Node {
  std::vector<NodeId> deps;
  std::vector<uint32_t> members;  // launches (empty: a foreign node)
  bool alive = true;
  bool operator==(const Node& o) const { return deps == o.deps && members == o.members && alive == o.alive; }
};
struct PlanSeen {  // what a launch was told
  Kind kind;
  std::vector<NodeId> deps;
  bool merge;
  NodeId target;
  bool operator==(const PlanSeen& o) const { return kind == o.kind && deps == o.deps && merge == o.merge && target == o.target; }
};

struct Stream {
  uint64_t capture_id = 1;
  std::vector<Node> nodes;  // ids 100, 101, ...
  std::vector<Launch> launches;
  std::vector<NodeId> D;
  Planner planner;
  int window = 2, min_run = 8, merge_max = 4;
  bool head_on = true;
  long stop_at = -1;  // the first script stops after this many steps (the "runtime" refused the next one)
  bool stopped = false;
  std::vector<PlanSeen> plans;
  uint64_t scripts = 0, empty_scripts = 0, moved = 0, regroup_calls = 0;
  size_t last_script_steps = 0;
  // the run that is being captured, for the head's checks
  size_t run_first_node = 0, run_first_launch = 0;
  std::vector<NodeId> run_base;

  static size_t idx(NodeId n) { return (size_t)(n - 100); }
  bool reaches(size_t from, size_t to) const {  // node `from` is ordered after node `to`
    std::vector<size_t> todo{from};
    std::set<size_t> seen;
    while (!todo.empty()) {
      const size_t n = todo.back();
      todo.pop_back();
      for (NodeId d : nodes[n].deps) {
        if (idx(d) == to) return true;
        if (seen.insert(idx(d)).second) todo.push_back(idx(d));
      }
    }
    return false;
  }
  std::vector<size_t> copies(uint32_t launch) const {
    std::vector<size_t> c;
    for (size_t n = 0; n < nodes.size(); ++n)
      if (nodes[n].alive)
        for (uint32_t m : nodes[n].members)
          if (m == launch) c.push_back(n);
    return c;
  }
  // what every graph must guarantee, also between two steps of a script; `exactly_once`: no launch runs twice
  void verify_graph(bool exactly_once) const {
    for (const Node& n : nodes) {
      if (!n.alive) continue;
      for (NodeId d : n.deps) CHECK(nodes[idx(d)].alive);  // nothing waits for a node that is gone
      CHECK((int)n.members.size() <= std::max(merge_max, 1));
      for (size_t a = 0; a < n.members.size(); ++a) {
        CHECK(launches[n.members[a]].key == launches[n.members[0]].key);  // one key per node
        CHECK(n.members.size() == 1 || launches[n.members[a]].key != 0);
        for (size_t b = 0; b < a; ++b) CHECK(!hazard(launches[n.members[a]].fp, launches[n.members[b]].fp));
      }
    }
    for (uint32_t l = 0; l < launches.size(); ++l) {
      const size_t c = copies(l).size();
      CHECK(c >= 1);
      if (exactly_once) CHECK(c == 1);
    }
    // every pair with a hazard is ordered as issued, in all of their copies
    for (uint32_t j = 0; j < launches.size(); ++j)
      for (uint32_t i = 0; i < j; ++i)
        if (hazard(launches[i].fp, launches[j].fp))
          for (size_t a : copies(i))
            for (size_t b : copies(j)) CHECK(a != b && reaches(b, a));
    // a foreign node is ordered with everything around it (issue order of nodes is creation order; a launch may sit in an OLDER
    // node of its run, never across a foreign node)
    for (size_t f = 0; f < nodes.size(); ++f) {
      if (!nodes[f].members.empty()) continue;
      for (size_t n = 0; n < nodes.size(); ++n) {
        if (!nodes[n].alive) continue;
        if (n < f) CHECK(reaches(f, n));
        if (n > f) CHECK(reaches(n, f));
      }
    }
  }
  // ... and whatever is captured next waits for every node
  void verify_stream() const {
    for (size_t n = 0; n < nodes.size(); ++n) {
      if (!nodes[n].alive) continue;
      bool ok = false;
      for (NodeId d : D) ok = ok || idx(d) == n || reaches(idx(d), n);
      CHECK(ok);
    }
    for (NodeId d : D) CHECK(nodes[idx(d)].alive);
  }
  // the run's first `count` launches are one path from the run's base: every node of theirs that is left waits for the one before
  void verify_head_path(size_t head_nodes) const {
    NodeId prev = 0;
    bool first = true;
    for (size_t n = run_first_node; n < run_first_node + head_nodes; ++n) {
      if (!nodes[n].alive) continue;
      if (first) CHECK(nodes[n].deps == run_base);
      else CHECK(nodes[n].deps == std::vector<NodeId>{prev});
      first = false;
      prev = 100 + n;
    }
    CHECK(!first);
  }

  void apply(const HeadScript& script, Run& run) {
    const size_t n_head = (size_t)min_run;
    CHECK(nodes.size() == run_first_node + n_head && launches.size() == run_first_launch + n_head);
    const std::vector<Node> before(nodes.begin(), nodes.begin() + (ptrdiff_t)run_first_node);
    const long stop = stopped ? -1 : stop_at;
    size_t done = 0, destroyed = 0;
    last_script_steps = script.steps.size();
    for (const HeadStep& st : script.steps) {
      if (stop >= 0 && (long)done == stop) break;
      CHECK(idx(st.node) >= run_first_node && idx(st.node) < nodes.size());  // nothing before the run is named
      Node& n = nodes[idx(st.node)];
      if (st.op == HeadStep::kRewrite) {
        CHECK(destroyed == 0 && n.alive);  // rewrites first
        CHECK(st.payload.size() == st.members.size() * sizeof(uint32_t) && !st.members.empty());
        std::vector<uint32_t> m(st.members.size());
        memcpy(m.data(), st.payload.data(), std::min(st.payload.size(), m.size() * sizeof(uint32_t)));
        for (size_t k = 0; k < m.size(); ++k) {
          CHECK(m[k] == run_first_launch + st.members[k]);  // the payloads are those of the members, in issue order
          CHECK(k == 0 || st.members[k] > st.members[k - 1]);
          CHECK(launches[m[k]].key == st.key);
        }
        CHECK(m != n.members);  // only nodes whose content changes
        n.members = m;
      } else if (st.op == HeadStep::kSetStreamDeps) {
        CHECK(n.alive);
        D = {st.node};
      } else {
        CHECK(n.alive);
        for (const Node& o : nodes)
          if (o.alive)
            for (NodeId d : o.deps) CHECK(d != st.node);  // nothing depends on it
        for (NodeId d : D) CHECK(d != st.node);          // nor does the stream
        n.alive = false;
        ++destroyed;
      }
      ++done;
      // every prefix of the script is a correct graph
      verify_graph(false);
      verify_head_path(n_head);
      CHECK(std::vector<Node>(nodes.begin(), nodes.begin() + (ptrdiff_t)run_first_node) == before);
    }
    run.head_applied(done);
    D = run.tail();  // what the launch side installs last
    if (done == script.steps.size()) {
      moved += script.moved;
      CHECK(destroyed == script.moved);
      verify_graph(!stopped);  // every launch exactly once (unless an earlier script of this stream stopped)
      // the planner's tail is the chain's last node
      size_t last = 0;
      for (size_t n = run_first_node; n < nodes.size(); ++n)
        if (nodes[n].alive) last = n;
      CHECK(D == std::vector<NodeId>{100 + last});
      CHECK(last == run_first_node + script.groups - 1);
      // an independent launch next: relaxed on the run's base (a window of one has no room beside the tail)
      Footprint free_fp;
      static char elsewhere[64];
      free_fp.add(elsewhere, 64, true);
      const Plan p = run.plan(D.data(), D.size(), free_fp, window, min_run, 0, merge_max);
      if (window >= 2) CHECK(p.kind == kRelaxed && p.deps == run_base && !p.merge);
      else CHECK(p.kind == kWindow && !p.restart);
    } else {
      stopped = true;
      CHECK(D.size() == 1 && nodes[idx(D[0])].alive);
    }
    verify_stream();
  }

  void launch(const Footprint& fp, uint64_t key, bool with_payload = true) {
    Run& run = planner.run(capture_id);
    const uint32_t me = (uint32_t)launches.size();
    Plan p = run.plan(D.data(), D.size(), fp, window, min_run, key, merge_max);
    plans.push_back(PlanSeen{p.kind, p.deps, p.merge, p.target});
    launches.push_back(Launch{fp, key});
    if (p.merge) {
      Node& n = nodes[idx(p.target)];
      CHECK(n.alive && p.member == (int)n.members.size());
      CHECK(p.payload.size() == n.members.size() * sizeof(uint32_t) && !memcmp(p.payload.data(), n.members.data(), p.payload.size()));
      n.members.push_back(me);
      CHECK(run.commit(p, p.target, fp, &me, sizeof me));
    } else {
      if (p.restart) {
        run_first_node = nodes.size();
        run_first_launch = me;
        run_base = p.deps;
      }
      nodes.push_back(Node{p.deps, {me}, true});
      CHECK(run.commit(p, 100 + nodes.size() - 1, fp, with_payload ? &me : nullptr, with_payload ? sizeof me : 0));
    }
    D = run.tail();
    if (head_on && p.head && !p.merge) {
      ++regroup_calls;
      const HeadScript script = run.regroup_head(min_run, merge_max);
      if (script.empty()) {
        ++empty_scripts;
        CHECK(run.tail() == D);
      } else {
        ++scripts;
        apply(script, run);
      }
    }
  }
  void foreign_node() {
    nodes.push_back(Node{D, {}, true});
    D = {100 + nodes.size() - 1};
  }
  size_t alive_nodes() const {
    size_t a = 0;
    for (const Node& n : nodes) a += n.alive;
    return a;
  }
};

static char g_mem[64 * 1024];
static Footprint own(int i) {  // reads a shared input, writes a place of its own
  Footprint f;
  f.add(g_mem, 1024, false);
  f.add(g_mem + 4096 + 64 * i, 64, true);
  return f;
}

// the decode step's head: two shapes alternating, min_run 8, merge 4
static void alternating_head() {
  Stream s;
  for (int i = 0; i < 8; ++i) s.launch(own(i), 1 + (uint64_t)(i % 2));
  CHECK(s.scripts == 1 && s.moved == 6 && s.alive_nodes() == 2);
  CHECK(s.last_script_steps == 2 + 2 * 6);
  CHECK((s.nodes[0].members == std::vector<uint32_t>{0, 2, 4, 6}) && (s.nodes[1].members == std::vector<uint32_t>{1, 3, 5, 7}));
  CHECK(s.nodes[1].deps == std::vector<NodeId>{100} && s.D == std::vector<NodeId>{101});
  // launch 9 is the first relaxed one; launch 10 starts its chain behind the head
  s.launch(own(8), 1);
  CHECK(s.plans.back().kind == kRelaxed && s.plans.back().deps.empty());
  s.launch(own(9), 2);
  CHECK(s.plans.back().kind == kWindow && !s.plans.back().merge && s.plans.back().deps == std::vector<NodeId>{101});
  for (int i = 10; i < 24; ++i) s.launch(own(i), 1 + (uint64_t)(i % 2));
  s.verify_graph(true);
  s.verify_stream();
  CHECK(s.alive_nodes() == 6);
  // A B A B A B A A | A A: groups {0 2 4 6} {1 3 5} {7}; the last group has room and the next launch of its key joins it
  Stream t;
  const int keys[10] = {1, 2, 1, 2, 1, 2, 1, 1, 1, 1};
  for (int i = 0; i < 8; ++i) t.launch(own(i), (uint64_t)keys[i]);
  CHECK(t.scripts == 1 && t.moved == 5 && t.alive_nodes() == 3);
  CHECK((t.nodes[2].members == std::vector<uint32_t>{7}) && t.D == std::vector<NodeId>{102});
  t.launch(own(8), 1);
  CHECK(t.plans.back().kind == kRelaxed);
  t.launch(own(9), 1);
  CHECK(t.plans.back().kind == kWindow && t.plans.back().merge && t.plans.back().target == 102);
  t.verify_graph(true);
  t.verify_stream();
  // a window of one: regrouped, still a chain; later launches join the last group
  Stream u;
  u.window = 1;
  for (int i = 0; i < 12; ++i) u.launch(own(i), 1 + (uint64_t)(i % 2));
  CHECK(u.scripts == 1 && u.moved == 6);
  for (const PlanSeen& p : u.plans) CHECK(p.kind != kRelaxed);
  u.verify_graph(true);
  u.verify_stream();
  // min_run 3, three launches of one shape: one node of three
  Stream v;
  v.min_run = 3;
  for (int i = 0; i < 3; ++i) v.launch(own(i), 7);
  CHECK(v.scripts == 1 && v.moved == 2 && v.alive_nodes() == 1 && v.nodes[0].members.size() == 3);
}

// the head stays as issued, and every plan is the one a planner that is never asked gives
static void no_script() {
  struct Case {
    const char* what;
    int merge, conflict_at, keyless, on;
    bool distinct_keys;
  } cases[] = {{"a conflict in the head", 4, 5, 0, 1, false},   {"no two launches of a key", 4, -1, 0, 1, true},
               {"merge 1", 1, -1, 0, 1, false},                  {"the key off", 4, -1, 0, 0, false},
               {"keyless launches only", 4, -1, 1, 1, false}};
  for (const Case& c : cases) {
    Stream s, ref;
    s.merge_max = ref.merge_max = c.merge;
    s.head_on = c.on != 0;
    ref.head_on = false;
    for (int i = 0; i < 12; ++i) {
      Footprint f = own(i);
      if (i == c.conflict_at) f.add(g_mem + 4096 + 64 * 2, 64, false);  // reads what launch 2 wrote
      const uint64_t key = c.keyless ? 0 : (c.distinct_keys && i < 8 ? 10 + (uint64_t)i : 1 + (uint64_t)(i % 2));
      s.launch(f, key);
      ref.launch(f, key);
    }
    if (s.scripts != 0 || !(s.plans == ref.plans)) printf("  (%s)\n", c.what);
    CHECK(s.scripts == 0 && s.moved == 0);
    CHECK(s.plans == ref.plans && s.nodes == ref.nodes && s.D == ref.D);
    s.verify_graph(true);
    s.verify_stream();
  }
  // a launch that left no payload cannot be built in another node: no script when it would have to move ...
  Stream a;
  for (int i = 0; i < 8; ++i) a.launch(own(i), i == 5 ? 0 : 1, i != 5);
  CHECK(a.scripts == 0);
  // ... and it stays where it is when nothing before it moved
  Stream b;
  for (int i = 0; i < 8; ++i) b.launch(own(i), i == 0 ? 0 : 1, i != 0);
  CHECK(b.scripts == 1 && b.moved == 5 && (b.nodes[0].members == std::vector<uint32_t>{0}));
  // a keyless launch with a payload keeps a node to itself, the others regroup around it
  Stream c;
  for (int i = 0; i < 8; ++i) c.launch(own(i), i == 3 ? 0 : 1);
  CHECK(c.scripts == 1 && c.moved == 5 && (c.nodes[1].members == std::vector<uint32_t>{3}) && c.alive_nodes() == 3);
  // a run broken by a foreign node starts its head over
  Stream d;
  for (int i = 0; i < 5; ++i) d.launch(own(i), 1);
  d.foreign_node();
  for (int i = 5; i < 14; ++i) d.launch(own(i), 1);
  CHECK(d.scripts == 1 && d.moved == 6 && d.nodes[4].alive && d.nodes[4].members.size() == 1);
  d.verify_graph(true);
  d.verify_stream();
}

struct Rng {
  uint64_t s;
  uint32_t next(uint32_t n) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)((s >> 11) % n);
  }
};

// one random sequence; `stop_at` >= 0: its first script stops there.  -> the steps of the first script (0: there was none)
static size_t random_sequence(uint64_t seed, long stop_at, uint64_t& scripts, uint64_t& moved, uint64_t& calls) {
  Rng r{seed * 0x9E3779B97F4A7C15ull + 1};
  Stream s, ref;
  s.window = ref.window = 1 + (int)r.next(3);
  s.min_run = ref.min_run = 1 + (int)r.next(8);
  s.merge_max = ref.merge_max = 1 + (int)r.next(8);
  s.stop_at = stop_at;
  ref.head_on = false;
  const int len = 1 + (int)r.next(12);
  const uint32_t nkeys = 1 + r.next(3), npool = 6 + r.next(24);
  const int foreign_at = (int)r.next((uint32_t)len + 1);
  const uint32_t write_one_in = 2 + r.next(6);
  size_t first_steps = 0;
  for (int i = 0; i < len + 3; ++i) {  // (three more launches than drawn: after a stopped script the run goes on)
    if (i == foreign_at) {
      s.foreign_node();
      ref.foreign_node();
    }
    Footprint f;
    const int nr = 1 + (int)r.next(3);
    for (int k = 0; k < nr; ++k) f.add(g_mem + 1024 * r.next(npool), 512 + 512 * r.next(2), r.next(write_one_in) == 0);
    const uint64_t key = r.next(5) == 0 ? 0 : 1 + r.next(nkeys);
    const bool with_payload = key != 0 || r.next(2) != 0;  // (some keyless launches leave nothing to build them from)
    s.launch(f, key, with_payload);
    if (s.scripts == 1 && first_steps == 0) first_steps = s.last_script_steps;
    if (s.scripts == 0) {  // until a head is regrouped, the planner answers as if it were never asked
      ref.launch(f, key, with_payload);
      CHECK(s.plans == ref.plans && s.D == ref.D);
    }
    CHECK((int)s.D.size() <= s.window);
  }
  s.verify_graph(!s.stopped);  // (after a script that stopped, a launch may run twice)
  s.verify_stream();
  scripts += s.scripts;
  moved += s.moved;
  calls += s.regroup_calls;
  return first_steps;
}

static void random_sequences() {
  uint64_t scripts = 0, moved = 0, calls = 0;
  for (uint64_t seed = 1; seed <= 4000; ++seed) random_sequence(seed, -1, scripts, moved, calls);
  printf("  %llu launches asked, %llu scripts, %llu launches gave up their node\n", (unsigned long long)calls,
         (unsigned long long)scripts, (unsigned long long)moved);
  CHECK(scripts > 200 && moved > scripts);
}

static void stopped_scripts() {
  uint64_t scripts = 0, moved = 0, calls = 0, stops = 0;
  for (uint64_t seed = 1; seed <= 1500; ++seed) {
    uint64_t a = 0, b = 0, c = 0;
    const size_t steps = random_sequence(seed, -1, a, b, c);
    for (size_t stop = 0; stop < steps; ++stop, ++stops) random_sequence(seed, (long)stop, scripts, moved, calls);
  }
  printf("  %llu scripts stopped at every one of their steps\n", (unsigned long long)stops);
  CHECK(stops > 500);
  // the decode step's head stopped after the rewrites and one destroy: the tail is the newest node left, and nothing joins it
  Stream s;
  s.stop_at = 4;
  for (int i = 0; i < 12; ++i) s.launch(own(i), 1 + (uint64_t)(i % 2));
  CHECK(s.stopped && !s.nodes[7].alive && s.nodes[6].alive);
  CHECK(s.plans[8].kind == kRelaxed && !s.plans[9].merge && s.plans[9].deps == std::vector<NodeId>{106});
  s.verify_graph(false);
  s.verify_stream();
}

int main() {
  struct {
    const char* name;
    void (*fn)();
  } cases[] = {{"alternating head", alternating_head},
               {"no script", no_script},
               {"random sequences", random_sequences},
               {"stopped scripts", stopped_scripts}};
  for (auto& c : cases) {
    const int before = g_failed;
    c.fn();
    printf("%s: %s\n", c.name, g_failed == before ? "ok" : "FAILED");
  }
  return g_failed ? 1 : 0;
}

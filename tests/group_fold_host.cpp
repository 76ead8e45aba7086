// Host check of aqlm_amd/csrc/group_fold.h: where the workgroups of a folded grouped launch sit.  Stand-alone (its own main, no
// HIP), built with the address and undefined-behaviour sanitizers by tests/test_group_fold_host.py.
#include <stdio.h>

#include <vector>

#include "../aqlm_amd/csrc/group_fold.h"

namespace gf = aqlm::group_fold;

static int failures = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++failures;                 \
      printf("FAIL: " __VA_ARGS__); \
      printf("\n");               \
    }                             \
  } while (0)

int main() {
  for (int fold : {1, 2, 4}) {
    for (int nseg = 1; nseg <= 8; ++nseg) {
      const unsigned grid = gf::grid(nseg, fold);
      CHECK(grid == (unsigned)(nseg * gf::kStreams / fold), "grid of %d members at fold %d is %u", nseg, fold, grid);
      std::vector<int> visits((size_t)nseg * gf::kStreams, 0);
      for (unsigned block = 0; block < grid; ++block) {
        const gf::Place at = gf::place(block, fold);
        CHECK(at.segment >= 0 && at.segment < nseg, "block %u fold %d: segment %d of %d", block, fold, at.segment, nseg);
        CHECK(at.slice == (int)(block % 16u), "block %u fold %d: slice %d is not block %% 16", block, fold, at.slice);
        if (at.segment < 0 || at.segment >= nseg) continue;
        for (int pass = 0; pass < fold; ++pass) {
          const int st = gf::stream(at, pass);
          CHECK(st >= 0 && st < gf::kStreams, "block %u fold %d pass %d: stream %d", block, fold, pass, st);
          CHECK(st % gf::kSlices == at.slice, "block %u fold %d pass %d: stream %d leaves slice %d", block, fold, pass, st, at.slice);
          if (st >= 0 && st < gf::kStreams) ++visits[(size_t)at.segment * gf::kStreams + st];
        }
      }
      for (size_t i = 0; i < visits.size(); ++i)
        CHECK(visits[i] == 1, "fold %d, %d members: (segment %zu, stream %zu) visited %d times", fold, nseg, i / gf::kStreams,
              i % gf::kStreams, visits[i]);
    }
    printf("fold %d: %s\n", fold, failures ? "failed" : "ok");
  }
  // the rule that picks the factor: the key's value from that many members on, the unfolded kernel below and for any other value
  for (int members = 1; members <= 8; ++members) {
    CHECK(gf::choose(1, members) == 1, "key 1 folds %d members", members);
    CHECK(gf::choose(2, members) == (members >= 2 ? 2 : 1), "key 2 at %d members", members);
    CHECK(gf::choose(4, members) == (members >= 4 ? 4 : 1), "key 4 at %d members", members);
    CHECK(gf::choose(0, members) == gf::choose(gf::kDefaultFold, members), "key 0 is the default at %d members", members);
    CHECK(gf::choose(3, members) == 1 && gf::choose(8, members) == 1 && gf::choose(-1, members) == 1, "an unknown key value folds");
    CHECK(gf::grid(members, gf::choose(4, members)) >= (unsigned)gf::kStreams, "folded grid under 256 workgroups");
  }
  printf("choose: %s\n", failures ? "failed" : "ok");
  return failures ? 1 : 0;
}

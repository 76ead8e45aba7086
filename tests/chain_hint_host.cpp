// Host check of aqlm_amd/csrc/chain_hint.h: when aqlm_hip_gemv_1x16_packed_chain hands the next layer's entry stream to its prefetch
// waves.  Stand-alone (its own main, no HIP), built with the address and undefined-behaviour sanitizers by
// tests/test_chain_hint_host.py.
//
// The buffer layout is restated here from packed_format.h (as tests/packed_model.py restates it), and the requests are the loop of
// the prefetch waves in gemv_1x16_packed_body, walked literally for every workgroup and every wave count: whenever the hint is
// kept, no request may end behind used_bytes; and the hint is dropped only where one would.
#include <stdio.h>

#include <initializer_list>

#include "../aqlm_amd/csrc/chain_hint.h"

namespace ch = aqlm::chain_hint;

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      printf("FAIL: " __VA_ARGS__); \
      printf("\n");                 \
    }                               \
  } while (0)

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Layout {
  size_t off_ent, ent_bytes, used;
};

// format v7, 16 slices x 16 row groups, 8-element vectors (packed_layout)
static Layout layout(int out_features, int waves, int steps, int entry_bytes, bool relabel) {
  const size_t nst = 256, RG = ((size_t)out_features + 15) / 16;
  const size_t off_rowstart = up(256 + nst * 16 * 16, 256);
  const size_t off_acc = up(off_rowstart + nst * (RG + 1) * 4, 256);
  Layout L;
  L.off_ent = up(off_acc + (size_t)8 * out_features * 8, 1024);
  L.ent_bytes = nst * waves * steps * (entry_bytes == 3 ? (size_t)776 : (size_t)1024);
  const size_t off_cb = up(L.off_ent + L.ent_bytes, 1024) + (size_t)65536 * 2;
  L.used = relabel ? off_cb + (size_t)65536 * 16 : L.off_ent + L.ent_bytes;
  return L;
}

// first byte behind the last byte the prefetch waves of any workgroup ask for: the kernel's loop, 64 lanes x 16 bytes per request
static size_t walk(size_t off_ent, uint32_t block_bytes, int npw) {
  size_t end = 0;
  for (int block = 0; block < 256; ++block)
    for (int pw = 0; pw < npw; ++pw)
      for (uint32_t off = (uint32_t)pw * 1024u; off < block_bytes; off += (uint32_t)npw * 1024u) {
        const size_t last_lane = off_ent + (size_t)block * block_bytes + off + 63 * 16 + 16;
        if (last_lane > end) end = last_lane;
      }
  return end;
}

int main() {
  long kept = 0, dropped = 0, parent_over = 0, parent_over_other = 0;
  size_t worst = 0;
  for (int eb : {3, 4}) {
    for (int relabel = 0; relabel < 2; ++relabel) {
      const int before = failures;
      for (int out : {37, 512, 1000})
        for (int waves = 1; waves <= 16; ++waves)
          for (int steps = 1; steps <= 40; ++steps) {
            if (eb == 3 && steps > 32) continue;  // the 3-byte form exists up to 32 steps per wave
            const Layout L = layout(out, waves, steps, eb, relabel != 0);
            const ch::Hint h = ch::decide(L.off_ent, L.ent_bytes, 256, L.used, false);
            const uint32_t bb = (uint32_t)(L.ent_bytes / 256);
            bool fits = true;
            for (int npw = 1; npw <= 7; ++npw) {
              const size_t end = walk(L.off_ent, bb, npw);
              CHECK(end == ch::request_end(L.off_ent, bb, 255), "request_end: %d waves x %d steps, %d-byte entries, %d prefetch waves: "
                    "walked %zu, the header says %zu", waves, steps, eb, npw, end, ch::request_end(L.off_ent, bb, 255));
              if (end > L.used) {
                fits = false;
                if (end - L.used > worst) worst = end - L.used;
              }
              if (h.kept)
                CHECK(end <= L.used, "%d -> waves %d steps %d, %d-byte entries, relabelled %d, %d prefetch waves: the kept hint reads "
                      "%zu bytes past used_bytes", out, waves, steps, eb, relabel, npw, end - L.used);
            }
            CHECK(h.kept == fits, "waves %d steps %d, %d-byte entries, relabelled %d: hint %s although the requests %s", waves, steps, eb,
                  relabel, h.kept ? "kept" : "dropped", fits ? "stay inside the buffer" : "leave it");
            if (h.kept) {
              CHECK(h.ent_offset == L.off_ent && h.block_bytes == bb, "waves %d steps %d: hint (%zu, %u), layout (%zu, %u)", waves,
                    steps, h.ent_offset, h.block_bytes, L.off_ent, bb);
              ++kept;
            } else {
              ++dropped;
            }
            // the rule before this header existed: every uniform-geometry buffer kept its hint
            if (!fits) ++(eb == 3 && !relabel ? parent_over : parent_over_other);
            if (eb == 4 || relabel) CHECK(h.kept, "waves %d steps %d, %d-byte entries, relabelled %d: hint dropped", waves, steps, eb, relabel);
            if (eb == 3 && !relabel) CHECK(h.kept == (bb % 1024u == 0u), "waves %d steps %d: %u bytes per block, hint %s", waves, steps,
                                           bb, h.kept ? "kept" : "dropped");
          }
      printf("entry bytes %d relabelled %d: %s\n", eb, relabel, failures == before ? "ok" : "failed");
    }
  }
  {
    const int before = failures;
    // 4 waves x 1 step of 3-byte entries are 3104 bytes per block: the last request of the last block ends 992 bytes over
    const Layout L = layout(512, 4, 1, 3, false);
    CHECK(L.ent_bytes / 256 == 3104 && walk(L.off_ent, 3104, 2) == L.used + 992, "4 x 1 x 776: %zu bytes per block, %zu bytes over",
          L.ent_bytes / 256, walk(L.off_ent, 3104, 2) - L.used);
    CHECK(!ch::decide(L.off_ent, L.ent_bytes, 256, L.used, false).kept, "4 x 1 x 776 keeps its hint");
    // a sweep that could not tell the two rules apart would prove nothing: the old rule must be caught, and only where it was wrong
    CHECK(parent_over > 0 && parent_over_other == 0, "keeping every hint reads past the buffer in %ld 3-byte unrelabelled layouts and %ld others",
          parent_over, parent_over_other);
    CHECK(worst == 1024 - 8, "worst over-read %zu bytes", worst);  // 776 = 8 x 97: a stream is a multiple of 8 bytes (11 waves x 3 steps: 8 past a KiB)
    const Layout V = layout(512, 4, 2, 4, false);
    CHECK(!ch::decide(V.off_ent, V.ent_bytes, 256, V.used, true).kept, "variable geometry keeps its hint");
    CHECK(!ch::decide(V.off_ent, 0, 256, V.used, false).kept && !ch::decide(V.off_ent, V.ent_bytes, 0, V.used, false).kept, "an empty stream keeps its hint");
    printf("old rule: over the buffer in %ld layouts, by up to %zu bytes; hints kept %ld, dropped %ld\n", parent_over, worst, kept, dropped);
    printf("edges: %s\n", failures == before ? "ok" : "failed");
  }
  return failures ? 1 : 0;
}

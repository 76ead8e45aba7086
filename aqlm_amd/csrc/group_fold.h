// Folded grouped launches of the packed 1x16 matvec (gemv_1x16_packed_group_fold_kernel, packed_gemv_kernels.h): where a workgroup
// of the folded grid sits.  Plain C++ with no dependency on HIP, so that the kernel, the launch code and the host test
// (tests/group_fold_host.cpp) read one and the same function.
//
// An unfolded segment is 256 workgroups = 16 row groups x 16 slices, stream = group * 16 + slice, slice = block % 16.  Folded by
// F (1, 2, 4; F divides 16) a segment is 256 / F workgroups; workgroup b of it keeps slice b % 16 -- 256 / F is a multiple of
// 16, so the slice is still blockIdx.x % 16 and the XCD / L2 placement is what it was -- fills slice and x once and walks the
// row groups b / 16, b / 16 + 16 / F, ... in F passes.
#ifndef AQLM_GROUP_FOLD_H_
#define AQLM_GROUP_FOLD_H_

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQLM_FOLD_HD __host__ __device__
#else
#define AQLM_FOLD_HD
#endif

namespace aqlm {
namespace group_fold {

constexpr int kSlices = 16, kGroups = 16, kStreams = kSlices * kGroups;
// Measured on the 64-layer decode step at a capture window of 2 (profiles/group_fold.json; us per step, five alternations in one
// process), fold x packed_capture_merge:   merge 4      6      8
//                                 fold 1   342.9  330.6  335.5      (1 = the unfolded grouped kernel)
//                                 fold 2   327.3  310.0  307.1
//                                 fold 4   292.1  328.7  305.9
// Four passes in nodes of four: a node is exactly 256 workgroups, one LDS slot per CU and chain, and a slice is filled 4 times
// per layer instead of 16.  (Six members at four passes are 384 workgroups: one and a half rounds of the chip.)
constexpr int kDefaultFold = 4;  // tuning key packed_group_fold at 0

struct Place {
  int segment;      // which member of the node
  int slice;        // == block % 16
  int first_group;  // row group of pass 0
  int group_step;   // pass j walks row group first_group + j * group_step
};

AQLM_FOLD_HD inline bool valid(int fold) { return fold == 1 || fold == 2 || fold == 4; }
AQLM_FOLD_HD inline unsigned grid(int members, int fold) { return (unsigned)members * (unsigned)(kStreams / fold); }

AQLM_FOLD_HD inline Place place(unsigned block, int fold) {
  const unsigned shift = 8u - ((unsigned)fold >> 1);  // log2(256 / F) for F = 1, 2, 4: shifts, not a division in front of the first load
  const unsigned b = block & ((1u << shift) - 1u);
  Place q;
  q.segment = (int)(block >> shift);
  q.slice = (int)(b & (unsigned)(kSlices - 1));
  q.first_group = (int)(b >> 4);
  q.group_step = kGroups >> ((unsigned)fold >> 1);
  return q;
}
AQLM_FOLD_HD inline int stream(const Place& q, int pass) { return (q.first_group + pass * q.group_step) * kSlices + q.slice; }

// The fold factor of a node of `members` launches under the tuning value `key` (0 = default, 1 = off, 2, 4; anything else = off):
// members >= F, so the folded grid never has fewer than 256 workgroups.
AQLM_FOLD_HD inline int choose(int key, int members) {
  const int f = key == 0 ? kDefaultFold : key;
  return valid(f) && members >= f ? f : 1;
}

}  // namespace group_fold
}  // namespace aqlm
#endif  // AQLM_GROUP_FOLD_H_

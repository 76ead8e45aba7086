// Chain prefetch of the packed 1x16 matvec (aqlm_hip_gemv_1x16_packed_chain): what the launch tells its prefetch waves about the
// NEXT layer's packed buffer, and when it tells them nothing.  Plain C++ with no dependency on HIP, so that the entry and the host
// test (tests/chain_hint_host.cpp) read one and the same rule.
//
// The prefetch waves of workgroup b read the next layer's entry stream of workgroup b in whole requests of 64 lanes x 16 bytes
// (gemv_1x16_packed_body, packed_gemv_kernels.h):
//     for (off = pw * 1024; off < block_bytes; off += NPW * 1024)  load [stream(b) + off, stream(b) + off + 1024)
// so together they touch [stream(b), stream(b) + block_bytes rounded up to a whole KiB), whatever NPW is.  A stream of 4-byte
// entries is waves x steps KiB.  A stream of 3-byte entries is waves x steps x 776 bytes, in general no whole number of KiB: the
// last request of a block then runs into the next block's stream, and the last request of the LAST block runs past the entry
// area.  In a relabelled buffer the permutation and the codebook image follow the entries, and the bytes are the buffer's own; in
// any other buffer the entry area ends the buffer (used_bytes), and the request would read memory the caller never handed in.
// The data is thrown away, but the read is not the library's to make: the hint is dropped and the launch runs as the plain entry.
#ifndef AQLM_CHAIN_HINT_H_
#define AQLM_CHAIN_HINT_H_

#include <stddef.h>
#include <stdint.h>

namespace aqlm {
namespace chain_hint {

constexpr uint32_t kRequest = 1024;  // bytes of one request of a prefetch wave

struct Hint {
  bool kept;             // false: no prefetch waves, the launch is the plain one
  size_t ent_offset;     // entry area inside the next layer's buffer
  uint32_t block_bytes;  // bytes of one workgroup's stream
};

// offset inside the buffer of the first byte behind the last request for workgroup `block`
inline size_t request_end(size_t off_ent, uint32_t block_bytes, int block) {
  return off_ent + (size_t)block * block_bytes + ((size_t)block_bytes + kRequest - 1) / kRequest * kRequest;
}

// off_ent / ent_bytes / used_bytes / streams: the layout of the next layer's buffer (PackedLayout).  Variable geometry: dropped,
// the hint assumes workgroup b of both layers sits on one XCD with the same slice.
inline Hint decide(size_t off_ent, size_t ent_bytes, int streams, size_t used_bytes, bool variable_geometry) {
  Hint h{false, 0, 0};
  if (variable_geometry || streams < 1 || ent_bytes / (size_t)streams == 0 || ent_bytes / (size_t)streams > 0xffffffffu) return h;
  const uint32_t block_bytes = (uint32_t)(ent_bytes / (size_t)streams);
  if (request_end(off_ent, block_bytes, streams - 1) > used_bytes) return h;  // the last request would leave the buffer
  h.kept = true;
  h.ent_offset = off_ent;
  h.block_bytes = block_bytes;
  return h;
}

}  // namespace chain_hint
}  // namespace aqlm
#endif  // AQLM_CHAIN_HINT_H_

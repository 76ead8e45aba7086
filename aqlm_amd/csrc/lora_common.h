// What the LoRA launches share (lora_bgmv.hip: per-row matvec; lora_bgmv_routed.hip: the same per (token, expert) pair of a
// mixture-of-experts block; lora_sgmv.hip: segmented MFMA GEMM; lora_sgmv_routed.hip: the same on pair tiles of one expert): the
// device contract of the adapter table and the ids, and the argument checks of the entry points.
//
// The contract: an id selects a table entry, so it is range-checked BEFORE it forms an address -- a row whose id lies outside
// [0, num_adapters) touches no table slot and its y row is never written -- and an entry whose rank is no multiple of 8 in
// 8..max_rank (a table that does not belong to this launch) counts as "no adapter".
#pragma once
#include "aqlm_common.h"

namespace aqlm {

constexpr int kLoraMaxRank = 128;  // include/aqlm_hip.h: "max_rank a multiple of 8 in 8..128"

// the table is read through the constant address space (a uniform address: the fields arrive by s_load), and the pointers it
// holds are device-global: said through the address space, or every access through them is a FLAT one
typedef const aqlm_hip_lora_entry __attribute__((address_space(4)))* lora_entry_ptr;
typedef __attribute__((address_space(1))) const u32x4* lora_gbl_u32x4_ptr;

// id of row b, or -1 when it names no adapter; ids == NULL: adapter 0 for every row.  (R: the type the caller goes on with; the
// narrowing sits inside the selection, where it costs the kernels of lora_sgmv.hip nothing.)
template <class R = long>
__device__ __forceinline__ R lora_row_id(const void* ids, int ids_int64, int b, int nadapters) {
  long id = 0;
  if (ids) id = ids_int64 ? reinterpret_cast<const long*>(ids)[b] : (long)reinterpret_cast<const int*>(ids)[b];
  return (id < 0 || id >= (long)nadapters) ? (R)-1 : (R)id;
}

// ... of the rows of a 16-row tile: lanes 0..15 the id of row b0 + lane, or -1 when the row does not exist or names no adapter;
// lanes 16..63: -1
__device__ __forceinline__ int lora_tile_id(const void* ids, int ids_int64, int b0, int rows, int nadapters, int lane) {
  const int b = b0 + lane;
  if (lane >= 16 || b >= rows) return -1;
  return lora_row_id<int>(ids, ids_int64, b, nadapters);
}

// rank of an entry as the kernels use it: an entry that does not belong to this launch counts as rank 0 -- its rows are left
// alone, and nothing is indexed past the workspace row or with a row length of B that is not whole 16-byte pieces
__device__ __forceinline__ int lora_rank(int rank, int max_rank) { return (rank < 8 || rank > max_rank || (rank & 7)) ? 0 : rank; }

inline bool lora_shape_ok(int out_features, int in_features, int max_rank, int rows, int max_rows) {
  return out_features >= 1 && in_features >= 8 && in_features % 8 == 0 && max_rank >= 8 && max_rank <= kLoraMaxRank &&
         max_rank % 8 == 0 && rows >= 1 && rows <= max_rows;
}

// the argument checks of the entry points up to the workspace size, in the order in which they report.  x_rows / y_rows: how many
// rows x and y hold when that is not `rows` (the routed launch: token or pair rows of x, a y row per pair and projection)
inline int lora_check_args(const char* who, const aqlm_hip_lora_entry* table, int num_adapters, int max_rank, const void* ids,
                           int ids_int64, int rows, const void* x, long x_row_stride, const void* y, long y_row_stride,
                           int out_features, int in_features, int dtype, const void* workspace, int max_rows, int x_rows = 0,
                           int y_rows = 0) {
  if (x_rows <= 0) x_rows = rows;
  if (y_rows <= 0) y_rows = rows;
  if (int e = check_not_null(who, table && x && y && workspace)) return e;
  if (!aligned8(table) || (ids && !ids_aligned(ids, ids_int64)) || (reinterpret_cast<uintptr_t>(y) & 1u) || !aligned16(workspace)) {
    set_last_error("%s: table / ids / y / workspace misaligned (8 bytes / the id size / 2 bytes / 16 bytes)", who);
    return AQLM_HIP_E_INVALID;
  }
  if (num_adapters < 1 || rows < 1 || out_features < 1 || in_features < 1 || max_rank < 1) {
    set_last_error("%s: bad sizes (adapters=%d rows=%d out=%d in=%d max_rank=%d)", who, num_adapters, rows, out_features,
                   in_features, max_rank);
    return AQLM_HIP_E_INVALID;
  }
  if (y_row_stride < out_features || x_row_stride < in_features) {
    set_last_error("%s: row strides (x %ld, y %ld) shorter than the rows (in=%d, out=%d)", who, x_row_stride, y_row_stride,
                   in_features, out_features);
    return AQLM_HIP_E_INVALID;
  }
  {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
    const uintptr_t x1 = x0 + ((uintptr_t)(x_rows - 1) * (uintptr_t)x_row_stride + (uintptr_t)in_features) * 2;
    const uintptr_t y1 = y0 + ((uintptr_t)(y_rows - 1) * (uintptr_t)y_row_stride + (uintptr_t)out_features) * 2;
    if (x0 < y1 && y0 < x1) {
      set_last_error("%s: y aliases x (y is read and written in place while other workgroups still read x)", who);
      return AQLM_HIP_E_INVALID;
    }
  }
  if (int e = check_dtype(who, dtype)) return e;
  if (!lora_shape_ok(out_features, in_features, max_rank, rows, max_rows) || !aligned16(x) || (x_rows > 1 && x_row_stride % 8 != 0)) {
    set_last_error("%s: shape outside the kernels (rank a multiple of 8 in 8..%d, in_features %% 8 == 0, 1..%d rows, x rows "
                   "16-byte aligned; got max_rank=%d in=%d rows=%d x stride %ld)", who, kLoraMaxRank, max_rows, max_rank,
                   in_features, rows, x_row_stride);
    return AQLM_HIP_E_UNSUPPORTED;
  }
  return 0;
}

inline int lora_check_workspace(const char* who, size_t workspace_bytes, size_t need) {
  if (workspace_bytes >= need) return 0;
  set_last_error("%s: workspace of %zu bytes, %zu bytes needed", who, workspace_bytes, need);
  return AQLM_HIP_E_INVALID;
}

}  // namespace aqlm

"""ctypes binding of libaqlm_hip.so (include/aqlm_hip.h).

The library is built ahead of time by ``aqlm_amd/csrc/Makefile`` (``__graft_entry__.build()``) and lives
in-tree next to this file.  There is NO fallback: if the shared object is missing or a symbol is absent,
importing this module raises, and every op that needs it raises with it.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AQLM_AMD_HIP_LIB: another build of the same library (same-box A/B runs of two commits, tools/gpu/r3_ab*.sh); default: in-tree
LIB_PATH = os.environ.get("AQLM_AMD_HIP_LIB") or os.path.join(_HERE, "libaqlm_hip.so")
ABI_VERSION = 9

F16, BF16 = 0, 1
F32 = 2   # dW and the outputs of the gradient entries, and the reference of aqlm_hip_code_search_1x16, only
CODE_SEARCH_EPS = 2.0 ** -17   # AQLM_HIP_CODE_SEARCH_EPS
KMEANS_EPS = 2.0 ** -17        # AQLM_HIP_KMEANS_EPS
E_INVALID, E_UNSUPPORTED = -1, -2
MAX_GEMV_BATCH = 8
OP_GEMM_1X16_MFMA = 1
OP_GEMV_1X16_PACKED = 3
OP_GEMV_8X8_LUT = 4
OP_GEMM_KX8_MFMA = 6
OP_GEMV_1X16_G16_PACKED = 5

MAX_SEGMENTS = 4
MAX_ROUTED_PAIRS = 64     # aqlm_hip_gemv_1x16_routed: (token, expert) pairs per call
MAX_ROUTED_EXPERTS = 256
ROUTED_ENTRY_WORDS = 4    # aqlm_hip_routed_entry: codes, codebook, scales, bias (device pointers)
MAX_GROUPED_PAIRS = 1 << 18  # aqlm_hip_gemm_1x16_grouped / aqlm_hip_moe_bucket: (token, expert) pairs per call
GROUPED_TILE_PAIRS = (16, 32, 64, 128)

_vp, _ci, _cl, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t


class Segment(ctypes.Structure):
    """aqlm_hip_segment (include/aqlm_hip.h): one layer of a shared-input launch."""

    _fields_ = [("codes", _vp), ("codebook", _vp), ("scales", _vp), ("bias", _vp), ("y", _vp),
                ("y_row_stride", _cl), ("out_features", _ci), ("reserved", _ci)]


_segp = ctypes.POINTER(Segment)


PACKED_RELABELLED, PACKED_VARGEOM, PACKED_HAS_CODEBOOK = 1, 2, 4   # aqlm_hip_packed_desc.flags
PREPACK_NO_RELABEL, PREPACK_UNIFORM_ONLY = 1, 2                   # aqlm_hip_prepack_1x16_ex flags


class PackedDesc(ctypes.Structure):
    """aqlm_hip_packed_desc (include/aqlm_hip.h): what the kernels need to know about a prepacked 1x16 buffer."""

    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("out_features", ctypes.c_int32),
                ("in_features", ctypes.c_int32), ("slices_log2", ctypes.c_int32), ("waves", ctypes.c_int32),
                ("steps", ctypes.c_int32), ("entry_bytes", ctypes.c_int32), ("used_bytes", ctypes.c_uint64),
                ("x_copies", ctypes.c_uint32), ("codebook_absmax", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("rows_per_group", ctypes.c_int32), ("slice_groups", ctypes.c_uint8 * 32)]

    def as_ints(self):
        """The descriptor as a list of ints (what the registered torch op takes); the float travels as its bit pattern, the 32
        row-group counts as four 64-bit words."""
        import struct

        groups = bytes(self.slice_groups)
        return [int(self.magic), int(self.version), int(self.out_features), int(self.in_features),
                int(self.slices_log2), int(self.waves), int(self.steps), int(self.entry_bytes), int(self.used_bytes),
                int(self.x_copies), struct.unpack("<I", struct.pack("<f", float(self.codebook_absmax)))[0],
                int(self.flags), int(self.rows_per_group)] + [int.from_bytes(groups[8 * i:8 * i + 8], "little", signed=True) for i in range(4)]

    @classmethod
    def from_ints(cls, v):
        import struct

        absmax = struct.unpack("<f", struct.pack("<I", int(v[10]) & 0xFFFFFFFF))[0] if len(v) > 10 else 0.0
        groups = b"".join(int(x).to_bytes(8, "little", signed=True) for x in v[13:17]) if len(v) >= 17 else bytes(32)
        return cls(*[int(x) for x in v[:10]], absmax, int(v[11]) if len(v) > 11 else 0, int(v[12]) if len(v) > 12 else 0,
                   (ctypes.c_uint8 * 32)(*groups))

    @property
    def relabelled(self) -> bool:
        return bool(self.flags & PACKED_RELABELLED)

    @property
    def variable_geometry(self) -> bool:
        return bool(self.flags & PACKED_VARGEOM)


_descp = ctypes.POINTER(PackedDesc)
_descpp = ctypes.POINTER(_descp)


class Xgmi(ctypes.Structure):
    """aqlm_hip_xgmi (include/aqlm_hip.h): one rank's view of the one-shot all-reduce state."""

    _fields_ = [("peer_pub", _vp), ("peer_flag", _vp), ("epoch", _vp), ("status", _vp), ("rank", _ci), ("world", _ci),
                ("max_elems", _ci), ("spin_limit", ctypes.c_uint32)]


_xgp = ctypes.POINTER(Xgmi)


class RoutedPackedEntry(ctypes.Structure):
    """aqlm_hip_routed_packed_entry (include/aqlm_hip.h): one prepacked (expert, projection) of the routed packed launch; filled by
    aqlm_hip_routed_packed_entry_fill, copied to the device as part of the launch's table."""

    _fields_ = [("entries", _vp), ("wave_info", _vp), ("row_starts", _vp), ("codebook", _vp), ("scales", _vp), ("bias", _vp),
                ("out_features", ctypes.c_int32), ("rows_per_group", ctypes.c_int32), ("waves", ctypes.c_int32),
                ("steps", ctypes.c_int32), ("x_copies", ctypes.c_int32), ("entry_stream_bytes", ctypes.c_uint32),
                ("codebook_absmax", ctypes.c_float), ("reserved", ctypes.c_int32)]


ROUTED_PACKED_ENTRY_WORDS = ctypes.sizeof(RoutedPackedEntry) // 8   # 64-bit words of a table entry


class RoutedPackedGeometry(ctypes.Structure):
    """aqlm_hip_routed_packed_geometry: the launch-wide values of one table (aqlm_hip_gemv_1x16_routed_packed_geometry)."""

    _fields_ = [("out_features", ctypes.c_int32), ("in_features", ctypes.c_int32), ("in_group_size", ctypes.c_int32),
                ("rows_per_group", ctypes.c_int32), ("max_waves", ctypes.c_int32), ("slice_first", ctypes.c_int32),
                ("lds_bytes", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


class LoraEntry(ctypes.Structure):
    """aqlm_hip_lora_entry (include/aqlm_hip.h): one adapter of a layer's device table -- A [rank][in], B [out][rank], rank, scaling."""

    _fields_ = [("a", _vp), ("b", _vp), ("rank", ctypes.c_int32), ("scaling", ctypes.c_float)]


LORA_ENTRY_WORDS = ctypes.sizeof(LoraEntry) // 8   # 64-bit words of a table entry
MAX_LORA_ROWS = 256      # aqlm_hip_lora_bgmv: rows per call
MAX_LORA_SGMV_ROWS = 65536   # aqlm_hip_lora_sgmv: rows per call
MAX_LORA_SGMV_ROUTED_PAIRS = 65536   # aqlm_hip_lora_sgmv_routed: (token, expert) pairs per call
MAX_LORA_RANK = 128

_rpep = ctypes.POINTER(RoutedPackedEntry)
_rpgp = ctypes.POINTER(RoutedPackedGeometry)

# name -> (restype, argtypes); mirrors include/aqlm_hip.h one to one
SIGNATURES = {
    "aqlm_hip_abi_version": (_ci, []),
    "aqlm_hip_last_error": (ctypes.c_char_p, []),
    "aqlm_hip_gemv_1x16": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp]),
    "aqlm_hip_gemv_1x16_multi": (_ci, [_segp, _ci, _vp, _ci, _ci, _ci, _cl, _ci, _vp]),
    "aqlm_hip_gemv_1x16_routed": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _ci, _vp, _cl, _ci, _vp, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_moe_bucket_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_moe_bucket": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp]),
    "aqlm_hip_gemm_1x16_grouped_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_gemm_1x16_grouped": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _ci, _vp, _cl, _ci, _vp, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_gemm_1x16_grouped_transposed_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_gemm_1x16_grouped_transposed": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _vp, _cl, _vp, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_gemv_1x16_packed_multi": (_ci, [_segp, _descpp, _ci, _vp, _ci, _ci, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_1x16_packed_multi_cells": (_ci, [_segp, _descpp, _ci, _vp, _ci, _ci, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_1x16_routed_packed_lds_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_routed_packed_entry_fill": (_ci, [_descp, _vp, _vp, _vp, _vp, _rpep]),
    "aqlm_hip_gemv_1x16_routed_packed_geometry": (_ci, [_descpp, _ci, _rpgp]),
    "aqlm_hip_gemv_1x16_routed_packed_supported": (_ci, [_descpp, _ci]),
    "aqlm_hip_gemv_1x16_routed_packed": (_ci, [_vp, _rpgp, _ci, _ci, _vp, _ci, _ci, _ci, _vp, _cl, _ci, _vp, _ci, _vp, _sz, _vp]),
    "aqlm_hip_lora_workspace_bytes": (_sz, [_ci, _ci]),
    "aqlm_hip_lora_bgmv_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_bgmv": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _vp, _cl, _vp, _cl, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_lora_bgmv_routed_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_lora_bgmv_routed_supported": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_bgmv_routed": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _vp, _cl, _ci, _vp, _ci, _ci, _ci, _vp, _sz,
                                  _vp]),
    "aqlm_hip_lora_sgmv_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_lora_sgmv_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_sgmv": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _vp, _cl, _vp, _cl, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_lora_sgmv_routed_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_sgmv_routed_supported": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_sgmv_routed": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _vp, _cl, _ci, _vp, _ci, _ci, _ci, _vp,
                                  _sz, _vp]),
    "aqlm_hip_lora_transpose_routed_bytes": (_sz, [_ci, _ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_transpose_routed_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_transpose_routed": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_lora_grad_routed_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_lora_grad_routed": (_ci, [_vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _vp, _cl, _cl, _ci, _ci, _vp, _cl,
                                  _cl, _ci, _cl, _vp, _sz, _ci, _vp]),
    "aqlm_hip_codebook_grad_chunk": (_ci, []),
    "aqlm_hip_codebook_grad_1x16_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_codebook_grad_1x16_max_chunks": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_codebook_grad_1x16_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_codebook_grad_1x16": (_ci, [_vp, _cl, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _sz, _vp]),
    "aqlm_hip_scales_grad_1x16_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_scales_grad_1x16": (_ci, [_vp, _cl, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp]),
    "aqlm_hip_codebook_grad_kx8_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_codebook_grad_kx8_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_codebook_grad_kx8": (_ci, [_vp, _cl, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _sz, _vp]),
    "aqlm_hip_scales_grad_kx8_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_scales_grad_kx8": (_ci, [_vp, _cl, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp]),
    "aqlm_hip_code_search_1x16_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_code_search_1x16_workspace_bytes": (_sz, [_cl, _ci]),
    "aqlm_hip_code_search_1x16": (_ci, [_vp, _ci, _cl, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _cl, _vp, _vp, _sz, _vp]),
    "aqlm_hip_calib_delta_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_calib_delta": (_ci, [_vp, _vp, _vp, _vp, _ci, _cl, _ci, _ci, _ci, _ci, _ci, _vp, _cl, _vp]),
    "aqlm_hip_calib_rows_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_calib_rows": (_ci, [_vp, _cl, _vp, _cl, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
    "aqlm_hip_calib_codebook_grad_1x16_supported": (_ci, [_ci, _ci, _ci]),
    "aqlm_hip_calib_codebook_grad_1x16_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_calib_codebook_grad_1x16": (_ci, [_vp, _cl, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _sz, _vp]),
    "aqlm_hip_calib_codebook_grad_kx8_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_calib_codebook_grad_kx8_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_calib_codebook_grad_kx8": (_ci, [_vp, _cl, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _sz, _vp]),
    "aqlm_hip_kmeans_supported": (_ci, [_cl, _ci, _ci]),
    "aqlm_hip_kmeans_workspace_bytes": (_sz, [_cl, _ci, _ci]),
    "aqlm_hip_kmeans_assign": (_ci, [_vp, _cl, _vp, _ci, _ci, ctypes.c_float, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aqlm_hip_kmeans_update": (_ci, [_vp, _vp, _cl, _ci, _ci, ctypes.c_float, _vp, _vp]),
    "aqlm_hip_code_search_kx8_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_code_search_kx8_workspace_bytes": (_sz, [_cl, _ci, _ci, _ci]),
    "aqlm_hip_code_search_kx8": (_ci, [_vp, _ci, _cl, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_ci), _vp, _ci, _cl, _vp,
                                 _vp, _vp, _sz, _vp]),
    "aqlm_hip_code_search_kx8_xtx_supported": (_ci, [_ci, _ci, _ci, _ci, _ci]),
    "aqlm_hip_code_search_kx8_xtx_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_code_search_kx8_xtx": (_ci, [_vp, _cl, _cl, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_ci),
                                     _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "aqlm_hip_code_search_1x16_xtx_supported": (_ci, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_code_search_1x16_xtx_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_code_search_1x16_xtx": (_ci, [_vp, _cl, _cl, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _sz, _vp]),
    "aqlm_hip_gemv_kx8_multi": (_ci, [_segp, _ci, _vp, _ci, _ci, _ci, _ci, _cl, _ci, _vp]),
    "aqlm_hip_gemv_kx8": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp]),
    "aqlm_hip_prepack_1x16_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_prepack_1x16": (_ci, [_vp, _ci, _ci, _ci, _vp, _sz, _descp, _vp]),
    "aqlm_hip_prepack_1x16_ex": (_ci, [_vp, _ci, _ci, _ci, _vp, _sz, _descp, _ci, _vp]),
    "aqlm_hip_packed_set_codebook": (_ci, [_descp, _vp, _vp, _vp]),
    "aqlm_hip_packed_plan_relabel": (_ci, [_vp, _ci, _vp]),
    "aqlm_hip_packed_plan_relabel_ex": (_ci, [_vp, _ci, _ci, _vp]),
    "aqlm_hip_packed_plan_geometry": (_ci, [_vp, _ci, _ci, _ci, _vp]),
    "aqlm_hip_packed_desc_read": (_ci, [_vp, _sz, _descp]),
    "aqlm_hip_unpack_1x16": (_ci, [_descp, _vp, _vp, _vp]),
    "aqlm_hip_dequant_1x16_packed": (_ci, [_descp, _vp, _vp, _vp, _vp, _ci, _vp]),
    "aqlm_hip_gemv_1x16_packed": (_ci, [_descp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _cl, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_1x16_packed_image": (_ci, [_descp, _ci, _ci, _sz, ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(_ci)]),
    "aqlm_hip_gemv_1x16_packed_cells": (_ci, [_descp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _cl, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_1x16_packed_chain": (_ci, [_descp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _cl, _cl, _ci, _vp, _sz, _descp, _vp, _vp, _vp]),
    "aqlm_hip_gemv_1x16_packed_chain_plan": (_ci, [_descp, _ci, _ci, _descp, ctypes.POINTER(_ci), ctypes.POINTER(_ci), ctypes.POINTER(_sz)]),
    "aqlm_hip_gemv_1x16_packed_partials": (_ci, [_descp, _vp, _vp, _vp, _ci, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_1x16_packed_publish": (_ci, [_descp, _vp, _vp, _vp, _ci, _cl, _ci, _xgp, _vp, _vp, _vp]),
    "aqlm_hip_xgmi_state_bytes": (_sz, [_ci]),
    "aqlm_hip_xgmi_finalize": (_ci, [_xgp, _vp, _vp, _vp, _vp, _ci, _ci, _cl, _ci, _vp]),
    "aqlm_hip_gemv_8x8_lut": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_8x8_lut_multi": (_ci, [_segp, _ci, _vp, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_8x8_lut_fused": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemv_8x8_lut_multi_fused": (_ci, [_segp, _ci, _vp, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_8x8_planar_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_8x8_planar_pack": (_ci, [_vp, _ci, _ci, _ci, _vp, _sz, _vp]),
    "aqlm_hip_8x8_planar_unpack": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp]),
    "aqlm_hip_gemv_8x8_lut_planar": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, ctypes.c_float, _vp, _sz, _ci, _vp]),
    "aqlm_hip_gemv_8x8_lut_batch": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _ci, ctypes.c_float, _vp, _sz, _vp]),
    "aqlm_hip_gemv_8x8_lut_planar_multi": (_ci, [_segp, ctypes.POINTER(ctypes.c_float), _ci, _vp, _ci, _ci, _ci, _vp, _sz, _ci, _vp]),
    "aqlm_hip_gemv_generic": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp]),
    "aqlm_hip_dequant_1x16": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_dequant_kx8": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_dequant_generic": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "aqlm_hip_gemm_1x16_mfma": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemm_1x16_scan": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cl, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemm_1x16_scan_workspace_bytes": (_sz, [_ci, _ci, _ci]),
    "aqlm_hip_gemm_kx8_mfma": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp]),
    "aqlm_hip_gemm_kx8_mfma_ws": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp, _sz, _vp]),
    "aqlm_hip_gemm_8x8_mfma": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cl, _cl, _ci, _vp]),
    "aqlm_hip_workspace_bytes": (_sz, [_ci, _ci, _ci, _ci]),
    "aqlm_hip_checksum": (_ci, [_vp, _sz, _vp, _vp]),
    "aqlm_hip_set_tuning": (_ci, [ctypes.c_char_p, _ci]),
    "aqlm_hip_get_tuning": (_ci, [ctypes.c_char_p, ctypes.POINTER(_ci)]),
    "aqlm_hip_capture_overlap_stats": (_ci, [ctypes.POINTER(ctypes.c_uint64)]),
    "aqlm_hip_capture_overlap_stats_ex": (_ci, [ctypes.POINTER(ctypes.c_uint64), _ci]),
}


class AqlmHipError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the MI355X HIP library has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C aqlm_amd/csrc`. "
            "aqlm_amd has no fallback path."
        )
    # torch bundles its own libamdhip64.so (same SONAME libamdhip64.so.7); importing torch first makes the
    # dynamic loader resolve our NEEDED entry to the runtime torch already loaded, so stream handles and device
    # pointers are shared with torch.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - the C ABI is usable without torch
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    v = lib.aqlm_hip_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {v}, expected {ABI_VERSION}; rebuild it")
    return lib


lib = _load()


def last_error() -> str:
    return (lib.aqlm_hip_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "") -> None:
    """Map a C-ABI return code to the reference's exception types (cuda_kernel.cpp:9-25, 136-145)."""
    if rc == 0:
        return
    msg = last_error() or what
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == E_INVALID:
        raise ValueError(msg)
    raise AqlmHipError(f"HIP error {rc}: {msg}")


def set_tuning(key: str, value: int) -> None:
    check(lib.aqlm_hip_set_tuning(key.encode(), int(value)), "set_tuning")


def get_tuning(key: str) -> int:
    v = _ci(0)
    check(lib.aqlm_hip_get_tuning(key.encode(), ctypes.byref(v)), "get_tuning")
    return v.value


CAPTURE_OVERLAP_FIELDS = ("seen", "relaxed", "kept_conflict", "kept_window", "runs_broken", "api_failures",
                          "merged", "merge_refused", "nodes_added", "folded", "head_regrouped", "head_moved", "head_refused")


def capture_overlap_stats(reset: bool = False) -> dict:
    """Counters of the packed matvec launches made on a stream under capture (aqlm_hip_capture_overlap_stats);
    `reset` zeroes them after reading."""
    out = (ctypes.c_uint64 * len(CAPTURE_OVERLAP_FIELDS))()
    check(lib.aqlm_hip_capture_overlap_stats_ex(out, len(out)), "capture_overlap_stats")
    if reset:
        check(lib.aqlm_hip_capture_overlap_stats_ex(None, 0), "capture_overlap_stats")
    return dict(zip(CAPTURE_OVERLAP_FIELDS, (int(v) for v in out)))


def packed_image(desc: "PackedDesc", rows: int = 1, dtype: int = F16):
    """-> (dynamic LDS bytes, x window) of the packed 1x16 launch for `rows` input rows of the layer `desc` describes, under the
    current tuning (aqlm_hip_gemv_1x16_packed_image); window 8208 = compact, 65520 = full, 0 = slice first.  No device needed."""
    lds, win = _sz(0), ctypes.c_uint32(0)
    check(lib.aqlm_hip_gemv_1x16_packed_image(ctypes.byref(desc), int(rows), int(dtype), 0, ctypes.byref(lds), ctypes.byref(win), None),
          "packed_image")
    return int(lds.value), int(win.value)


def packed_image_blocks_per_cu(desc: "PackedDesc", rows: int = 1, dtype: int = F16, probe_lds_bytes: int = 0) -> int:
    """Workgroups of that launch's kernel the runtime lets share a CU (hipOccupancyMaxActiveBlocksPerMultiprocessor at the launch's
    block size) at `probe_lds_bytes` of dynamic LDS, 0 = the launch's own.  Needs the current device."""
    n = _ci(0)
    check(lib.aqlm_hip_gemv_1x16_packed_image(ctypes.byref(desc), int(rows), int(dtype), int(probe_lds_bytes), None, None, ctypes.byref(n)),
          "packed_image")
    return n.value


def packed_chain_plan(desc: "PackedDesc", next_desc=None, rows: int = 1, dtype: int = F16):
    """-> (hint kept, prefetch waves, dynamic LDS bytes) of what aqlm_hip_gemv_1x16_packed_chain would launch for `rows` input rows
    of the layer `desc` describes when `next_desc` names the next layer, under the current tuning
    (aqlm_hip_gemv_1x16_packed_chain_plan).  No device needed."""
    kept, waves, lds = _ci(0), _ci(0), _sz(0)
    check(lib.aqlm_hip_gemv_1x16_packed_chain_plan(ctypes.byref(desc), int(rows), int(dtype), None if next_desc is None else ctypes.byref(next_desc),
                                                   ctypes.byref(kept), ctypes.byref(waves), ctypes.byref(lds)), "packed_chain_plan")
    return bool(kept.value), int(waves.value), int(lds.value)

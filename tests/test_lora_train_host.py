"""The dense LoRA training route, the parts that need no GPU: the route predicate as a truth table, the C ABI of aqlm_hip_lora_grad
(declared, bound, exported, ABI 9; the slab rule a function of rows and dim alone) and the checks the Python launch wrappers make
before any native call."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aqlm_hip_lora_grad", "aqlm_hip_lora_grad_supported", "aqlm_hip_lora_grad_slabs", "aqlm_hip_lora_grad_workspace_bytes")


def test_takes_train_route_is_a_pure_table_and_off_by_default(monkeypatch):
    import aqlm_amd.lora as lora

    assert (lora.TRAIN_MIN_ROWS, lora.TRAIN_MAX_ROWS) == (1, 0)
    for flags in itertools.product((False, True), repeat=5):
        for rows in (0, 1, 80, 65536, 65537):
            assert not lora.takes_train_route(*flags[:4], rows, flags[4]), "TRAIN_MAX_ROWS = 0 switches the route off"
    monkeypatch.setattr(lora, "TRAIN_MAX_ROWS", lora.AQLM_HIP_MAX_LORA_SGMV_ROWS)
    for is_cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for rows in (0, 1, 80, 65536, 65537):
            want = is_cuda and dtype_ok and grad and not compiling and supported and 1 <= rows <= 65536
            assert lora.takes_train_route(is_cuda, dtype_ok, grad, compiling, rows, supported) == want
    monkeypatch.setattr(lora, "TRAIN_MAX_ROWS", 64)
    assert lora.takes_train_route(True, True, True, False, 64, True) and not lora.takes_train_route(True, True, True, False, 65, True)


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    for name in ("lora_grad", "lora_grad_supported", "lora_grad_slabs", "lora_sgmv_workspace_floats"):
        assert callable(getattr(hk, name)) and not hasattr(torch.ops.aqlm, name)
    # the sizes: every slab a whole number of 32-row steps, none empty, 256 workgroups on a 4096 x 4096 call
    assert hk.lora_grad_slabs(4096, 4096) == 16 and hk.lora_grad_slabs(1, 8) == 1 and hk.lora_grad_slabs(65, 520) == 3
    for rows, dim in ((1, 8), (33, 264), (4100, 264), (65536, 14336)):
        slabs = hk.lora_grad_slabs(rows, dim)
        steps = (rows + 31) // 32
        per = (steps + slabs - 1) // slabs
        assert 1 <= slabs <= 64 and (slabs - 1) * per < steps
        assert nat.lib.aqlm_hip_lora_grad_workspace_bytes(rows, 24, dim) == slabs * 24 * dim * 4
    assert hk.lora_grad_supported(8, 128, 65536)
    assert not any(hk.lora_grad_supported(*bad) for bad in ((12, 8, 1), (8, 12, 1), (8, 136, 1), (8, 8, 0), (8, 8, 65537)))
    assert hk.lora_sgmv_workspace_floats(80, 24, 2048) == 80 * hk.lora_sgmv_splits(2048) * 24


def test_launch_wrappers_reject_bad_arguments_before_any_native_call(monkeypatch):
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from aqlm_amd.inference_kernels import ops_lora

    class _NoLaunch:  # the queries pass through, a launch is a failure
        def __getattr__(self, name):
            if name in ("aqlm_hip_lora_grad", "aqlm_hip_lora_sgmv"):
                return lambda *a: pytest.fail(f"{name} reached with bad arguments")
            return getattr(nat.lib, name)

    monkeypatch.setattr(ops_lora, "_lib", _NoLaunch())
    rows, dim, rank = 4, 16, 8
    v, w = torch.zeros((rows, dim), dtype=torch.float16), torch.zeros((rows, 1, rank))
    table = torch.zeros(nat.LORA_ENTRY_WORDS, dtype=torch.int64)
    bad = [
        (ValueError, dict(v=v[:, ::2], geometry=[1, rank, dim // 2, 0])),            # inner stride
        (NotImplementedError, dict(v=v.float())),                                   # dtype of V
        (ValueError, dict(w=w.half())),                                             # dtype of w
        (ValueError, dict(w=w[:3])),                                                # rows of w
        (ValueError, dict(table=table[:-1])),                                       # table size
        (ValueError, dict(geometry=[1, rank, dim, 1])),                             # adapter outside the table
        (ValueError, dict(ids=torch.zeros(rows))),                                  # ids dtype
        (ValueError, dict(ids=torch.zeros(rows + 1, dtype=torch.int64))),           # ids length
        (ValueError, dict(out=torch.zeros((rank, dim + 8)))),                       # out shape
        (NotImplementedError, dict(v=v[:, :12], geometry=[1, rank, 12, 0])),        # dim % 8
        (NotImplementedError, dict(w=torch.zeros((rows, 9, rank)))),                # slices
    ]
    for exc, change in bad:
        args = dict(v=v, w=w, ids=None, table=table, geometry=[1, rank, dim, 0], out=None)
        args.update(change)
        with pytest.raises(exc):
            hk.lora_grad(**args)
    y, x = torch.zeros((rows, 16), dtype=torch.float16), torch.zeros((rows, 2048), dtype=torch.float16)
    need = hk.lora_sgmv_workspace_floats(rows, rank, 2048)
    for ws in (torch.zeros(need - 1), torch.zeros(need, dtype=torch.float64), torch.zeros(2 * need)[::2]):
        with pytest.raises(ValueError, match="workspace"):
            hk.lora_sgmv_(y, x, None, table, [1, rank, 16, 2048], workspace=ws)

"""CPU-only: the layout of aqlm_amd/inference_kernels after hip_kernel.py was split by op family.

``hip_kernel`` stays the one namespace callers and tests use: everything ``_launch`` and the ``ops_*`` modules define must be there
under the same name and as the same object (an op added to a family module later and not re-exported fails here); each of the
new modules must be importable first in a fresh interpreter; and the set of ``aqlm::`` ops is the one the single file registered.
"""
import importlib
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "aqlm_amd.inference_kernels"

# the module-level constants (and caches) of each new module; functions and classes are found by their __module__
CONSTANTS = {
    "_launch": ("_DT", "_NO_GUARD", "_WORKSPACES", "_GRAD_DT", "_GRAD_TORCH_DT", "_LIB"),
    "ops_moe": ("_MOE_SCHEMA", "ROUTED_PACKED_GEOMETRY_INTS", "_ROUTED_PACKED_CELLS"),
    "ops_lora": ("_LORA_GMV_SCHEMA", "SGMV_ROUTED_TILE_PAIRS"),
    "ops_grad": ("CODEBOOK_GRAD_CHUNK", "CODEBOOK_GRAD_ENTRIES"),
    "ops_search": ("CODE_SEARCH_EPS", "KMEANS_EPS", "CODE_SEARCH_KX8_MAX_BEAM", "CODE_SEARCH_1X16_XTX_MAX_BEAM"),
}

# every aqlm:: op hip_kernel.py registered before the split
OPS = """
code1x16_dequant_packed code1x16_matmat code1x16_matmat_dequant code1x16_matmat_dequant_transposed code1x16_matmat_multi
code1x16_matmat_packed code1x16_moe_matmat code1x16_moe_matmat_grouped code1x16_moe_matmat_grouped_transposed
code1x16_moe_matmat_packed code1x8_matmat code1x8_matmat_dequant code1x8_matmat_dequant_transposed code2x8_matmat
code2x8_matmat_dequant code2x8_matmat_dequant_transposed code8x8_matmat_planar code_search_1x16 code_search_kx8
codebook_grad_1x16 codebook_grad_kx8 codekx8_matmat codekx8_matmat_multi generic_matmat generic_matmat_dequant
generic_matmat_dequant_transposed kmeans_assign kmeans_update_ lora_bgmv_ lora_bgmv_routed_ lora_grad_routed lora_sgmv_
lora_sgmv_routed_ lora_transpose_routed_ moe_bucket scales_grad_1x16 scales_grad_kx8
""".split()


@pytest.mark.parametrize("name", sorted(CONSTANTS))
def test_every_definition_is_the_same_object_in_hip_kernel(name):
    hk = importlib.import_module(f"{PACKAGE}.hip_kernel")
    module = importlib.import_module(f"{PACKAGE}.{name}")
    defined = [n for n, v in vars(module).items()
               if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == module.__name__]
    assert defined  # the walk found the module's definitions
    for n in defined + list(CONSTANTS[name]):
        assert hasattr(module, n), f"{name}.{n} is listed in this test and gone from the module"
        assert getattr(hk, n, None) is getattr(module, n), f"{name}.{n} is not re-exported by hip_kernel as the same object"


@pytest.mark.parametrize("name", sorted(CONSTANTS))
def test_each_module_imports_first_and_the_ops_are_the_same(name):
    code = (f"import {PACKAGE}.{name}\n"
            f"import {PACKAGE}.hip_kernel\n"
            "import torch\n"
            "print(' '.join(sorted(s.split('::')[1] for s in torch._C._dispatch_get_all_op_names()"
            " if s.startswith('aqlm::') and '.' not in s)))\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.split() == sorted(OPS)

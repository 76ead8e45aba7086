#!/usr/bin/env python3
"""Record the reference's own Triton gemv on the GPU for tests/test_reference_triton.py: tests/golden/reference_triton_golden.npz.

Needs the MI355X and the staged reference kernel (oracle/_ref/triton_kernel.py, `make -C oracle ref`); the committed .npz is what
travels, so the test does not depend on the staged file.  Per case (the seeded layer make_layer(SEED, in, out, K, nbits, g) with
bias, one row) it records

  * `<case>/sha256` -- of the layer's input arrays, so that a test can prove it regenerated the same inputs;
  * `<case>/y_triton32` -- triton_matmul(x, codes, codebooks, scales, bias), its fp16 output up-cast to float32 (exact).

    python oracle/gen_triton_golden.py [OUT.npz]
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 11
CASES = [(1, 16, 8, 1024, 512), (2, 8, 8, 1024, 512), (8, 8, 32, 2048, 256)]  # (K, nbits, g, in, out)


def case_name(K, nbits, g, fin, fout):
    return f"{K}x{nbits}g{g}_{fin}x{fout}"


def inputs_sha256(L):
    h = hashlib.sha256()
    for k in ("x", "codes", "codebooks", "scales", "bias"):
        h.update(L[k].tobytes())
    return h.hexdigest()


def main():
    import numpy as np
    import torch

    sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
    import reference_triton as rt
    from oracle import aqlm_oracle as orc

    ref = rt.load_reference()
    if ref is None:
        sys.exit("oracle/_ref/triton_kernel.py is not staged (make -C oracle ref) or Triton is missing")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "reference_triton_golden.npz")
    dev = torch.device("cuda:0")
    rec = {}
    for K, nbits, g, fin, fout in CASES:
        L = orc.make_layer(SEED, fin, fout, K, nbits, g, batch=1, bias=True)
        t = {k: torch.from_numpy(L[k]).to(dev) for k in ("x", "codes", "codebooks", "scales", "bias")}
        y = ref.triton_matmul(t["x"].clone(), t["codes"], t["codebooks"], t["scales"], t["bias"]).float().cpu().numpy()
        name = case_name(K, nbits, g, fin, fout)
        rec[f"{name}/sha256"] = np.array(inputs_sha256(L))
        rec[f"{name}/y_triton32"] = y.astype(np.float32)
        print(name, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()

"""Training LoRA adapters on a dense AQLM layer on the MI355X: ``LoraQuantizedLinear`` with ``aqlm.lora.TRAIN_MAX_ROWS`` switched on
(``_DenseAdapterFunction``: aqlm_hip_lora_sgmv forward, the same launch on the transposed table for grad_x, aqlm_hip_lora_grad for
grad_A / grad_B) against fp64 autograd of the function and against the torch path of the same call.

Tolerance per element: the project's own, ``check_bound`` of tests/test_lora_sgmv_gpu.py -- ``el_tol * mean|g64| + 4 ulp_T`` with
el_tol 2e-3 (fp16) / 1.6e-2 (bf16).  In addition each gradient's MEAN absolute error on the new route must not exceed the torch
path's: the new route keeps t and u in fp32 and rounds once, the torch path rounds the intermediate and every product to 16 bits
(the mean, because the maximum over a few thousand elements is noise)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIN, FOUT, ROWS = 2048, 256, 80  # two sgmv slices of in_features, so t arrives in two slices
RANKS = {"a": 8, "b": 24, "c": 16}
SCALINGS = {"a": 2.0, "b": 0.5, "c": 1.25}


def _quantized(seed, fin, fout, dtype):
    from aqlm import QuantizedLinear
    from oracle import aqlm_oracle as orc

    L = orc.make_layer(seed, fin, fout, 1, 16, 8, batch=1, bias=True)
    m = QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=True, device=DEV, dtype=dtype)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)  # noqa: E731
    with torch.no_grad():
        m.codes.copy_(torch.from_numpy(L["codes"]).to(DEV))
        m.codebooks.copy_(f(L["codebooks"]))
        m.scales.copy_(f(L["scales"]).reshape(m.scales.shape))
        m.bias.copy_(f(L["bias"]))
    return m


def _wrapped(dtype, fin=FIN, fout=FOUT):
    import aqlm_amd.lora as lora

    w = lora.LoraQuantizedLinear(_quantized(31, fin, fout, dtype))
    gen = torch.Generator().manual_seed(5)
    for name, r in RANKS.items():
        w.add_adapter(name, (torch.randn((r, fin), generator=gen) / fin ** 0.5).to(dtype),
                      (torch.randn((fout, r), generator=gen) / r ** 0.5).to(dtype), SCALINGS[name])
    w.lora_A["b"].weight.requires_grad_(True)
    w.lora_B["b"].weight.requires_grad_(True)
    return lora, w


def _grads64(w, x, gy, ids):
    """fp64 autograd of y = x W^T + bias + sum_a [ids == a] scaling_a (x A_a^T) B_a^T -> gradients of x, A_b, B_b."""
    base = w.base_layer
    cb = base.codebooks.double()[0, :, 0, :]  # [65536, 8]
    w64 = (cb[base.codes.long().reshape(base.out_features, -1) & 0xFFFF] * base.scales.double().reshape(-1, 1, 1)).reshape(base.out_features, -1)
    x64 = x.detach().double().reshape(-1, x.shape[-1]).requires_grad_(True)
    a64, b64 = (w.lora_A["b"].weight.detach().double().requires_grad_(True), w.lora_B["b"].weight.detach().double().requires_grad_(True))
    y = x64 @ w64.T + base.bias.double()
    for i, name in enumerate(w.bank.names):
        A, B = (a64, b64) if name == "b" else (w.lora_A[name].weight.double(), w.lora_B[name].weight.double())
        y = y + (ids == i).double()[:, None] * (SCALINGS[name] * ((x64 @ A.T) @ B.T))
    y.backward(gy.double().reshape(y.shape))
    return x64.grad.reshape(x.shape), a64.grad, b64.grad


def _errors(g, g64, dtype, what):
    """The per-element tolerance of tests/test_lora_sgmv_gpu.py; -> the mean absolute error."""
    g, g64 = g.double().cpu().numpy(), g64.cpu().numpy()
    assert np.isfinite(g).all(), f"{what}: non-finite gradient"
    mant = 10 if dtype == torch.float16 else 7
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(g64), 2.0 ** -14))) - mant)
    err = np.abs(g - g64)
    bound = (2e-3 if dtype == torch.float16 else 1.6e-2) * np.mean(np.abs(g64)) + 4 * ulp
    print(f"{what}: worst error / bound {float((err / bound).max()):.3f}, mean error {err.mean():.4g}")
    assert not (err > bound).any(), f"{what}: {(err > bound).sum()} elements outside the bound, worst {err.max():.4g}"
    return err.mean()


@pytest.mark.parametrize("mode", ["name", "ids", "seq"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_dense_train_route_against_fp64_and_the_torch_path(dtype, mode, monkeypatch):
    lora, w = _wrapped(dtype)
    from aqlm_amd.inference_kernels import hip_kernel as hk

    assert lora.TRAIN_MAX_ROWS == 0, "the route is opt-in"
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((2, 40, FIN) if mode == "seq" else (ROWS, FIN), generator=gen).to(dtype).to(DEV)
    gy = torch.randn(x.shape[:-1] + (FOUT,), generator=gen).to(dtype).to(DEV)
    if mode == "name":
        sel, row_ids = "b", torch.ones(ROWS, dtype=torch.int64, device=DEV)
    elif mode == "ids":
        sel = row_ids = torch.tensor([(1, 0, 3, 1, 2)[b % 5] for b in range(ROWS)], device=DEV)  # 3 lies outside the bank
    else:
        sel, row_ids = torch.tensor([1, 0], device=DEV), torch.tensor([1] * 40 + [0] * 40, device=DEV)
    w.bank.select(sel)
    grads, torch_path = [], []
    real_grad, real_torch = hk.lora_grad, w._torch_path
    monkeypatch.setattr(hk, "lora_grad", lambda *a, **k: (grads.append(a[4][2]), real_grad(*a, **k))[1])
    monkeypatch.setattr(w, "_torch_path", lambda *a: (torch_path.append(1), real_torch(*a))[1])

    def step():
        for p in w.parameters():
            p.grad = None
        xg = x.clone().requires_grad_(True)
        y = w(xg)
        y.backward(gy)
        assert all(w.lora_A[n].weight.grad is None and w.lora_B[n].weight.grad is None for n in ("a", "c"))
        return y.detach(), xg.grad, w.lora_A["b"].weight.grad, w.lora_B["b"].weight.grad

    with torch.no_grad():
        served = w(x)  # the SGMV route
    monkeypatch.setattr(lora, "TRAIN_MAX_ROWS", lora.AQLM_HIP_MAX_LORA_SGMV_ROWS)
    y, *new = step()
    assert sorted(grads) == [FOUT, FIN] and not torch_path, "the device route was not taken (one lora_grad per trained weight)"
    assert torch.equal(y, served), "the training forward is not the serving route's output"
    monkeypatch.setattr(lora, "TRAIN_MAX_ROWS", 0)  # the default: the torch path, no lora_grad launch
    _, *old = step()
    assert len(grads) == 2 and torch_path == [1]
    for g, gt, g64, what in zip(new, old, _grads64(w, x, gy, row_ids), ("grad_x", "grad_A", "grad_B")):
        e_new = _errors(g, g64, dtype, f"{mode} {what} device route")
        e_old = _errors(gt, g64, dtype, f"{mode} {what} torch path")
        assert e_new <= e_old, f"{what}: mean error {e_new:.4g} on the device route, {e_old:.4g} on the torch path"


def test_an_odd_out_features_keeps_the_torch_path(monkeypatch):
    lora, w = _wrapped(torch.float16, fin=1024, fout=298)
    monkeypatch.setattr(lora, "TRAIN_MAX_ROWS", lora.AQLM_HIP_MAX_LORA_SGMV_ROWS)
    torch_path, real_torch = [], w._torch_path
    monkeypatch.setattr(w, "_torch_path", lambda *a: (torch_path.append(1), real_torch(*a))[1])
    w.bank.select("b")
    x = torch.randn((ROWS, 1024), generator=torch.Generator().manual_seed(2)).half().to(DEV)
    w(x).float().sum().backward()
    assert torch_path == [1] and torch.isfinite(w.lora_A["b"].weight.grad).all()

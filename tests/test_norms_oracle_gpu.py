"""RMSNorm, fused residual RMSNorm and LayerNorm kernels vs fp64, at the
launch geometries the one-shape tests in test_ops_gpu.py never reach:
every VPT instantiation of the fused kernel with a ragged last sweep, the
row stride past 8192 blocks, the dw/db row-accumulation loop, partial
waves, one row, eps-dominated rows, and rows whose mean dwarfs their spread.
Rule, references and k: kernel_oracle.py."""
import dataclasses

import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
DEV = "cuda:0"

# H: VPT=1 / ragged VPT=1 / VPT=2, 4, 8 with a ragged last sweep / the limit
RMS_CASES = [(3, 64, 1.0), (3, 768, 1.0), (3, 2112, 1.0), (3, 4160, 1.0),
             (3, 8256, 1.0), (3, 16384, 1.0),
             (8200, 64, 1.0),          # rows stride the 8192-block grid
             (3, 768, 1e-3)]           # eps dominates mean(x^2)


def g(t):
    return t.to(DEV)


@pytest.mark.parametrize("rows,H,mag", RMS_CASES)
def test_rmsnorm_vs_fp64(rows, H, mag):
    x, dy = ko.bf(rows, H, scale=mag, seed=1), ko.bf(rows, H, seed=2)
    w = ko.bf(H, seed=3)
    y, invr = ops._C.rmsnorm_fwd(g(x), g(w), EPS)
    dx, dw = ops._C.rmsnorm_bwd(g(x), g(w), g(dy), invr)
    assert dw.dtype == torch.float32
    ko.check_all(f"rmsnorm[{rows}x{H},{mag}]",
                 {"y": y, "invr": invr, "dx": dx, "dw": dw},
                 ko.rmsnorm(x, w, EPS, dy))


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("rows,H,mag", RMS_CASES)
def test_rmsnorm_residual_vs_fp64(rows, H, mag, with_res):
    x, dy = ko.bf(rows, H, scale=mag, seed=1), ko.bf(rows, H, seed=2)
    w = ko.bf(H, seed=3)
    res = ko.bf(rows, H, scale=mag, seed=5) if with_res else None
    dxr = ko.bf(rows, H, seed=4) if with_res else None
    tag = f"rmsnorm_res[{rows}x{H},{mag},{'res' if with_res else 'nores'}]"

    y, xr, invr = ops._C.rmsnorm_res_fwd(
        g(x), g(res) if with_res else None, g(w), EPS)
    if with_res:
        ko.check(tag + ".xr", xr, ko.residual_sum(x, res))
    else:
        assert torch.equal(xr.cpu(), x)
    # everything downstream is judged from the xr the kernel formed
    specs = ko.rmsnorm(xr, w, EPS, dy, dxr)
    dx, dw = ops._C.rmsnorm_res_bwd(xr, g(w), g(dy),
                                    g(dxr) if with_res else None, invr)
    assert dw.dtype == torch.float32
    ko.check_all(tag, {"y": y, "invr": invr, "dx": dx, "dw": dw}, specs)

    # the autograd wrapper: same numbers, and dres is dx
    xg, wg = g(x).requires_grad_(True), g(w).requires_grad_(True)
    rg = g(res).requires_grad_(True) if with_res else None
    y2, xr2 = ops.rmsnorm_residual(xg, rg, wg, EPS)
    if with_res:
        torch.autograd.backward([y2, xr2], [g(dy), g(dxr)])
    else:
        y2.backward(g(dy))
    assert torch.equal(y2, y) and torch.equal(xr2, xr)
    assert torch.equal(xg.grad, dx)
    if with_res:
        ko.check(tag + ".dres", rg.grad, specs["dx"])
    # dw's atomics may land in another order: judged, not bit-compared
    ko.check(tag + ".dw_bf16", wg.grad,
             dataclasses.replace(specs["dw"], bf16=True))


def test_rmsnorm_residual_rejects_rows_wider_than_its_kernels():
    H = 16392
    x, w = g(ko.bf(2, H, seed=1)), g(ko.bf(H, seed=3))
    with pytest.raises(RuntimeError, match="16384"):
        ops._C.rmsnorm_res_fwd(x, None, w, EPS)
    with pytest.raises(RuntimeError, match="16384"):
        ops._C.rmsnorm_res_bwd(x, w, x, None,
                               torch.ones(2, device=DEV))
    # the plain kernel loops over columns and takes any H
    y, invr = ops._C.rmsnorm_fwd(x, w, EPS)
    ko.check_all("rmsnorm[2x16392]", {"y": y, "invr": invr},
                 ko.rmsnorm(x, w, EPS))


LN_CASES = [(3, 768), (3, 1600), (3, 2056),   # partial wave / H/8 > 256
            (8200, 64),                        # row stride
            (2100, 64),                        # dw/db accumulate over rows
            (1, 768),
            ("offset", 100.0), ("offset", 200.0), "const"]


@pytest.mark.parametrize("case", LN_CASES, ids=str)
def test_layernorm_vs_fp64(case):
    x, w, b, dy = ko.ln_inputs(case)
    y, mu, rstd = ops._C.layernorm_fwd(g(x), g(w), g(b), EPS)
    dx, dw, db = ops._C.layernorm_bwd(g(x), g(w), g(dy), mu, rstd)
    assert dw.dtype == db.dtype == torch.float32
    specs = ko.layernorm(x, w, b, EPS, dy)
    if case == "const":
        # a constant row has var = 0 exactly: rstd is 1/sqrt(eps)
        assert torch.allclose(specs["rstd"].ref[:2],
                              torch.full((2,), EPS ** -0.5,
                                         dtype=torch.float64))
    ko.check_all(f"layernorm[{case}]",
                 {"y": y, "mu": mu, "rstd": rstd, "dx": dx, "dw": dw,
                  "db": db}, specs)

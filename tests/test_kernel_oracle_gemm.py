"""CPU checks of the weight-gradient reference and of ops.linear: the torch
fallback of ops.wgrad_gemm_ passes the rule, deliberately wrong references
fail it on every shape the GPU test runs, and ops.linear equals F.linear."""
import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko
import kernel_oracle_gemm as kg
from torch_on_k8s_amd import ops

NKS = ((256, 256), (512, 768), (768, 768), (2304, 256), (256, 2304))
MS = (64, 448)


@pytest.mark.parametrize("NK", NKS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", MS)
def test_fallback_passes_and_mutants_fail(M, NK):
    N, K = NK
    dy, x, old = kg.wgrad_inputs(M, N, K, seed=M + N + 3 * K)
    assert not ops.wgrad_fast_path(dy, x, old)        # CPU tensors
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16)
    ops.wgrad_gemm_(dy, x, out, False)
    ko.check(f"fallback[{M},{N},{K}].overwrite", out, kg.wgrad(dy, x))
    acc = old.clone()
    ops.wgrad_gemm_(dy, x, acc, True)
    ko.check(f"fallback[{M},{N},{K}].accumulate", acc,
             kg.wgrad(dy, x, old, rounded_twice=True))

    # a result that is right by the one-rounding rule ...
    good = kg.wgrad(dy, x, old).ref.to(torch.bfloat16)
    assert ko.compare("good", good, kg.wgrad(dy, x, old)).violations == 0
    # ... breaks every wrong reference
    for flag in ("drop_last_step", "transposed", "ignore_old", "swap_blocks"):
        bad = kg.wgrad(dy, x, old, **{flag: True})
        assert ko.compare(flag, good, bad).violations > 0, flag


def test_wgrad_gemm_rejects_misfit_shapes():
    dy, x, old = kg.wgrad_inputs(64, 256, 256)
    with pytest.raises(ValueError):
        ops.wgrad_gemm_(dy, x[:32], old, True)
    with pytest.raises(ValueError):
        ops.wgrad_gemm_(dy, x, old.t()[:, :128], True)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("shape", ((3, 5, 24), (7, 24)))
def test_linear_equals_f_linear_bitwise(dtype, shape, monkeypatch):
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(*shape, generator=g).to(dtype)
    w0 = torch.randn(40, shape[-1], generator=g).to(dtype)
    dy = torch.randn(*shape[:-1], 40, generator=g).to(dtype)
    res = []
    for fn in (ops.linear, F.linear):
        x = x0.clone().requires_grad_()
        w = w0.clone().requires_grad_()
        y = fn(x, w)
        y.backward(dy)
        res.append((y.detach(), x.grad, w.grad))
    for got, want in zip(*res):
        assert torch.equal(got, want)


def test_linear_accumulates_in_place_only_when_marked(monkeypatch):
    """A marked weight without hooks gets its gradient added into the
    existing .grad storage; a post-accumulate hook switches that off and
    fires once per backward."""
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(6, 16, generator=g)
    w = torch.nn.Parameter(torch.randn(8, 16, generator=g))
    flat = torch.ones(8 * 16)
    w.grad = flat.view(8, 16)
    w._tok_flat_grad = True
    dy = torch.randn(6, 8, generator=g)
    ops.linear(x, w).backward(dy)
    assert w.grad.data_ptr() == flat.data_ptr()
    assert torch.equal(w.grad, 1 + dy.t() @ x)

    fired = []
    w.register_post_accumulate_grad_hook(lambda p: fired.append(1))
    flat.fill_(1.0)
    ops.linear(x, w).backward(dy)
    assert fired == [1]
    assert torch.equal(w.grad, 1 + dy.t() @ x)


def test_tensor_hook_switches_in_place_off(monkeypatch):
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 16, generator=g)
    w = torch.nn.Parameter(torch.randn(8, 16, generator=g))
    flat = torch.ones(8 * 16)
    w.grad = flat.view(8, 16)
    w._tok_flat_grad = True
    seen = []
    w.register_hook(lambda gr: seen.append(gr.clone()))
    dy = torch.randn(6, 8, generator=g)
    ops.linear(x, w).backward(dy)
    assert len(seen) == 1 and torch.equal(seen[0], dy.t() @ x)
    assert torch.equal(w.grad, 1 + dy.t() @ x)


def test_dispatch_table(monkeypatch):
    """Measured winners go to the kernel, the measured loser and every
    unmeasured shape to the library; hip_all overrides for tests."""
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)
    assert ops.wgrad_band(28672, 4096) == 4 and ops.wgrad_band(4096, 4096) == 8
    assert ops.wgrad_band(6144, 4096) is None
    assert ops.wgrad_band(256, 256) is None
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    assert ops.wgrad_band(256, 256) == 4 and ops.wgrad_band(6144, 4096) == 4
    assert ops.wgrad_band(4096, 4096) == 8
    monkeypatch.setenv("TOK_WGRAD_IMPL", "blas")
    assert ops.wgrad_band(28672, 4096) is None


def test_wgrad_impl_env(monkeypatch):
    monkeypatch.setenv("TOK_WGRAD_IMPL", "blas")
    assert ops.wgrad_impl() == "blas"
    monkeypatch.setenv("TOK_WGRAD_IMPL", "nope")
    with pytest.raises(ValueError):
        ops.wgrad_impl()

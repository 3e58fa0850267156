"""The input gradient of ops.linear through the transposed weight copy
(TOK_DGRAD_IMPL=wt_all unless a test says otherwise): dx against the fp64
reference of kernel_oracle_dgrad per element, bitwise against the TN call it
stands for, the routing rules, and llama-tiny inside the trainer."""
import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko
import kernel_oracle_dgrad as kd
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext

pytestmark = pytest.mark.gpu

# several tiles each way; partial tiles in N and K; one K tile, long N;
# square with an asymmetric W (a copy that was not transposed would fit)
MNKS = ((128, 256, 192), (64, 72, 136), (192, 512, 64), (128, 256, 256))

_inputs = {}


@pytest.fixture(autouse=True)
def transposed_everywhere(monkeypatch):
    """These shapes are not in the dispatch table; transpose anyway."""
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt_all")
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)


def inputs(M, N, K):
    """(dy, W, x) on the GPU and the Spec of dx, computed once per shape."""
    key = (M, N, K)
    if key not in _inputs:
        dy, w = kd.dgrad_inputs(M, N, K, seed=M + N + 3 * K)
        x = ko.bf(M, K, seed=7)
        _inputs[key] = (dy.cuda(), w.cuda(), x.cuda(), kd.dgrad(dy, w))
    return _inputs[key]


def backward(dy, w, x, x_grad=True):
    xr = x.clone().requires_grad_(x_grad)
    wr = w.clone().requires_grad_()
    ops.linear(xr, wr).backward(dy)
    return xr.grad, wr.grad


def spy_on(monkeypatch, name):
    """Log (copies of the arguments, copy of the result) of every call of
    ops.<name>: the optimizer rewrites the live weights after backward."""
    calls = []
    real = getattr(ops, name)

    def spy(*a, **kw):
        seen = tuple(t.clone() for t in a)
        out = real(*a, **kw)
        calls.append((seen, out.clone()))
        return out

    monkeypatch.setattr(ops, name, spy)
    return calls


@pytest.mark.parametrize("MNK", MNKS, ids=lambda s: "x".join(map(str, s)))
def test_dx_matches_fp64_and_tn_call_bitwise(MNK, monkeypatch):
    M, N, K = MNK
    dy, w, x, spec = inputs(M, N, K)
    if N == K:
        assert not torch.equal(w, w.t())
    launches = spy_on(monkeypatch, "transpose_2d_")
    dx, dw = backward(dy, w, x)
    assert len(launches) == 1
    ko.check(f"dgrad_wt[{M},{N},{K}]", dx, spec)
    assert torch.equal(dx, F.linear(dy, w.t().contiguous()))
    monkeypatch.setenv("TOK_DGRAD_IMPL", "blas")
    dx_nn, dw_nn = backward(dy, w, x)
    assert len(launches) == 1
    assert torch.equal(dw, dw_nn)
    ko.check(f"dgrad_nn[{M},{N},{K}]", dx_nn, spec)


def test_unlisted_shape_defaults_to_library(monkeypatch):
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt")
    M, N, K = 128, 256, 192
    assert (N, K) not in ops._DGRAD_DISPATCH
    dy, w, x, _ = inputs(M, N, K)
    launches = spy_on(monkeypatch, "transpose_2d_")
    dx, _ = backward(dy, w, x)
    assert not launches
    assert torch.equal(dx, dy.mm(w))


def test_shape_in_table_takes_transposed_path(monkeypatch):
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt")
    M, N, K = 128, 256, 192
    monkeypatch.setitem(ops._DGRAD_DISPATCH, (N, K), True)
    dy, w, x, spec = inputs(M, N, K)
    launches = spy_on(monkeypatch, "transpose_2d_")
    dx, _ = backward(dy, w, x)
    assert len(launches) == 1
    (src, wt), _ = launches[0]
    assert tuple(src.shape) == (N, K) and tuple(wt.shape) == (K, N)
    assert torch.equal(dx, F.linear(dy, w.t().contiguous()))
    ko.check("dgrad_wt.table", dx, spec)
    # a measured loser stays on the library
    monkeypatch.setitem(ops._DGRAD_DISPATCH, (N, K), False)
    backward(dy, w, x)
    assert len(launches) == 1


def test_wgrad_hip_all_does_not_imply_wt_all(monkeypatch):
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt")
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    dy, w, x, _ = inputs(128, 256, 256)
    launches = spy_on(monkeypatch, "transpose_2d_")
    dx, _ = backward(dy, w, x)
    assert not launches and torch.equal(dx, dy.mm(w))


def test_nothing_launched_when_x_needs_no_grad(monkeypatch):
    dy, w, x, _ = inputs(128, 256, 192)
    launches = spy_on(monkeypatch, "transpose_2d_")
    dgrads = spy_on(monkeypatch, "dgrad")
    dx, dw = backward(dy, w, x, x_grad=False)
    assert dx is None and not launches and not dgrads
    assert torch.equal(dw, backward(dy, w, x)[1])


# ---- llama-tiny inside the trainer ---------------------------------------
def _trainer(**kw):
    torch.cuda.set_device(0)
    cfg = TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=128, **kw)
    return Trainer(cfg, DistContext(device=torch.device("cuda", 0)))


def test_tiny_step_every_dgrad_judged_and_loss_equals_blas(monkeypatch):
    monkeypatch.setenv("TOK_DGRAD_IMPL", "blas")
    tb = _trainer()
    loss_b = tb.train_step()
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt_all")
    launches = spy_on(monkeypatch, "transpose_2d_")
    dgrads = spy_on(monkeypatch, "dgrad")
    tw = _trainer()
    loss_w = tw.train_step()
    # step 1's loss is formed before any backward ran: bit-equal
    assert loss_w == loss_b
    nlin = sum(1 for n, p in tw.module.named_parameters()
               if p.dim() == 2 and "embed" not in n)
    assert len(dgrads) == nlin and len(launches) == nlin
    for i, ((dy2, w), dx) in enumerate(dgrads):
        ko.check(f"tiny.dgrad{i}[{tuple(w.shape)}]", dx, kd.dgrad(dy2, w))
        assert torch.equal(dx, F.linear(dy2, w.t().contiguous()))


def test_graph_step_equals_eager_step():
    tg = _trainer(hip_graph=True)
    tg.train_step(sync=False)        # two warm-up steps and one replay
    te = _trainer(clip_on_device=True)
    while te.step_count < tg.step_count:
        te.train_step(sync=False)
    assert tg.step_count == 3
    for a, b in zip(tg.fb.buckets, te.fb.buckets):
        assert torch.equal(a.flat_grad, b.flat_grad)
        assert torch.equal(a.flat_param, b.flat_param)

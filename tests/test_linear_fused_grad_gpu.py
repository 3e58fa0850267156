"""ops.linear inside the trainer on llama-tiny: the weight gradients the
HIP path leaves in the flat buckets, judged per element by the rule of
kernel_oracle against fp64 references formed from the very operands each
wgrad call received (recorded on the way in), and the library path judged
against the same references.

Only the weight gradients of the linear layers can differ between the two
paths: forward and dgrad are the same library calls on the same values, so
every other gradient must be bit-equal.

llama-tiny's shapes are not in the dispatch table (nobody trains them for
speed), so the HIP runs set TOK_WGRAD_IMPL=hip_all: the kernel wherever it
can run.
"""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_gemm as kg
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext

pytestmark = pytest.mark.gpu


def _trainer(**kw):
    torch.cuda.set_device(0)
    cfg = TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=128, **kw)
    return Trainer(cfg, DistContext(device=torch.device("cuda", 0)))


def _record(monkeypatch):
    """Log (dy, x, out before, out after, accumulate, out's address) of
    every ops.wgrad_gemm_ call."""
    calls = []
    real = ops.wgrad_gemm_

    def spy(dy, x, out, accumulate, **kw):
        before = out.clone()
        real(dy, x, out, accumulate, **kw)
        calls.append((dy.cpu(), x.cpu(), before.cpu(), out.clone().cpu(),
                      accumulate, out.data_ptr()))
        return out

    monkeypatch.setattr(ops, "wgrad_gemm_", spy)
    return calls


def _linear_weights(tr):
    return {n: p for n, p in tr.module.named_parameters()
            if p.dim() == 2 and "embed" not in n}


def _check_calls(calls, tag):
    for i, (dy, x, before, after, acc, _) in enumerate(calls):
        assert ops.wgrad_fast_path(dy.cuda(), x.cuda(), after.cuda())
        ko.check(f"{tag}.call{i}[{tuple(after.shape)}]", after,
                 kg.wgrad(dy, x, before if acc else None))


def _sum_spec(parts, lib):
    """Spec of the sum over micro-steps of dy^T x for one weight. What is
    already in the bucket is bf16: the HIP path has rounded every partial
    sum but the last before it adds the next product, the library path
    rounds every product before its add_. Each such rounding is allowed its
    worst-case half ulp, 2^-8 of the (larger) sum of |partials| so far."""
    specs = [kg.wgrad(dy, x) for dy, x in parts]
    ref = sum(s.ref for s in specs)
    scale = sum(s.scale for s in specs)
    spec = ko.Spec(ref, scale, ko.kred(parts[0][0].shape[0] + len(parts)),
                   True)
    if len(parts) > 1:
        early = specs if lib else specs[:-1]
        spec.tiny = spec.tiny + ko.BF16_HALF_ULP * sum(
            s.ref.abs() for s in early).reshape(-1)
    return spec


@pytest.mark.parametrize("accum", (1, 2))
def test_hip_step_matches_blas_step(accum, monkeypatch):
    monkeypatch.setenv("TOK_WGRAD_IMPL", "blas")
    tb = _trainer(grad_accum_steps=accum)
    tb.train_step()
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    calls = _record(monkeypatch)
    th = _trainer(grad_accum_steps=accum)
    th.train_step()
    wb, wh = _linear_weights(tb), _linear_weights(th)
    assert len(calls) == accum * len(wh)
    assert all(c[4] for c in calls)          # in place, accumulate=True
    _check_calls(calls, f"accum{accum}")
    # every call landed in its weight's flat-bucket view
    by_ptr = {}
    for dy, x, _, _, _, ptr in calls:
        by_ptr.setdefault(ptr, []).append((dy, x))
    for name, p in wh.items():
        parts = by_ptr[p.grad.data_ptr()]
        assert len(parts) == accum
        ko.check(f"accum{accum}.hip.{name}", p.grad, _sum_spec(parts, False))
        ko.check(f"accum{accum}.blas.{name}", wb[name].grad,
                 _sum_spec(parts, True))
    # nothing else moved
    for (n, a), (_, b) in zip(tb.module.named_parameters(),
                              th.module.named_parameters()):
        if n not in wh:
            assert torch.equal(a.grad, b.grad), n


def test_graph_step_equals_eager_step(monkeypatch):
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    tg = _trainer(hip_graph=True)
    tg.train_step(sync=False)        # two warm-up steps and one replay
    te = _trainer(clip_on_device=True)
    while te.step_count < tg.step_count:
        te.train_step(sync=False)
    for a, b in zip(tg.fb.buckets, te.fb.buckets):
        assert torch.equal(a.flat_grad, b.flat_grad)
        assert torch.equal(a.flat_param, b.flat_param)


def test_post_accumulate_hook_still_fires(monkeypatch):
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    calls = _record(monkeypatch)
    tr = _trainer()
    name, w = next(iter(_linear_weights(tr).items()))
    fired = []
    w.register_post_accumulate_grad_hook(lambda p: fired.append(1))
    tr.train_step()
    assert fired == [1]
    fresh = [c for c in calls if not c[4]]
    assert len(fresh) == 1                   # that weight alone
    dy, x = fresh[0][0], fresh[0][1]
    assert tuple(fresh[0][3].shape) == tuple(w.shape)
    ko.check(f"hook.{name}", w.grad, kg.wgrad(dy, x))

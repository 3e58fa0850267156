"""Clip / LR-schedule / accumulation knobs of the training step, CPU tier.

The torch fallbacks of grad_sumsq_ / grad_norm_finalize_ are the oracle of
the HIP kernels, so they are checked against fp64 here; the trainer checks
run the fp32 CPU trainer through the same step code the GPU uses.
"""
import json

import numpy as np
import pytest
import torch

from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext

U = 2.0 ** -24  # fp32 unit roundoff
CPU = torch.device("cpu")


def _cfg(**kw):
    base = dict(model="llama-tiny", micro_batch=1, seq_len=32, dtype="fp32",
                grad_accum_steps=2)
    base.update(kw)
    return TrainerConfig(**base)


def test_grad_sumsq_blocks_geometry():
    # one slot per 256 threads x 8 elements, capped at 2048 blocks
    assert ops.grad_sumsq_blocks(8) == 1
    assert ops.grad_sumsq_blocks(2048) == 1
    assert ops.grad_sumsq_blocks(2048 + 8) == 2
    assert ops.grad_sumsq_blocks(2048 * 2048) == 2048
    assert ops.grad_sumsq_blocks(1 << 30) == 2048


@pytest.mark.parametrize("n", [8, 1032])
def test_sumsq_fallback_vs_fp64(n):
    """Every slot is written and the slots add up to sum(g^2). Bound: each
    square rounds once and a fp32 sum of n positive terms is off by at
    most (n-1) roundings whatever its order, so (n+1)*2^-24 relative."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    part = torch.full((ops.grad_sumsq_blocks(n) + 2,), float("nan"))
    ops.grad_sumsq_(g, part)
    assert torch.isfinite(part).all()      # no slot left unwritten
    ref = g.double().pow(2).sum().item()
    got = part.double().sum().item()
    assert abs(got - ref) <= (n + 1) * U * ref


@pytest.mark.parametrize("clip", [0.25, 1e9, 0.0])
def test_finalize_fallback_vs_fp64(clip):
    """norm = sqrt(sum)*inv, gscale = inv*min(1, clip/(norm+1e-6)) against
    fp64. P partials summed in fp32: <= (P-1) roundings, halved by the
    sqrt; then sqrt, two multiplies, an add and a divide round once each
    (and inv_count itself is rounded to fp32) -> (P + 8) * 2^-24."""
    part = torch.tensor([3.0, 0.5, 7.25, 1e-3, 11.0])
    inv = 1.0 / 6.0
    out = torch.zeros(2)
    ops.grad_norm_finalize_(part, out, inv_count=inv, clip=clip)
    norm = float(np.sqrt(part.double().sum().item())) * inv
    coef = min(1.0, clip / (norm + 1e-6)) if clip > 0 else 1.0
    tol = (len(part) + 8) * U
    assert abs(out[0].item() - norm) <= tol * norm
    assert abs(out[1].item() - inv * coef) <= tol * inv * coef
    if clip == 0.25:
        assert coef < 1.0                   # this case does clip
    else:
        # inactive clip: exactly the fp32 average factor
        assert out[1].item() == float(np.float32(inv))


def test_two_buckets_one_finalize():
    """One finalize over the concatenated partials of two buckets."""
    gen = torch.Generator().manual_seed(5)
    g1, g2 = torch.randn(64, generator=gen), torch.randn(4104, generator=gen)
    s1, s2 = ops.grad_sumsq_blocks(64), ops.grad_sumsq_blocks(4104)
    ws = torch.zeros(s1 + s2)
    p1, p2 = ws.split([s1, s2])
    ops.grad_sumsq_(g1, p1)
    ops.grad_sumsq_(g2, p2)
    out = torch.zeros(2)
    ops.grad_norm_finalize_(ws, out, inv_count=1.0, clip=0.0)
    ref = float(np.sqrt(g1.double().pow(2).sum().item() +
                        g2.double().pow(2).sum().item()))
    n = 64 + 4104
    assert abs(out[0].item() - ref) <= (n + 8) * U * ref


def test_adamw_fallback_device_scalars_match_host_args():
    gen = torch.Generator().manual_seed(1)
    p0, g = torch.randn(64, generator=gen), torch.randn(64, generator=gen)
    lr, gs = 3e-3, 0.37
    res = []
    for dev in (False, True):
        p, m, v = p0.clone(), torch.zeros(64), torch.zeros(64)
        kw = dict(lr_dev=torch.tensor(lr), gscale_dev=torch.tensor([gs])) \
            if dev else {}
        ops.fused_adamw_(
            p, g, m, v, lr=float(np.float32(lr)) if not dev else 99.0,
            beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=1,
            grad_scale=float(np.float32(gs)) if not dev else 99.0, **kw)
        res.append((p, m, v))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _probe_norm():
    """Norm of the averaged grads of step 1 (clipping off)."""
    tr = Trainer(_cfg(), DistContext(device=CPU))
    tr.train_step()
    return (tr.fb.grad_norm() / 2).item()


def test_trainer_device_clip_matches_host_clip():
    """Same seed -> same grads at step 1; the device path must hand AdamW
    the gscale the host path computes, to rel 1e-6 (a handful of fp32
    operations apart). grad_clip is half the probed norm, so the clip is
    active (coef ~ 0.5)."""
    norm0 = _probe_norm()
    clip = 0.5 * norm0
    ctx = DistContext(device=CPU)

    host = Trainer(_cfg(grad_clip=clip), ctx)
    seen = {}
    real = host.opt.step

    def spy(grad_scale=None, lr=None):
        seen["scale"] = grad_scale
        return real(grad_scale=grad_scale, lr=lr)

    host.opt.step = spy
    host.train_step()

    dev = Trainer(_cfg(grad_clip=clip, clip_on_device=True), ctx)
    dev.train_step()
    gscale = dev.fb.norm_out[1].item()

    inv = 1.0 / 2  # world 1, accum 2
    assert seen["scale"] < 0.75 * inv       # clip really active
    assert gscale == pytest.approx(seen["scale"], rel=1e-6)
    assert dev.last_grad_norm().item() == pytest.approx(norm0, rel=1e-6)
    # and the same update came out of it
    for a, b in zip(host.fb.buckets, dev.fb.buckets):
        assert torch.allclose(a.flat_param, b.flat_param, rtol=0, atol=1e-6)


def test_trainer_device_clip_inactive_is_exact_average():
    tr = Trainer(_cfg(grad_clip=1e9, clip_on_device=True),
                 DistContext(device=CPU))
    tr.train_step()
    assert tr.fb.norm_out[1].item() == float(np.float32(1.0 / 2))


def test_device_clip_off_leaves_step_signature():
    """clip_on_device=False: opt.step is still called as
    step(grad_scale=, lr=) and no workspace exists."""
    tr = Trainer(_cfg(grad_clip=0.5), DistContext(device=CPU))
    assert tr.fb.norm_out is None
    calls = []
    real = tr.opt.step
    tr.opt.step = lambda grad_scale=None, lr=None: (
        calls.append(1), real(grad_scale=grad_scale, lr=lr))[1]
    tr.train_step()
    assert calls == [1]


def test_hip_graph_accepts_clip_schedule_accum():
    """The configuration itself is accepted: on a CPU context construction
    now gets as far as the device check and stops there."""
    cfg = _cfg(hip_graph=True, grad_clip=1.0, lr_warmup_steps=2,
               grad_accum_steps=2)
    with pytest.raises(AssertionError, match="needs a GPU"):
        Trainer(cfg, DistContext(device=CPU))


def test_metrics_carry_grad_norm_and_lr(tmp_path):
    path = str(tmp_path / "m.json")
    tr = Trainer(_cfg(grad_clip=1.0, clip_on_device=True, lr=1e-3,
                      lr_warmup_steps=4, metrics_path=path),
                 DistContext(device=CPU))
    tr.train_step()
    rec = json.load(open(path))
    assert rec["lr"] == pytest.approx(1e-3 / 4)
    assert rec["grad_norm"] == pytest.approx(
        (tr.fb.grad_norm() / 2).item(), rel=1e-6)

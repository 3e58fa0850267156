"""The captured (hip_graph) training step with grad clip, LR schedule and
gradient accumulation, on llama-tiny.

A fresh graph trainer's first train_step() runs three optimizer steps (two
real warm-up steps on a side stream, then the first replay), so the runs
below are lined up by step_count, not by number of calls.
"""
import math

import numpy as np
import pytest
import torch

from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ACCUM = 2


def _trainer(**kw):
    torch.cuda.set_device(0)
    cfg = TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=128, **kw)
    return Trainer(cfg, DistContext(device=torch.device("cuda", 0)))


def _knobs(clip):
    # the schedule's peak is TrainerConfig.lr, the LR of the plain runs
    return dict(grad_clip=clip, lr_warmup_steps=2, lr_decay_steps=6,
                grad_accum_steps=ACCUM)


def _run_to(tr, step):
    losses = []
    while tr.step_count < step:
        losses.append(tr.train_step(sync=False).clone())
    assert tr.step_count == step
    return losses


def _params(tr):
    return [b.flat_param.clone() for b in tr.fb.buckets]


def _max_diff(pa, pb):
    return max((a.float() - b.float()).abs().max().item()
               for a, b in zip(pa, pb))


def _lr_of_step(tr, step):
    """The schedule's LR for optimizer step `step` (1-based)."""
    saved = tr.step_count
    tr.step_count = step - 1
    try:
        return tr.current_lr()
    finally:
        tr.step_count = saved


def _record_lrs(tr):
    """Log the host LR of every step the trainer stages (warm-up steps
    included)."""
    log = []
    real = tr._stage_step

    def staged():
        real()
        log.append(tr._last_lr)

    tr._stage_step = staged
    return log


def _norm_rel_tol(tr):
    """Bound of the device norm for this model's buckets; derivation in
    test_grad_norm_gpu.py (adds on the longest chain of each kernel, sqrt
    halves, +3 single roundings, safety factor 2)."""
    d_sumsq = 0
    for b in tr.fb.buckets:
        k = math.ceil((b.numel // 8) / (256 * ops.grad_sumsq_blocks(b.numel)))
        d_sumsq = max(d_sumsq, 8 * math.ceil(k / 4) + 2 + 6 + 3)
    slots = sum(ops.grad_sumsq_blocks(b.numel) for b in tr.fb.buckets)
    d_fin = math.ceil(slots / 1024) + 6 + 15
    return 2 * ((d_sumsq + d_fin) / 2 + 3) * U


def _check_norm(tr):
    """Device norm of the step just run vs the grads still in the buckets:
    fp64 within the kernel bound; fb.grad_norm() (itself an fp32 sum with
    an error of its own) within twice that."""
    tol = _norm_rel_tol(tr)
    got = tr.last_grad_norm().item()
    ref64 = math.sqrt(sum(b.flat_grad.double().pow(2).sum().item()
                          for b in tr.fb.buckets)) / ACCUM
    ref32 = tr.fb.grad_norm().item() / ACCUM
    print(f"step {tr.step_count}: norm {got:.6e} rel err vs fp64 "
          f"{abs(got - ref64) / ref64:.2e} tol {tol:.2e}")
    assert abs(got - ref64) <= tol * ref64
    assert abs(got - ref32) <= 2 * tol * ref32
    # clip is active: gscale well below the plain average factor
    assert tr.fb.norm_out[1].item() < 0.75 / ACCUM


@pytest.fixture(scope="module")
def clip():
    """Half the grad norm of step 1, probed with clipping off."""
    tr = _trainer(grad_accum_steps=ACCUM)
    tr.train_step()
    return 0.5 * tr.fb.grad_norm().item() / ACCUM


@pytest.fixture(scope="module")
def graph_run(clip, tmp_path_factory):
    """The uninterrupted graph run with all knobs: checked after every
    call, checkpointed at step 3, params kept at steps 5 and 6."""
    tr = _trainer(hip_graph=True, **_knobs(clip))
    lrs = _record_lrs(tr)
    ck = str(tmp_path_factory.mktemp("ck") / "step3")
    run = {"losses": [], "params": {}, "lrs": lrs, "ck": ck, "checks": []}
    while tr.step_count < 6:
        run["losses"].append(tr.train_step(sync=False).clone())
        step = tr.step_count
        run["checks"].append(
            (step, tr._lr_dev.item(), _lr_of_step(tr, step)))
        _check_norm(tr)
        if step == 3:
            tr.save_checkpoint(ck)
        if step in (5, 6):
            run["params"][step] = _params(tr)
    return run


def test_device_lr_after_each_replay(graph_run):
    assert [c[0] for c in graph_run["checks"]] == [3, 4, 5, 6]
    for step, lr_dev, lr_host in graph_run["checks"]:
        assert lr_dev == float(np.float32(lr_host)), step
    # the schedule really moved: warm-up, peak, decay
    lrs = graph_run["lrs"]
    assert len(lrs) == 6 and lrs[0] < lrs[1] and lrs[5] < lrs[2]


def test_two_graph_trainers_bit_equal(graph_run, clip):
    tr = _trainer(hip_graph=True, **_knobs(clip))
    losses = _run_to(tr, 5)
    for a, b in zip(graph_run["params"][5], _params(tr)):
        assert torch.equal(a, b)
    assert len(losses) == 3
    for a, b in zip(graph_run["losses"], losses):
        assert torch.equal(a, b)


def test_graph_matches_eager_as_closely_as_before(graph_run, clip):
    """Calibrated: d_plain is what graph-vs-eager differ by after 5 steps
    with no knobs (both paths predate the knobs); graph-vs-eager with the
    knobs may differ by at most twice that (0 demands bit equality)."""
    g0 = _trainer(hip_graph=True)
    e0 = _trainer()
    _run_to(g0, 5)
    _run_to(e0, 5)
    d_plain = _max_diff(_params(g0), _params(e0))
    del g0, e0

    e1 = _trainer(clip_on_device=True, **_knobs(clip))
    e1.train_step()
    _check_norm(e1)                 # step 1, same state as the probe
    _run_to(e1, 5)
    d_knobs = _max_diff(graph_run["params"][5], _params(e1))
    print(f"d_plain {d_plain:.3e}  d_knobs {d_knobs:.3e}")
    assert d_knobs <= 2 * d_plain


def test_resume_from_checkpoint_continues_identically(graph_run, clip):
    """Load the step-3 checkpoint into a fresh graph trainer. Its first
    call runs steps 4..6 (two warm-up steps, one replay): same LR sequence
    and the same params as the uninterrupted run at step 6."""
    tr = _trainer(hip_graph=True, **_knobs(clip))
    tr.load_checkpoint(graph_run["ck"])
    assert tr.step_count == 3
    lrs = _record_lrs(tr)
    tr.train_step(sync=False)
    assert tr.step_count == 6
    assert lrs == graph_run["lrs"][3:6]
    assert tr._lr_dev.item() == float(np.float32(_lr_of_step(tr, 6)))
    for a, b in zip(graph_run["params"][6], _params(tr)):
        assert torch.equal(a, b)

"""GPU tests of the on-device grad norm (grad_sumsq_ + grad_norm_finalize_)
and of AdamW's device-scalar lr / grad scale.

Tolerance of the norm, derived from the kernels' structure (u = 2^-24):

  * a bf16 value has 8 significant bits, so each square is exact in fp32
    and only additions round. All terms are >= 0, so a sum whose longest
    chain of additions has depth d is within d*u (first order) of exact.
  * sumsq kernel, bucket of nvec 16-byte vectors on B blocks of 256
    threads: the busiest thread reads k = ceil(nvec / (256*B)) vectors,
    dealt round-robin to 4 accumulators -> 8*ceil(k/4) fused adds on one
    accumulator, +2 to join the four, +6 for the 64-lane butterfly, +3 for
    the four waves of the block.
  * finalize kernel, P partials on 1024 threads: ceil(P/1024) adds per
    thread, +6 butterfly, +15 for the sixteen waves.
  * sqrt halves the relative error of the sum and rounds once; the
    multiply by inv_count rounds once, inv_count itself once -> +3.
    gscale adds an add, a divide and a multiply -> +3 more.

  rel(norm) <= (d_sumsq + d_finalize)/2 * u + 3u, times a safety factor 2
  for second-order terms. For the sizes below that is about 3e-6 (every
  case has ceil(k/4) = 1; a 256 MB bucket would have ceil(k/4) = 8).
"""
import math

import pytest
import torch

from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 2048
# just past three whole grid sweeps, ragged tail of 37 vectors (~12.6M)
BIG = 3 * CAP * 256 * 8 + 8 * 37

CASES = {
    "one_vector": [8],
    "two_blocks_ragged": [4096 + 8],
    "past_grid_sweep": [BIG],
    "two_buckets": [4096 + 8, 64 * 1000],
}


def dev():
    return torch.device("cuda", 0)


def norm_rel_tol(sizes):
    d_sumsq = 0
    for n in sizes:
        k = math.ceil((n // 8) / (256 * ops.grad_sumsq_blocks(n)))
        d_sumsq = max(d_sumsq, 8 * math.ceil(k / 4) + 2 + 6 + 3)
    slots = sum(ops.grad_sumsq_blocks(n) for n in sizes)
    d_fin = math.ceil(slots / 1024) + 6 + 15
    return 2 * ((d_sumsq + d_fin) / 2 + 3) * U


@pytest.fixture(scope="module")
def inputs():
    """bf16 buckets per case + the fp64 sum of squares of the quantized
    values (computed once, never modified)."""
    gen = torch.Generator(device="cuda").manual_seed(7)
    out = {}
    for name, sizes in CASES.items():
        gs = [(torch.randn(n, device=dev(), generator=gen) *
               (0.02 * (i + 1))).bfloat16() for i, n in enumerate(sizes)]
        ref = sum(g.double().pow(2).sum().item() for g in gs)
        out[name] = (gs, ref)
    return out


def run_norm(gs, inv_count, clip):
    slots = [ops.grad_sumsq_blocks(g.numel()) for g in gs]
    ws = torch.full((sum(slots),), float("nan"), device=dev())
    for g, part in zip(gs, ws.split(slots)):
        ops.grad_sumsq_(g, part)
    out = torch.zeros(2, device=dev())
    ops.grad_norm_finalize_(ws, out, inv_count=inv_count, clip=clip)
    return ws, out


def test_python_geometry_matches_extension():
    assert ops._C.grad_sumsq_max_blocks() == CAP
    for n in (8, 2048, 2056, 4104, CAP * 2048, BIG, 1 << 31):
        assert ops.grad_sumsq_blocks(n) == ops._C.grad_sumsq_blocks(n)


@pytest.mark.parametrize("name", list(CASES))
def test_norm_and_gscale_vs_fp64(inputs, name):
    gs, ref = inputs[name]
    inv = 1.0 / 6.0
    norm_ref = math.sqrt(ref) * inv
    clip = 0.5 * norm_ref                       # active: coef ~ 0.5
    ws, out = run_norm(gs, inv, clip)
    assert torch.isfinite(ws).all()             # every slot written
    tol = norm_rel_tol(CASES[name])
    norm, gscale = out.tolist()
    print(f"{name}: rel err norm {abs(norm - norm_ref) / norm_ref:.3e} "
          f"tol {tol:.3e}")
    assert abs(norm - norm_ref) <= tol * norm_ref
    gscale_ref = inv * min(1.0, clip / (norm_ref + 1e-6))
    assert gscale_ref < 0.75 * inv
    assert abs(gscale - gscale_ref) <= (tol + 3 * U) * gscale_ref

    # inactive clip: exactly the fp32 averaging factor
    _, out2 = run_norm(gs, inv, 1e9)
    assert out2[1].item() == torch.tensor(inv).item()
    assert out2[0].item() == norm


@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_repeatable(inputs, name):
    gs, _ = inputs[name]
    ws1, out1 = run_norm(gs, 0.5, 1.0)
    ws2, out2 = run_norm(gs, 0.5, 1.0)
    assert torch.equal(ws1, ws2)
    assert torch.equal(out1, out2)


def test_nonfinite_norm_propagates():
    """As on the host path (torch.clamp keeps NaN): a NaN gradient must
    not turn into 'no clip'."""
    g = torch.ones(64, device=dev()).bfloat16()
    g[5] = float("nan")
    _, out = run_norm([g], 1.0, 1.0)
    assert math.isnan(out[0].item()) and math.isnan(out[1].item())


def test_rejects_wrong_workspace():
    g = torch.ones(64, device=dev()).bfloat16()
    with pytest.raises(RuntimeError):
        ops.grad_sumsq_(g, torch.zeros(CAP + 1, device=dev()))
    with pytest.raises(RuntimeError):
        ops.grad_sumsq_(g.float(), torch.zeros(1, device=dev()))
    with pytest.raises(RuntimeError):
        ops.grad_norm_finalize_(torch.zeros(4, device=dev()),
                                torch.zeros(1, device=dev()),
                                inv_count=1.0, clip=1.0)


@pytest.mark.parametrize("use_step_dev", [False, True])
def test_adamw_device_scalars_bit_identical(use_step_dev):
    """lr_dev / gscale_dev holding float32(lr) / float32(gscale) give the
    very bits the host arguments give; the host twins are ignored."""
    torch.manual_seed(0)
    n = 4096 + 8
    p0 = torch.randn(n).bfloat16().to(dev())
    g = torch.randn(n).bfloat16().to(dev())
    lr, gs = 1e-2, 0.37
    res = []
    for on_dev in (False, True):
        p = p0.clone()
        m = torch.zeros(n, device=dev())
        v = torch.zeros(n, device=dev())
        sd = torch.zeros((), dtype=torch.int32, device=dev()) \
            if use_step_dev else None
        kw = {}
        if on_dev:
            pair = torch.tensor([lr, gs], device=dev())
            kw = dict(lr_dev=pair[:1], gscale_dev=pair[1:])
        for step in range(1, 4):
            if sd is not None:
                sd += 1
            ops.fused_adamw_(p, g, m, v, lr=99.0 if on_dev else lr,
                             beta1=0.9, beta2=0.95, eps=1e-8,
                             weight_decay=0.1, step=step,
                             grad_scale=99.0 if on_dev else gs,
                             step_dev=sd, **kw)
        res.append((p, m, v))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], p0)       # it did update

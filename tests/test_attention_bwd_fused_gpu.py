"""GPU numerics: fused dK+dV attention backward (64 keys per wave) and the
split dV / dK pair it replaces, each against the fp32 reference.

Reference = ops.attention_ref in fp32 on bf16-quantised inputs, tolerance
as in test_attention_gpu.py: err < 0.04 * max(1, |g_ref|max) per gradient.
Every case runs through both backward paths; both must meet the reference
and every output must be finite. The shapes are the smallest at which the
fused kernel's block / wave / key-half / q-tile boundaries are all hit.
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

CASES = [
    # two key blocks; the second has one live wave whose second 32-key
    # half is ragged (keys 320-327) and three waves with no keys; rep = 4
    (1, 328, 4, 1, 128, True),
    # three key blocks; diagonal subtile skip in every wave position;
    # B > 1; S % 64 == 0 but S % 256 != 0
    (2, 576, 8, 2, 128, True),
    # D = 64; non-causal (no skip, every q tile visited); ragged tail of 8
    (1, 264, 2, 2, 64, False),
    # S smaller than one wave-pair's keys; padded q rows exercise the
    # row-constant padding
    (1, 96, 2, 1, 128, True),
]
SPIKED = (1, 328, 2, 2, 128, True)


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def problem(B, S, Hq, Hkv, D, causal, spiked=False):
    """Inputs and fp32 reference gradients, computed once per shape."""
    torch.manual_seed(3)
    q = (torch.randn(B, S, Hq, D) * 0.5).bfloat16().float()
    k = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    v = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    do = (torch.randn(B, S, Hq, D) * 0.5).bfloat16().float()
    if spiked:
        # backward analogue of the spiked-softmax forward test: a large
        # lse lands in the S accumulator's start value
        k[0, 300] *= 30.0
        q[0, 310] *= 8.0
    qr = q.clone().requires_grad_(True)
    kr = k.clone().requires_grad_(True)
    vr = v.clone().requires_grad_(True)
    ops.attention_ref(qr, kr, vr, causal).float().backward(do)
    return (q, k, v, do), (qr.grad, kr.grad, vr.grad), \
        ka.of_floats(q, k, v, do, causal)


def check(case, split, spiked=False):
    causal = case[5]
    (q, k, v, do), refs, specs = problem(*case, spiked=spiked)
    qg, kg, vg, dog = (t.bfloat16().to(dev()) for t in (q, k, v, do))
    o, lse = ops._C.attn_fwd(qg, kg, vg, causal)
    grads = ops._C.attn_bwd(qg, kg, vg, o, lse, dog, causal, split)
    for name, g_hip, g_ref in zip(("dq", "dk", "dv"), grads, refs):
        g = g_hip.float().cpu()
        assert torch.isfinite(g).all(), f"{name} has non-finite values"
        err = (g - g_ref).abs().max().item()
        scale = max(1.0, g_ref.abs().max().item())
        print(f"{name} split={split} max err {err:.5f} (bound "
              f"{0.04 * scale:.5f})")
        assert err < 0.04 * scale, f"{name} max err {err} (scale {scale})"
    ka.check_all(f"bwd_fused_file.split={split}[{case},spiked={spiked}]",
                 dict(zip(("dq", "dk", "dv"), grads)), specs)


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
@pytest.mark.parametrize("B,S,Hq,Hkv,D,causal", CASES)
def test_attn_backward_paths(B, S, Hq, Hkv, D, causal, split):
    check((B, S, Hq, Hkv, D, causal), split)


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_attn_backward_spiked(split):
    check(SPIKED, split, spiked=True)


def test_default_backward_is_fused():
    """The autograd path (no selector) runs the fused kernel: its dk/dv are
    bitwise those of an explicit split=False call."""
    case = CASES[3]
    causal = case[5]
    (q, k, v, do), _, _ = problem(*case)
    qg, kg, vg, dog = (t.bfloat16().to(dev()) for t in (q, k, v, do))
    o, lse = ops._C.attn_fwd(qg, kg, vg, causal)
    _, dk_f, dv_f = ops._C.attn_bwd(qg, kg, vg, o, lse, dog, causal, False)
    _, dk_d, dv_d = ops._C.attn_bwd(qg, kg, vg, o, lse, dog, causal)
    assert torch.equal(dk_f, dk_d) and torch.equal(dv_f, dv_d)

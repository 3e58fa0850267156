"""GPU numerics: the dQ kernels behind attn_bwd's dq_variant, each against
the fp32 reference: 0 = the 4-wave kernel (64 q rows per wave as two 32-row
halves), 1 = the 8-wave kernel in XCD-aware block order (the default),
2 = the 8-wave kernel in plain block order.

Reference and bound are those of test_attention_bwd_fused_gpu.py: fp32
ops.attention_ref on bf16-quantised inputs, err < 0.04 * max(1, |g_ref|max)
per gradient, every output finite. Every case runs through both variants.
The shapes are the smallest that hit the 4-wave kernel's block / wave / half
/ key-tile boundaries. The XCD-aware block order is a real permutation where
the block count is a multiple of 8 (dQ grids of 8, 16 and 48 blocks here,
and a fused dK+dV grid of 8 blocks in the last case) and the identity in
the other cases. max |dQ_v2 - dQ_old| is printed per case;
the element arithmetic and the key order of the sums are the same in all
kernels (measured: 0 in every case).
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

CASES = [
    # one block; wave 1 has a ragged upper half, waves 2-3 have no rows
    (1, 96, 2, 1, 128, True),
    # S smaller than one wave's 64 rows: 8 live rows in the upper half,
    # the single key tile is ragged; D = 64
    (1, 40, 2, 2, 64, True),
    # two q blocks; the key tail is 8 keys into a tile; rep = 4
    (1, 328, 4, 1, 128, True),
    # three q blocks, B > 1; the diagonal falls in every wave and half
    # position, including "upper half only"
    (2, 576, 8, 2, 128, True),
    # non-causal: every tile live for both halves; ragged tail
    (1, 264, 2, 2, 64, False),
    # 2 key blocks x 2 kv heads x 2 batches: the fused dK+dV kernel's grid
    # is 8 blocks, so its XCD-aware order permutes them (dQ grid: 16)
    (2, 264, 4, 2, 64, True),
]
SPIKED = (1, 328, 2, 2, 128, True)
VARIANTS = [0, 1, 2]
IDS = ["v2", "old-xcd", "old"]


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
        k[0, 300] *= 30.0
        q[0, 310] *= 8.0
    qr = q.clone().requires_grad_(True)
    kr = k.clone().requires_grad_(True)
    vr = v.clone().requires_grad_(True)
    ops.attention_ref(qr, kr, vr, causal).float().backward(do)
    return (q, k, v, do), (qr.grad, kr.grad, vr.grad), \
        ka.of_floats(q, k, v, do, causal)


@functools.lru_cache(maxsize=None)
def hip_grads(case, spiked, dq_variant):
    """(dq, dk, dv) of one case through one dQ variant; dq_variant None is
    the call without the selector."""
    causal = case[5]
    (q, k, v, do), _, _ = problem(*case, spiked=spiked)
    qg, kg, vg, dog = (t.bfloat16().to(dev()) for t in (q, k, v, do))
    o, lse = ops._C.attn_fwd(qg, kg, vg, causal)
    if dq_variant is None:
        return ops._C.attn_bwd(qg, kg, vg, o, lse, dog, causal)
    return ops._C.attn_bwd(qg, kg, vg, o, lse, dog, causal, False, dq_variant)


def check(case, dq_variant, spiked=False):
    _, refs, specs = problem(*case, spiked=spiked)
    grads = hip_grads(case, spiked, dq_variant)
    for name, g_hip, g_ref in zip(("dq", "dk", "dv"), grads, refs):
        g = g_hip.float().cpu()
        assert torch.isfinite(g).all(), f"{name} has non-finite values"
        err = (g - g_ref).abs().max().item()
        scale = max(1.0, g_ref.abs().max().item())
        print(f"{name} dq_variant={dq_variant} max err {err:.5f} (bound "
              f"{0.04 * scale:.5f})")
        assert err < 0.04 * scale, f"{name} max err {err} (scale {scale})"
    ka.check_all(f"bwd_dq_file.dq_variant={dq_variant}[{case},spiked={spiked}]",
                 dict(zip(("dq", "dk", "dv"), grads)), specs)


def check_variants_agree(case, spiked=False):
    dq_n, dk_n, dv_n = hip_grads(case, spiked, 0)
    for variant in (1, 2):
        dq_o, dk_o, dv_o = hip_grads(case, spiked, variant)
        diff = (dq_n.float() - dq_o.float()).abs().max().item()
        print(f"{case} spiked={spiked}: max |dQ_v2 - dQ_old| = {diff:.3e} "
              f"(dq_variant {variant})")
        # the dQ kernel must not touch dK and dV
        assert torch.equal(dk_n, dk_o) and torch.equal(dv_n, dv_o)


@pytest.mark.parametrize("dq_variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("B,S,Hq,Hkv,D,causal", CASES)
def test_attn_backward_dq_variants(B, S, Hq, Hkv, D, causal, dq_variant):
    check((B, S, Hq, Hkv, D, causal), dq_variant)


@pytest.mark.parametrize("dq_variant", VARIANTS, ids=IDS)
def test_attn_backward_dq_spiked(dq_variant):
    check(SPIKED, dq_variant, spiked=True)


@pytest.mark.parametrize("B,S,Hq,Hkv,D,causal", CASES)
def test_dk_dv_independent_of_dq_variant(B, S, Hq, Hkv, D, causal):
    check_variants_agree((B, S, Hq, Hkv, D, causal))


def test_dk_dv_independent_of_dq_variant_spiked():
    check_variants_agree(SPIKED, spiked=True)


def test_default_backward_dq():
    """The call without the selector (the autograd path) runs dq_variant 1.
    Its gradients are bitwise those of the explicit call, and bitwise those
    of dq_variant 0 as well: the dQ kernels differ in structure and block
    order, not in arithmetic."""
    case = CASES[3]
    for variant in (0, 1):
        for g_d, g_x in zip(hip_grads(case, False, None),
                            hip_grads(case, False, variant)):
            assert torch.equal(g_d, g_x)


def test_dq_variant_is_checked():
    case = CASES[0]
    (q, k, v, do), _, _ = problem(*case)
    qg, kg, vg, dog = (t.bfloat16().to(dev()) for t in (q, k, v, do))
    o, lse = ops._C.attn_fwd(qg, kg, vg, True)
    with pytest.raises(RuntimeError):
        ops._C.attn_bwd(qg, kg, vg, o, lse, dog, True, False, 7)

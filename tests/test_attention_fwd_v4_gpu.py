"""GPU numerics: the v4 attention forward (attn_fwd variant 0, the default)
and the v3 kernel it replaces (variant 1), each against the reference.

O: ops.attention_ref in fp32 on bf16-quantised inputs, bounds as in
test_attention_gpu.py (0.03 max-abs, 0.05 for the spiked inputs), and per
element the fp64 reference and rule of kernel_oracle_attention.py.

LSE: an fp64 logsumexp of the scaled, masked scores of the same inputs.
 * v3 (variant 1) must stay inside a worst-case fp32 bound: a score is a
   D-term fp32 sum and l an S-term one, so |err| <= (D + S) * 2^-24 *
   max(1, |score|max), with a floor of 1e-5 for the hardware log/exp.
 * v4 (variant 0) is judged per element by the rule of
   kernel_oracle_attention.py, as v3 is too; v4 is no longer measured
   against v3, which is itself a kernel under test.

The shapes are the smallest that reach each path of the kernel; see CASES.
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

CASES = [
    # one block, all four diagonal tiles, waves dropping out of strip_live
    (1, 256, 2, 2, 128, True),
    # two blocks, the second ragged: reversed block index; lanes with
    # kvg >= S and qrow >= S keep a -inf running max and must give no NaN
    (1, 320, 2, 1, 128, True),
    # D = 64 instantiations
    (1, 200, 2, 1, 64, True),
    (1, 128, 2, 2, 64, False),
    # GQA 4:1, batch stride, more than one block
    (2, 512, 8, 2, 128, True),
]
STRADDLE = (1, 256, 1, 1, 128, True)
SPIKED = (1, 256, 2, 2, 128, True)
BWD = (2, 512, 8, 2, 128, True)


def dev():
    return torch.device("cuda", 0)


def references(q, k, v, causal):
    """fp32 O reference, fp64 LSE reference [B,Hq,S], max |scaled score|."""
    B, S, Hq, D = q.shape
    rep = Hq // k.shape[2]
    o_ref = ops.attention_ref(q, k, v, causal).float()
    qd = q.double().permute(0, 2, 1, 3)
    kd = k.double().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    s = torch.matmul(qd, kd.transpose(-1, -2)) / (D ** 0.5)
    smax = s.abs().max().item()
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1),
                          float("-inf"))
    return o_ref, torch.logsumexp(s, dim=-1), smax


@functools.lru_cache(maxsize=None)
def problem(B, S, Hq, Hkv, D, causal, kind="random"):
    """bf16-exact inputs and their references, computed once per shape."""
    torch.manual_seed(2 if kind == "spiked" else 0)
    q = (torch.randn(B, S, Hq, D) * 0.5).bfloat16().float()
    k = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    v = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    if kind == "spiked":
        # the inputs of test_attn_spiked_softmax_branch: the running max
        # jumps at tile 3
        k[0, 230] *= 30.0
        q[0, 240] *= 8.0
        q, k = q.bfloat16().float(), k.bfloat16().float()
    elif kind == "straddle":
        # every q element 0.25, every element of key row j is c_j: scores
        # are exactly 2.828 * c_j. Tile 1 raises the max by 7.07 nats (the
        # defer path, P up to e^7), tile 2 by another 8.49 (the rescale
        # path); tile 3 stays level.
        c = torch.tensor([0.0, 2.5, 5.5, 5.5]).repeat_interleave(64)
        q = torch.full((B, S, Hq, D), 0.25)
        k = c.view(1, S, 1, 1).expand(B, S, Hkv, D).contiguous()
    return (q, k, v), references(q, k, v, causal), \
        ka.of_floats(q, k, v, None, causal)


def run_fwd(case, kind, variant):
    (q, k, v), _, _ = problem(*case, kind=kind)
    qg, kg, vg = (t.bfloat16().to(dev()) for t in (q, k, v))
    o, lse = ops._C.attn_fwd(qg, kg, vg, case[5], variant)
    return o.float().cpu(), lse.double().cpu()


def check(case, kind, variant, o_bound):
    B, S, Hq, Hkv, D, causal = case
    _, (o_ref, lse_ref, smax), specs = problem(*case, kind=kind)
    o, lse = run_fwd(case, kind, variant)
    assert torch.isfinite(o).all(), "O has non-finite values"
    assert torch.isfinite(lse).all(), "LSE has non-finite values"
    o_err = (o - o_ref).abs().max().item()
    lse_err = (lse - lse_ref).abs().max().item()
    fp32_bound = max(1e-5, (D + S) * 2.0 ** -24 * max(1.0, smax))
    print(f"variant {variant}: O err {o_err:.5f} (bound {o_bound}); LSE err "
          f"{lse_err:.3e} (v3 bound {fp32_bound:.3e})")
    assert o_err < o_bound, f"O max err {o_err}"
    if variant == 1:
        assert lse_err <= fp32_bound, f"LSE max err {lse_err} > {fp32_bound}"
    ka.check_all(f"fwd_v4_file.variant{variant}[{case},{kind}]",
                 {"o": o, "lse": lse}, specs)


@pytest.mark.parametrize("variant", [0, 1], ids=["v4", "v3"])
@pytest.mark.parametrize("B,S,Hq,Hkv,D,causal", CASES)
def test_attn_fwd_variants(B, S, Hq, Hkv, D, causal, variant):
    check((B, S, Hq, Hkv, D, causal), "random", variant, 0.03)


@pytest.mark.parametrize("variant", [0, 1], ids=["v4", "v3"])
def test_attn_fwd_threshold_straddle(variant):
    check(STRADDLE, "straddle", variant, 0.03)


@pytest.mark.parametrize("variant", [0, 1], ids=["v4", "v3"])
def test_attn_fwd_spiked(variant):
    check(SPIKED, "spiked", variant, 0.05)


def test_default_forward_is_v4():
    """ops.attention (no selector) runs variant 0: bitwise the same O."""
    (q, k, v), _, _ = problem(*CASES[1])
    qg, kg, vg = (t.bfloat16().to(dev()) for t in (q, k, v))
    o0, _ = ops._C.attn_fwd(qg, kg, vg, True, 0)
    assert torch.equal(ops.attention(qg, kg, vg, True), o0)


def test_attn_backward_through_v4():
    """The backward consumes the v4 forward's LSE, and dq's exponential is
    the folded exp2(fma()) form: gradients against the fp32 reference with
    the bound of test_attention_gpu.py."""
    B, S, Hq, Hkv, D, causal = BWD
    torch.manual_seed(1)
    q = (torch.randn(B, S, Hq, D) * 0.5).bfloat16().float()
    k = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    v = (torch.randn(B, S, Hkv, D) * 0.5).bfloat16().float()
    do = (torch.randn(B, S, Hq, D) * 0.5).bfloat16().float()
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ops.attention_ref(qr, kr, vr, causal).float().backward(do)
    qg, kg, vg = (t.bfloat16().to(dev()).requires_grad_(True)
                  for t in (q, k, v))
    ops.attention(qg, kg, vg, causal).backward(do.bfloat16().to(dev()))
    for name, g_hip, g_ref in [("dq", qg.grad, qr.grad),
                               ("dk", kg.grad, kr.grad),
                               ("dv", vg.grad, vr.grad)]:
        g = g_hip.float().cpu()
        assert torch.isfinite(g).all(), f"{name} has non-finite values"
        err = (g - g_ref).abs().max().item()
        scale = max(1.0, g_ref.abs().max().item())
        print(f"{name} max err {err:.5f} (bound {0.04 * scale:.5f})")
        assert err < 0.04 * scale, f"{name} max err {err} (scale {scale})"
    ka.check_all("bwd_through_v4",
                 {"dq": qg.grad, "dk": kg.grad, "dv": vg.grad},
                 ka.of_floats(q, k, v, do, causal))

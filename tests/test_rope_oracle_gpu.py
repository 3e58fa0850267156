"""RoPE and packed-QKV RoPE kernels vs fp64, forward and backward, at
D = 64 and 128, past their grid caps (4096 / 8192 blocks), with the 1-row
table of the decode step, and with a table longer than the sequence --
which must rotate batch element 1 by positions 0..S-1 like element 0, not
by S..2S-1. Rule, references and k: kernel_oracle.py."""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_rope(x, dy, cos, sin):
    xg = x.to(DEV).requires_grad_(True)
    y = ops.apply_rope(xg, cos.to(DEV), sin.to(DEV))
    y.backward(dy.to(DEV))
    return y.detach(), xg.grad


# B, S, H, D, table rows
@pytest.mark.parametrize("B,S,H,D,rows", [
    (2, 37, 3, 64, 37),
    (2, 37, 3, 128, 37),
    (2, 2056, 32, 128, 2056),   # 4112 blocks of work: the grid strides
    (4, 1, 2, 128, 1),          # decode: one position, 1-row table
    (4, 1, 2, 64, 1),
    (2, 37, 3, 64, 74),         # table of 2S rows
    (2, 37, 3, 128, 74),
])
def test_rope_vs_fp64(B, S, H, D, rows):
    cos, sin = ko.rope_table(rows, D)
    x, dy = ko.bf(B, S, H, D, seed=1), ko.bf(B, S, H, D, seed=2)
    y, dx = run_rope(x, dy, cos, sin)
    tag = f"rope[{B},{S},{H},{D};{rows}]"
    ko.check(tag + ".y", y, ko.rope(x, cos, sin, 1.0))
    ko.check(tag + ".dx", dx, ko.rope(dy, cos, sin, -1.0))
    if rows > S:   # same bits as with the table cut to its first S rows
        y2, dx2 = run_rope(x, dy, cos[:S].contiguous(), sin[:S].contiguous())
        assert torch.equal(y, y2) and torch.equal(dx, dx2)


def run_qkv(qkv, douts, cos, sin, Hq, Hkv, D):
    qg = qkv.to(DEV).requires_grad_(True)
    q, k, v = ops.qkv_rope(qg, cos.to(DEV), sin.to(DEV), Hq, Hkv, D)
    torch.autograd.backward([q, k, v], [d.to(DEV) for d in douts])
    return q.detach(), k.detach(), v.detach(), qg.grad


@pytest.mark.parametrize("B,S,Hq,Hkv,D,rows", [
    (2, 21, 4, 2, 64, 21),
    (2, 21, 4, 2, 128, 21),
    (2, 2064, 32, 16, 128, 2064),   # 8256 blocks of work: the grid strides
    (4, 1, 4, 2, 128, 1),           # decode
    (4, 1, 4, 2, 64, 1),
    (2, 21, 4, 2, 64, 42),          # table of 2S rows
    (2, 21, 4, 2, 128, 42),
])
def test_qkv_rope_vs_fp64(B, S, Hq, Hkv, D, rows):
    cos, sin = ko.rope_table(rows, D)
    qkv = ko.bf(B, S, (Hq + 2 * Hkv) * D, seed=1)
    douts = [ko.bf(B, S, h, D, seed=s)
             for h, s in ((Hq, 2), (Hkv, 3), (Hkv, 4))]
    q, k, v, dqkv = run_qkv(qkv, douts, cos, sin, Hq, Hkv, D)
    tag = f"qkv_rope[{B},{S},{Hq},{Hkv},{D};{rows}]"
    q_in, k_in, v_in = ko.qkv_split(qkv, Hq, Hkv, D)
    ko.check(tag + ".q", q, ko.rope(q_in, cos, sin))
    ko.check(tag + ".k", k, ko.rope(k_in, cos, sin))
    assert torch.equal(v.cpu(), v_in)            # v is a copy
    dq, dk, dv = ko.qkv_split(dqkv.cpu(), Hq, Hkv, D)
    ko.check(tag + ".dq", dq, ko.rope(douts[0], cos, sin, -1.0))
    ko.check(tag + ".dk", dk, ko.rope(douts[1], cos, sin, -1.0))
    assert torch.equal(dv, douts[2])
    if rows > S:
        again = run_qkv(qkv, douts, cos[:S].contiguous(),
                        sin[:S].contiguous(), Hq, Hkv, D)
        for a, b in zip((q, k, v, dqkv), again):
            assert torch.equal(a, b)


def test_rope_tables_shorter_than_the_sequence_are_rejected():
    B, S, H, D = 2, 8, 2, 64
    x = ko.bf(B, S, H, D, seed=1).to(DEV)
    for rows in (1, 4, 7):       # 1 and 4 divide S: accepted before
        cos, sin = (t.to(DEV) for t in ko.rope_table(rows, D))
        with pytest.raises(RuntimeError, match="rope table"):
            ops._C.rope(x, cos, sin, H, 1.0)
        qkv = ko.bf(B, S, 4 * D, seed=2).to(DEV)
        with pytest.raises(RuntimeError, match="rope table"):
            ops._C.qkv_rope_fwd(qkv, cos, sin, 2, 1, D)
        with pytest.raises(RuntimeError, match="rope table"):
            ops._C.qkv_rope_bwd(x, x[:, :, :1].contiguous(),
                                x[:, :, :1].contiguous(), cos, sin)

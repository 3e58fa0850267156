"""qkv_rope_append_paged_ against ops.qkv_rope_append_chunk_ on a contiguous
bf16 cache on the same device: q is bitwise equal, the pool rows at the
logical positions are bitwise the contiguous cache's rows, and every other
pool byte keeps its sentinel. pos 62 crosses a page boundary, -1 has a dead
first token, 250 ends two rows short of the table's end (64 * NP = 256),
sequence 4 has qlens 0, and sequence 5's tokens (130 .. 132, table entry
130 // 64 = 2) find entries 1 and 2 out of range: dead, zero q."""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, NP, P = 6, 4, 26
POS, QLENS = [62, 0, -1, 250, 64, 130], [5, 5, 5, 5, 0, 3]
TABLE = [[(11 * (NP * b + j) + 5) % P for j in range(NP)] for b in range(B)]
TABLE[5][1], TABLE[5][2] = -1, P + 5
SENT = 0x5A5B


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("Tq", [1, 5])
def test_paged_append_equals_contiguous(Tq, Hq, Hkv, D):
    W = (Hq + 2 * Hkv) * D
    qkv = ko.bf(B * Tq, W, seed=11).view(B, Tq, W).to(DEV)
    cos, sin = (t.to(DEV) for t in ko.rope_table(64 * NP, D))
    i32 = dict(dtype=torch.int32, device=DEV)
    pos, qlens = torch.tensor(POS, **i32), torch.tensor(QLENS, **i32)
    sent = dict(dtype=torch.int16, device=DEV)
    kc = torch.full((B, 64 * NP, Hkv, D), SENT, **sent).view(torch.bfloat16)
    vc = kc.clone()
    want_q = ops.qkv_rope_append_chunk_(qkv, cos, sin, pos, qlens, kc, vc, Hq,
                                        Hkv, D)
    want_q[5] = 0
    kp = torch.full((P, Hkv, 64, D), SENT, **sent).view(torch.bfloat16)
    vp = kp.clone()
    want_k, want_v = kp.clone(), vp.clone()
    n_live = 0
    for b in range(B):
        for i in range(min(QLENS[b], Tq)):
            p = POS[b] + i
            if 0 <= p < 64 * NP and 0 <= TABLE[b][p // 64] < P:
                want_k[TABLE[b][p // 64], :, p % 64] = kc[b, p]
                want_v[TABLE[b][p // 64], :, p % 64] = vc[b, p]
                n_live += 1
    assert n_live == (5 + 5 + 4 + 5 if Tq == 5 else 3)
    q = ops.qkv_rope_append_paged_(qkv, cos, sin, pos, qlens, kp, vp,
                                   torch.tensor(TABLE, **i32), Hq, Hkv, D)
    assert q.shape == (B, Tq, Hq, D)
    assert torch.equal(q.view(torch.int16), want_q.view(torch.int16))
    assert torch.equal(kp.view(torch.int16), want_k.view(torch.int16))
    assert torch.equal(vp.view(torch.int16), want_v.view(torch.int16))

"""qkv_rope_append_ on the GPU: q and the appended k row pass the RoPE
rule at each sequence's own position, v is a bitwise copy, EVERY other
cache row keeps its sentinel, and a position outside [0, Tmax) writes
nothing and returns a zero q row."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ragged as kr
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_SENT, V_SENT = 3.0, -5.0


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 2, 128)])
def test_qkv_rope_append_vs_fp64(Hq, Hkv, D):
    B, Tmax, pos = 4, 9, [0, 8, 5, -1]
    qkv = ko.bf(B, (Hq + 2 * Hkv) * D, seed=5)
    cos, sin = ko.rope_table(Tmax + 3, D)
    pt = torch.tensor(pos, dtype=torch.int32)
    kc = torch.full((B, Tmax, Hkv, D), K_SENT, dtype=torch.bfloat16,
                    device=DEV)
    vc = torch.full((B, Tmax, Hkv, D), V_SENT, dtype=torch.bfloat16,
                    device=DEV)
    q = ops.qkv_rope_append_(qkv.to(DEV), cos.to(DEV), sin.to(DEV),
                             pt.to(DEV), kc, vc, Hq, Hkv, D)
    assert q.shape == (B, Hq, D) and q.dtype == torch.bfloat16
    q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()

    specs, live = kr.qkv_rope_append(qkv, cos, sin, pt, Tmax, Hq, Hkv, D)
    rows = torch.nonzero(live).flatten()
    at = pt.long()[rows]
    ko.check_all(f"append[{Hq}/{Hkv},D={D}]",
                 {"q": q, "k": kc[rows, at]}, specs)
    v_in = qkv.view(B, Hq + 2 * Hkv, D)[:, Hq + Hkv:]
    assert torch.equal(vc[rows, at], v_in[rows])

    untouched = torch.ones(B, Tmax, dtype=torch.bool)
    untouched[rows, at] = False
    assert int(untouched.sum()) == B * Tmax - 3
    assert (kc[untouched] == K_SENT).all()
    assert (vc[untouched] == V_SENT).all()
    # the pos = -1 sequence changed nothing and got zeros
    assert (kc[3] == K_SENT).all() and (vc[3] == V_SENT).all()
    assert (q[3] == 0).all()

    # a wrong position is seen
    bad, _ = kr.qkv_rope_append(qkv, cos, sin, pt, Tmax, Hq, Hkv, D,
                                pos_shift=1)
    assert sorted(ko.violates({"q": q, "k": kc[rows, at]}, bad)) == \
        ["k", "q"]

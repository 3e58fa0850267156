"""qkv_rope_append_chunk_ on the GPU: q and the live k rows pass the RoPE
rule at pos[b] + i (kernel_oracle_ragged.qkv_rope_append over the tokens as
a flat batch, a dead token handed to it as position -1), v is a bitwise
copy, every other cache row keeps its sentinel, and the sequence that runs
off the cache end writes only the rows that exist."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ragged as kr
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_SENT, V_SENT = 3.0, -5.0


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 2, 128)])
def test_qkv_rope_append_chunk_vs_fp64(Hq, Hkv, D):
    B, Tq, Tmax = 3, 5, 11
    pos, qlens = [0, 7, Tmax - 2], [5, 3, 5]
    W = (Hq + 2 * Hkv) * D
    qkv = ko.bf(B * Tq, W, seed=7)
    cos, sin = ko.rope_table(Tmax + 3, D)
    kc = torch.full((B, Tmax, Hkv, D), K_SENT, dtype=torch.bfloat16,
                    device=DEV)
    vc = torch.full((B, Tmax, Hkv, D), V_SENT, dtype=torch.bfloat16,
                    device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    q = ops.qkv_rope_append_chunk_(
        qkv.view(B, Tq, W).to(DEV), cos.to(DEV), sin.to(DEV),
        torch.tensor(pos, **i32), torch.tensor(qlens, **i32), kc, vc, Hq, Hkv,
        D)
    assert q.shape == (B, Tq, Hq, D) and q.dtype == torch.bfloat16
    q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()

    i = torch.arange(Tq).view(1, Tq)
    flat = torch.where(i < torch.tensor(qlens).view(B, 1),
                       torch.tensor(pos).view(B, 1) + i, -1).reshape(-1)
    specs, live = kr.qkv_rope_append(qkv, cos, sin, flat, Tmax, Hq, Hkv, D)
    assert int(live.sum()) == 5 + 3 + 2
    rows = torch.nonzero(live).flatten()
    bi, at = rows // Tq, flat[rows]
    ko.check_all(f"append_chunk[{Hq}/{Hkv},D={D}]",
                 {"q": q.view(B * Tq, Hq, D), "k": kc[bi, at]}, specs)
    v_in = qkv.view(B * Tq, Hq + 2 * Hkv, D)[:, Hq + Hkv:]
    assert torch.equal(vc[bi, at], v_in[rows])
    assert (q.view(B * Tq, Hq, D)[~live] == 0).all()

    untouched = torch.ones(B, Tmax, dtype=torch.bool)
    untouched[bi, at] = False
    assert int(untouched.sum()) == B * Tmax - 10
    assert (kc[untouched] == K_SENT).all()
    assert (vc[untouched] == V_SENT).all()

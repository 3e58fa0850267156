"""The ragged-decode references judge themselves on the CPU: the fp32
fallbacks of both ops, rounded to bf16, pass the rule with no violation,
and every deliberately wrong reference fails it."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ragged as kr
from torch_on_k8s_amd import ops

B, TMAX = 4, 103
LENS = [103, 1, 37, 0]


def _decode_case(Hq, Hkv, D, lens=LENS, nan_fill=True):
    q, kc, vc = kr.ragged_inputs(B, TMAX, Hq, Hkv, D, lens,
                                 nan_fill=nan_fill)
    lt = torch.tensor(lens, dtype=torch.int32)
    out = ops.attention_decode_ragged(q.float(), kc.float(), vc.float(), lt)
    return q, kc, vc, ko.q16(out)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
@pytest.mark.parametrize("num_splits", [1, 3, 8])
def test_decode_ragged_fallback_passes(Hq, Hkv, D, num_splits):
    q, kc, vc, out = _decode_case(Hq, Hkv, D)
    assert torch.isfinite(out.float()).all()
    assert (out[3] == 0).all()                       # len 0: exactly zero
    specs = kr.attention_decode_ragged(q, kc, vc, LENS, num_splits)
    # the planted key takes (nearly) all the weight in kv head 0's q heads
    assert (specs["seq0"].ref[0, 0] - vc[0, LENS[0] // 2, 0].double()
            ).abs().max() < 0.05
    ko.check_all(f"ragged_cpu[{Hq}/{Hkv},D={D},S={num_splits}]",
                 kr.split_rows(out), specs)


def test_decode_ragged_budget_follows_the_chains():
    # more keys on a chain cost more; a chunk bounds the chain
    assert kr.k_decode_ragged(8200, 8200, 1, 128) > \
        kr.k_decode_ragged(100, 8200, 1, 128)
    assert kr.k_decode_ragged(8200, 8200, 32, 128) < \
        kr.k_decode_ragged(8200, 8200, 1, 128)
    # D = 64 puts 8 rows in a wave load: half the chain of D = 128
    assert kr.k_decode_ragged(4096, 4096, 1, 64) < \
        kr.k_decode_ragged(4096, 4096, 1, 128)


@pytest.mark.parametrize("wrong", [
    dict(len_shift=1), dict(len_shift=-1), dict(roll=1),
    dict(kv_head_shift=1)])
def test_decode_ragged_wrong_reference_fails(wrong):
    # finite rows beyond each length (a reference that reads one row too
    # many must meet a number, not NaN), and no length at Tmax or 0
    lens = [90, 2, 37, 64]
    q, kc, vc, out = _decode_case(8, 2, 64, lens=lens, nan_fill=False)
    got = kr.split_rows(out)
    good = kr.attention_decode_ragged(q, kc, vc, lens, 1)
    assert ko.violates(got, good) == []
    bad = kr.attention_decode_ragged(q, kc, vc, lens, 1, **wrong)
    assert ko.violates(got, bad), wrong


def _append_case(Hq, Hkv, D, pos, Tmax=9):
    Bn = len(pos)
    qkv = ko.bf(Bn, (Hq + 2 * Hkv) * D, seed=5)
    cos, sin = ko.rope_table(Tmax + 3, D)
    kc = torch.full((Bn, Tmax, Hkv, D), 3.0)
    vc = torch.full((Bn, Tmax, Hkv, D), -5.0)
    pt = torch.tensor(pos, dtype=torch.int32)
    q = ops.qkv_rope_append_(qkv.float(), cos, sin, pt, kc, vc, Hq, Hkv, D)
    return qkv, cos, sin, pt, ko.q16(q), ko.q16(kc), ko.q16(vc)


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 2, 128)])
def test_qkv_rope_append_fallback_passes(Hq, Hkv, D):
    pos, Tmax = [0, 8, 5, -1], 9
    qkv, cos, sin, pt, q, kc, vc = _append_case(Hq, Hkv, D, pos)
    specs, live = kr.qkv_rope_append(qkv, cos, sin, pt, Tmax, Hq, Hkv, D)
    assert live.tolist() == [True, True, True, False]
    rows = torch.nonzero(live).flatten()
    ko.check_all(f"append_cpu[{Hq}/{Hkv},D={D}]",
                 {"q": q, "k": kc[rows, pt.long()[rows]]}, specs)
    v_in = qkv.view(len(pos), Hq + 2 * Hkv, D)[:, Hq + Hkv:]
    assert torch.equal(vc[rows, pt.long()[rows]], v_in[rows])
    assert (q[3] == 0).all()
    # every other cache row still holds the sentinel
    untouched = torch.ones(len(pos), Tmax, dtype=torch.bool)
    untouched[rows, pt.long()[rows]] = False
    assert (kc[untouched] == 3.0).all() and (vc[untouched] == -5.0).all()


def test_qkv_rope_append_wrong_position_fails():
    pos, Tmax = [0, 8, 5, -1], 9
    qkv, cos, sin, pt, q, kc, _ = _append_case(4, 2, 64, pos)
    rows = torch.tensor([0, 1, 2])
    got = {"q": q, "k": kc[rows, pt.long()[rows]]}
    good, _ = kr.qkv_rope_append(qkv, cos, sin, pt, Tmax, 4, 2, 64)
    assert ko.violates(got, good) == []
    bad, _ = kr.qkv_rope_append(qkv, cos, sin, pt, Tmax, 4, 2, 64,
                                pos_shift=1)
    assert sorted(ko.violates(got, bad)) == ["k", "q"]


def test_split_helpers():
    # shapes alone; the default reaches its cap on one long sequence
    assert ops.decode_ragged_splits(1, 1, 8200) > 1
    assert ops.decode_ragged_splits(32, 8, 4096) >= 1
    assert ops.decode_ragged_splits(4, 2, 103) == 1
    for Tmax in (1, 103, 8200):
        for S in (1, 3, 8, 32):
            c = ops.decode_ragged_chunk(Tmax, S)
            assert c >= 1 and c * S >= Tmax

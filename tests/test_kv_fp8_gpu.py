"""FP8 (e4m3) KV cache on the GPU: the hardware decode of every code, the
fp8 decode kernel against fp64 over the exactly dequantized caches, lengths
on the chunk boundaries, both writing kernels against the format's bounds
and against each other, and capture. Rule: kernel_oracle.py; inputs,
reference, k and the quantizer bounds: kernel_oracle_fp8.py."""
import functools

import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_fp8 as k8
import kernel_oracle_ragged as kr
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F8 = torch.float8_e4m3fn


def decode(q, kc, vc, ks, vs, lens, S):
    lt = lens if torch.is_tensor(lens) else \
        torch.tensor(lens, dtype=torch.int32, device=DEV)
    return ops.attention_decode_ragged(
        q.to(DEV), kc.to(DEV), vc.to(DEV), lt, kscale=ks.to(DEV),
        vscale=vs.to(DEV), num_splits=S)


def test_code_table_is_ocp_e4m3():
    """One key of weight 1 and vscale 1: the output IS the decoded V row.
    Every e4m3 value is exact in bf16, so equality is exact; torch.equal
    is bitwise here except that code 0x80 (-0) comes out as +0: the output
    is o = 0 + 1 * v."""
    codes = torch.arange(256, dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0
    vc = codes.view(2, 1, 1, 128).view(F8)
    q, kc, _, ks, _ = k8.fp8_inputs(2, 1, 1, 1, 128, [1, 1])
    out = decode(q, kc, vc, ks, torch.ones(2, 1, 1), [1, 1], 1)
    want = vc.view(2, 1, 128).to(torch.bfloat16)
    got = out.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (bad[:8], got[got != want][:8], want[got != want][:8])


@functools.lru_cache(maxsize=None)
def case(B, Tmax, Hq, Hkv, D, lens):
    return k8.fp8_inputs(B, Tmax, Hq, Hkv, D, lens)


def run(name, Tmax, Hq, Hkv, D, lens, S):
    q, kc, vc, ks, vs = case(len(lens), Tmax, Hq, Hkv, D, tuple(lens))
    specs = k8.decode_specs(q, kc, vc, ks, vs, lens, S)
    out = decode(q, kc, vc, ks, vs, lens, S)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b, n in enumerate(lens):
        if n == 0:
            assert (out[b] == 0).all()
    ko.check_all(name, kr.split_rows(out), specs)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
@pytest.mark.parametrize("num_splits", [1, 3, 8])
def test_fp8_decode_vs_fp64(Hq, Hkv, D, num_splits):
    """A block step is 128 keys at D = 128 and 256 at D = 64: 301 keys are
    more than one full step plus a ragged tail at either."""
    run(f"fp8[{Hq}/{Hkv},D={D},S={num_splits}]", 301, Hq, Hkv, D,
        [301, 1, 130, 0], num_splits)


@pytest.mark.parametrize("D", [64, 128])
def test_fp8_lengths_on_chunk_boundaries(D):
    Tmax = 301
    c = ops.decode_ragged_chunk(Tmax, 3)
    assert 2 * c <= Tmax
    run(f"fp8_boundary[D={D},c={c}]", Tmax, 8, 2, D,
        [c - 1, c, c + 1, 2 * c], 3)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tq", [1, 5])
def test_quantizing_appends(Tq, D):
    """Sequence 0 starts at pos = -1 (token 0 is dead; the others, if any,
    land in rows 0..), 2 has qlens < Tq, 3 runs off the end of the cache; an
    all-zero k and v row; a row whose amax is negative."""
    B, Hq, Hkv, Tmax = 4, 4, 2, 10
    qkv = ko.bf(B, Tq, (Hq + 2 * Hkv) * D, seed=3).view(B, Tq, Hq + 2 * Hkv, D)
    qkv[1, 0, Hq + 1] = 0            # k head 1
    qkv[1, 0, Hq + Hkv] = 0          # v head 0
    qkv[3, 0, Hq + Hkv, 5] = -7.0    # v head 0: amax at a negative element
    qkv = qkv.view(B, Tq, -1).to(DEV)
    cos, sin = (t.to(DEV) for t in ko.rope_table(Tmax, D))
    pos = torch.tensor([-1, 3, 0, 7], dtype=torch.int32, device=DEV)
    qlens = torch.tensor([Tq, Tq, Tq - 1, Tq], dtype=torch.int32, device=DEV)

    kb = torch.zeros(B, Tmax, Hkv, D, dtype=torch.bfloat16, device=DEV)
    vb = torch.zeros_like(kb)
    q_ref = ops.qkv_rope_append_chunk_(qkv, cos.float(), sin.float(), pos,
                                       qlens, kb, vb, Hq, Hkv, D)

    def sentinel():
        c = torch.full((B, Tmax, Hkv, D), 0x55, dtype=torch.uint8, device=DEV)
        s = torch.full((B, Tmax, Hkv), -1.0, device=DEV)
        return c.view(F8), c.clone().view(F8), s, s.clone()

    kc, vc, ks, vs = sentinel()
    q = ops.qkv_rope_append_fp8_(qkv, cos.float(), sin.float(), pos, qlens,
                                 kc, vc, ks, vs, Hq, Hkv, D)
    assert torch.equal(q.view(torch.int16), q_ref.view(torch.int16))

    at = pos.long().view(B, 1) + torch.arange(Tq, device=DEV).view(1, Tq)
    live = (torch.arange(Tq, device=DEV).view(1, Tq) < qlens.view(B, 1)) \
        & (at >= 0) & (at < Tmax)
    rows = torch.arange(B, device=DEV).view(B, 1)
    src = at.clamp(0, Tmax - 1)
    kc2, vc2, ks2, vs2 = sentinel()
    ops.kv_quantize_append_(kb[rows, src], vb[rows, src], pos, qlens, kc2,
                            vc2, ks2, vs2)
    # the two kernels: identical bytes, dead rows' sentinels included
    for a, b in ((kc, kc2), (vc, vc2)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in ((ks, ks2), (vs, vs2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))

    written = torch.zeros(B, Tmax, dtype=torch.bool, device=DEV)
    written[rows.expand(B, Tq)[live], at[live]] = True
    assert int(written.sum()) == int(live.sum()) > 0
    for x, c, s in ((kb, kc, ks), (vb, vc, vs)):
        assert (c.view(torch.uint8)[~written] == 0x55).all()
        assert (s[~written] == -1.0).all()
        k8.check_quantizer(
            x[written].reshape(-1, D),
            c.view(torch.uint8)[written].reshape(-1, D).view(F8),
            s[written].reshape(-1))
    assert (vs[1, 3, 0] == 0) and (ks[1, 3, 1] == 0)
    assert float(vs[3, 7, 0]) == pytest.approx(7.0 / 448, rel=2.0 ** -22)


def test_fp8_decode_repeatable_and_capturable():
    B, Tmax, Hq, Hkv, D = 4, 301, 8, 2, 128
    q, kc, vc, ks, vs = (t.to(DEV) for t in k8.fp8_inputs(
        B, Tmax, Hq, Hkv, D, [Tmax] * B, poison=False))
    lens = torch.tensor([301, 1, 130, 0], dtype=torch.int32, device=DEV)
    for S in (1, 3):
        a = decode(q, kc, vc, ks, vs, lens, S)
        assert torch.equal(a, decode(q, kc, vc, ks, vs, lens, S))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            decode(q, kc, vc, ks, vs, lens, S)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = decode(q, kc, vc, ks, vs, lens, S)
        new = torch.tensor([2, 299, 0, 64], dtype=torch.int32, device=DEV)
        saved = lens.clone()
        lens.copy_(new)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, decode(q, kc, vc, ks, vs, new, S))
        assert not torch.equal(cap, a)
        lens.copy_(saved)


def test_scales_and_cache_dtype_must_agree():
    q, kc, vc, ks, vs = (t.to(DEV) for t in k8.fp8_inputs(1, 4, 1, 1, 64, [4]))
    lens = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="kscale"):
        ops.attention_decode_ragged(q, kc, vc, lens)
    kb = torch.zeros(1, 4, 1, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.attention_decode_ragged(q, kb, kb, lens, kscale=ks, vscale=vs)

"""attention_paged over e4m3 pools, and the two fp8 paged appends, vs fp64.

Geometry, tables and bounds are those of test_attention_paged_gpu (imported).
An element means float(code) * scale; the reference is the plain fp64 masked
softmax over code.float().double() * scale.double() gathered through the
table, judged by kernel_oracle_attention.check with mid = sum_j p_ij |v_j|
over the dequantized v. The fp32 chains are those counted in the docstring of
test_attention_paged_gpu, plus, from attn_paged_fp8.hip as written:
  score   +1: kscale * c2 and its product with the MFMA sum, two roundings
  o_acc   +1: p * vscale, one rounding of every term of o (half a unit,
          counted as one as kernel_oracle_fp8 does)
The kernel's exp is one add and a 1-ulp v_exp_f32 where the bf16 kernel has
one fma, and its wave fold has no product: K_EXP and its doubling stay.
Nothing is fitted to the kernel's output.
"""
import functools
import math

import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_attention as ka
from test_attention_paged_gpu import (B, DEV, LENS, NAN, P, QLENS, TABLE,
                                      TABLE2, TMAX, bounds, dev_i32, pool_of,
                                      table)
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def pools_of(codes, scale, tab, lens=LENS):
    """Logical codes [B,256,Hkv,D] uint8 and scales [B,256,Hkv] -> (code pool,
    scale pool): code 0x7F and a NaN scale in every unreferenced page and in
    every slot >= n of a tail page."""
    cp = pool_of(codes.float(), tab, lens).nan_to_num(0x7F).to(torch.uint8)
    sp = pool_of(scale.unsqueeze(-1), tab, lens).squeeze(-1)
    return cp.view(F8).to(DEV), sp.to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(Hq, Hkv, D, Tq):
    """bf16 q (NaN in rows >= m); codes over all byte values but the two NaN
    codes; scales that are no powers of two; one live K row and one live V
    row with scale 0 and codes 0."""
    g = torch.Generator().manual_seed(D + Hq + Hkv)
    q = ko.q16(torch.randn(B, Tq, Hq, D, generator=g))
    codes = torch.randint(0, 256, (2, B, TMAX, Hkv, D), generator=g,
                          dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x3A
    ks = (0.5 + torch.rand(B, TMAX, Hkv, generator=g)) / 96
    vs = (0.5 + torch.rand(B, TMAX, Hkv, generator=g)) / 7
    codes[0, 0, 100, 0], ks[0, 100, 0] = 0, 0.0
    codes[1, 2, 70, 0], vs[2, 70, 0] = 0, 0.0
    for b in range(B):
        q[b, bounds(b, Tq)[1]:] = NAN
    return q, codes[0], codes[1], ks, vs


@functools.lru_cache(maxsize=None)
def reference(Hq, Hkv, D, Tq, S):
    """Plain fp64 masked softmax per sequence and head -> AttnSpec."""
    q, kc, vc, ks, vs = inputs(Hq, Hkv, D, Tq)
    kd = kc.view(F8).float().double() * ks.double().unsqueeze(-1)
    vd = vc.view(F8).float().double() * vs.double().unsqueeze(-1)
    rep = Hq // Hkv
    nt = ops.extend_chunk(TMAX, S) // 64
    KS, fold = ka.k_score(D) + 1, (S if S > 1 else 0) + 1
    if Tq * rep <= 16:   # key-split
        KE = 2 * ka.K_EXP
        KA = ko.kred(17 * nt) + ko.kred(5 * nt + 4) + 4 + fold + 1
    else:
        KE, KA = ka.K_EXP, ko.kred(65 * nt) + ko.kred(17 * nt + 4) + fold + 1
    ref, mid, w32 = (torch.zeros(q.shape, dtype=torch.float64)
                     for _ in range(3))
    for b in range(B):
        n, m = bounds(b, Tq)
        if m == 0:
            continue
        qh = ko.f64(q[b, :m]).permute(1, 0, 2)
        kh = kd[b, :n].permute(1, 0, 2).repeat_interleave(rep, 0)
        vh = vd[b, :n].permute(1, 0, 2).repeat_interleave(rep, 0)
        ok = torch.arange(n).view(1, n) <= (n - m + torch.arange(m)).view(m, 1)
        s = (qh @ kh.mT / math.sqrt(D)).masked_fill(~ok, -math.inf)
        sabs = (qh.abs() @ kh.abs().mT / math.sqrt(D)).masked_fill(~ok, 0.0)
        p = torch.softmax(s, -1)
        e = (1 + (s - s.amax(-1, keepdim=True)).abs()).masked_fill(~ok, 0.0)
        w = KS * (sabs + (p * sabs).sum(-1, keepdim=True)) + \
            KE * (e + (p * e).sum(-1, keepdim=True)) + KA
        ref[b, :m] = (p @ vh).permute(1, 0, 2)
        mid[b, :m] = (p @ vh.abs()).permute(1, 0, 2)
        w32[b, :m] = ((p * w) @ vh.abs()).permute(1, 0, 2)
    k = KS + KE + KA
    return ka.AttnSpec(ref, mid, w32 / k, k, True)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("Tq", [1, 3, 19])
@pytest.mark.parametrize("S", [1, 2])
def test_paged_fp8_vs_fp64(Hq, Hkv, D, Tq, S):
    q, kc, vc, ks, vs = inputs(Hq, Hkv, D, Tq)
    spec = reference(Hq, Hkv, D, Tq, S)
    qg, lens, qlens = q.to(DEV), dev_i32(LENS), dev_i32(QLENS)

    def run(tab, rows=slice(None)):
        (kp, ksp), (vp, vsp) = pools_of(kc, ks, tab), pools_of(vc, vs, tab)
        return ops.attention_paged(qg[rows], kp, vp, dev_i32(tab[rows]),
                                   lens[rows], qlens[rows], kscale=ksp,
                                   vscale=vsp, num_splits=S)

    out = run(TABLE)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b in range(B):
        assert (out[b, bounds(b, Tq)[1]:] == 0).all()
    ka.check(f"paged_fp8[{Hq}/{Hkv},D={D},Tq={Tq},S={S}]", out, spec)
    assert torch.equal(out, run(TABLE))
    assert torch.equal(run(TABLE, slice(0, 1))[0], out[0])
    assert torch.equal(run(TABLE2), out)


@pytest.mark.parametrize("Tq", [1, 19])   # key-split, row layout
def test_captured_call_follows_new_table_lengths_and_scales(Tq):
    q, kc, vc, ks, vs = inputs(8, 2, 128, Tq)
    full = [TMAX] * B                 # every page of the pool holds data
    q = q.nan_to_num(0.25).to(DEV)
    (kp, ksp), (vp, vsp) = (pools_of(c, s, table(7, 3, full), full)
                            for c, s in ((kc, ks), (vc, vs)))
    tab, lens, qlens = dev_i32(table(7, 3, full)), dev_i32(LENS), dev_i32(QLENS)

    def call(t, n, m):
        return ops.attention_paged(q, kp, vp, t, n, m, kscale=ksp, vscale=vsp,
                                   num_splits=2)

    first = call(tab, lens, qlens)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(tab, lens, qlens)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = call(tab, lens, qlens)
    new_l, new_q, new_t = [64, 200, 0, 130, 19, 1], [7, 19, 3, 2, 19, 1], \
        table(5, 11, full)
    lens.copy_(dev_i32(new_l))
    qlens.copy_(dev_i32(new_q))
    tab.copy_(dev_i32(new_t))
    ksp.mul_(torch.linspace(0.5, 1.5, 64, device=DEV))
    vsp.mul_(torch.linspace(1.5, 0.5, 64, device=DEV))
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    want = call(dev_i32(new_t), dev_i32(new_l), dev_i32(new_q))
    assert torch.equal(cap, want) and not torch.equal(cap, first)


@pytest.mark.parametrize("Tq", [1, 5])
def test_paged_appends_equal_the_contiguous_ones(Tq):
    """Tokens across a page boundary, and dead ones: qlens short, pos = -1,
    table entry -1 and P + 5."""
    Hq, Hkv, D, nb, npg, npool = 4, 2, 128, 6, 2, 8
    tab = [[2, 5], [7, 0], [1, 3], [4, -1], [6, npool + 5], [3, 1]]
    pos, qlens = [3, 62, -1, 64, 10, 124], [Tq - 1, Tq, Tq, Tq, Tq, Tq]
    g = torch.Generator().manual_seed(Tq)
    qkv = ko.q16(torch.randn(nb, Tq, (Hq + 2 * Hkv) * D, generator=g)).to(DEV)
    qkv[4, 0, Hq * D:(Hq + 1) * D] = 0                 # an all-zero k row
    ang = torch.rand(64 * npg, D // 2, generator=g) * 6.0
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    pos_d, ql_d, tab_d = dev_i32(pos), dev_i32(qlens), dev_i32(tab)

    def blank(*shape):
        return (torch.full(shape + (D,), 0x55, dtype=torch.uint8,
                           device=DEV).view(F8),
                torch.full(shape, -1.0, device=DEV))

    def scattered(cache, scale):
        """The blank pools with every live token's contiguous row copied in."""
        pool, spool = blank(npool, Hkv, 64)
        live = torch.zeros(nb, Tq, dtype=torch.bool)
        for b in range(nb):
            for i in range(qlens[b]):
                p = pos[b] + i
                if 0 <= p < 64 * npg and 0 <= tab[b][p // 64] < npool:
                    live[b, i] = True
                    pid = tab[b][p // 64]
                    pool.view(torch.uint8)[pid, :, p % 64] = \
                        cache.view(torch.uint8)[b, p]
                    spool[pid, :, p % 64] = scale[b, p]
        return pool, spool, live.to(DEV)

    def same(got, want):
        return torch.equal(got.view(torch.uint8) if got.dtype == F8 else got,
                           want.view(torch.uint8) if want.dtype == F8 else want)

    for rope in (True, False):
        (kc, ks), (vc, vs) = blank(nb, 64 * npg, Hkv), blank(nb, 64 * npg, Hkv)
        (kp, ksp), (vp, vsp) = blank(npool, Hkv, 64), blank(npool, Hkv, 64)
        if rope:
            q_ref = ops.qkv_rope_append_fp8_(qkv, cos, sin, pos_d, ql_d, kc,
                                             vc, ks, vs, Hq, Hkv, D)
            q = ops.qkv_rope_append_paged_fp8_(qkv, cos, sin, pos_d, ql_d, kp,
                                               vp, ksp, vsp, tab_d, Hq, Hkv, D)
        else:
            k, v = (qkv.view(nb, Tq, Hq + 2 * Hkv, D)[:, :, s:s + Hkv]
                    .contiguous() for s in (Hq, Hq + Hkv))
            ops.kv_quantize_append_(k, v, pos_d, ql_d, kc, vc, ks, vs)
            ops.kv_quantize_append_paged_(k, v, pos_d, ql_d, kp, vp, ksp, vsp,
                                          tab_d)
        for cache, scale, pool, spool in ((kc, ks, kp, ksp), (vc, vs, vp, vsp)):
            want_p, want_s, live = scattered(cache, scale)
            assert same(pool, want_p) and same(spool, want_s)
        assert int(live.sum()) == (3 if Tq == 1 else 22)
        if rope:
            assert same(q, q_ref * live.view(nb, Tq, 1, 1))


def test_scale_mismatch_raises():
    q = torch.zeros(1, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    kp = torch.zeros(2, 1, 64, 64, dtype=torch.uint8, device=DEV).view(F8)
    kb = torch.zeros(2, 1, 64, 64, dtype=torch.bfloat16, device=DEV)
    sc = torch.ones(2, 1, 64, device=DEV)
    one, tab = dev_i32([1]), dev_i32([[0]])
    with pytest.raises(ValueError, match="need kscale"):
        ops.attention_paged(q, kp, kp, tab, one, one)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.attention_paged(q, kb, kb, tab, one, one, kscale=sc, vscale=sc)
    with pytest.raises(ValueError, match="kscale and vscale"):
        ops.attention_paged(q, kp, kp, tab, one, one, kscale=sc[:1], vscale=sc)

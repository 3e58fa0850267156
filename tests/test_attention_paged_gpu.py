"""attention_paged vs fp64: Tq new tokens per sequence over 64-token pages.

The reference is the plain fp64 masked softmax of test_attention_extend_gpu
on the logically gathered cache, judged by kernel_oracle_attention.check
(|got - ref| <= 2^-8 |ref| + 2^-8 mid + k 2^-23 scale + 2^-126, mid =
sum_j p_ij |v_j| for P's one bf16 rounding, kt_pack of attn_kv_tile.h). The
fp32 chains, counted from attn_paged.hip as written (the same arithmetic as
kt_attn of attn_kv_tile.h; one rounding = half a unit), n_t = chunk / 64 tiles per split:
  score      k_score(D): the D-term MFMA chain of S^T and c2 with its fma
  exp        K_EXP = 1 per key: one fma and a 1-ulp v_exp_f32. Key-split: 2,
             because the wave fold's weight e_w = exp2((m_w - M) c2) (a
             subtraction, a product, the exp) multiplies every key of wave w
             and |m_w - M| <= |s_j - M| for each of them
  o_acc      row layout 64 products and one alpha multiply per tile:
             kred(65 n_t); key-split 16 products and the multiply: kred(17 n_t)
  l_run      row layout 16 in-lane adds and fma(l, alpha, psum) per tile,
             then the four lanes of a row: kred(17 n_t + 4); key-split 4
             in-lane adds and the fma: kred(5 n_t + 4)
  wave fold  key-split only: one fma into o and one into L per wave, two
             roundings = one unit per wave: 4
  split fold attn_decode_ragged_combine: one unit per split; none at one split
  divide     1/l and o * (1/l): one unit
Nothing is fitted to the kernel's output.
"""
import functools
import math

import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_attention as ka
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, NP, P, TMAX = 6, 4, 24, 256
LENS = [200, 64, 129, 65, 5, 0]
QLENS = [19, 19, 1, 0, 19, 7]
NAN = float("nan")


def table(mul, add, lens=LENS):
    """Page j of sequence b, dealt in order from the bijection
    i -> (mul i + add) % P; unused entries are -1 and P + 5."""
    ids = iter((mul * i + add) % P for i in range(P))
    return [[next(ids) if 64 * j < n else (-1, P + 5)[j % 2]
             for j in range(NP)] for n in lens]


TABLE, TABLE2 = table(7, 3), table(5, 11)


def bounds(b, Tq, lens=LENS, qlens=QLENS):
    n = min(max(lens[b], 0), TMAX)
    return n, min(max(qlens[b], 0), Tq, n)


def pool_of(cache, tab, lens=LENS):
    """[B, 256, Hkv, D] -> pool [P, Hkv, 64, D]; NaN in every page no
    sequence references and in every row >= n of a tail page."""
    pool = torch.full((P, cache.shape[2], 64, cache.shape[3]), NAN,
                      dtype=cache.dtype)
    for b, n in enumerate(lens):
        for j in range(-(-n // 64)):
            rows = cache[b, 64 * j:min(64 * j + 64, n)]
            pool[tab[b][j], :, :rows.shape[0]] = rows.permute(1, 0, 2)
    return pool


@functools.lru_cache(maxsize=None)
def inputs(Hq, Hkv, D, Tq):
    """bf16 q and the logical caches. For Tq = 19 the planted key of the
    extend test: query 3 of sequence 0 must see it, query 2 must not. NaN in
    every q row >= m."""
    g = torch.Generator().manual_seed(D + Hq + Hkv)
    q = ko.q16(torch.randn(B, Tq, Hq, D, generator=g))
    kc = ko.q16(torch.randn(B, TMAX, Hkv, D, generator=g))
    vc = ko.q16(torch.randn(B, TMAX, Hkv, D, generator=g) * 0.5)
    if Tq == 19:
        q[0, 3, 0] = q[0, 2, 0]
        kc[0, LENS[0] - QLENS[0] + 3, 0] = ko.q16(2 * q[0, 2, 0].float())
    for b in range(B):
        q[b, bounds(b, Tq)[1]:] = NAN
    return q, kc, vc


@functools.lru_cache(maxsize=None)
def reference(Hq, Hkv, D, Tq, S):
    """Plain fp64 masked softmax per sequence and head -> AttnSpec."""
    q, kc, vc = inputs(Hq, Hkv, D, Tq)
    rep = Hq // Hkv
    nt = ops.extend_chunk(TMAX, S) // 64
    KS, fold = ka.k_score(D), (S if S > 1 else 0) + 1
    if Tq * rep <= 16:   # key-split
        KE, KA = 2 * ka.K_EXP, ko.kred(17 * nt) + ko.kred(5 * nt + 4) + 4 + fold
    else:
        KE, KA = ka.K_EXP, ko.kred(65 * nt) + ko.kred(17 * nt + 4) + fold
    ref, mid, w32 = (torch.zeros(q.shape, dtype=torch.float64)
                     for _ in range(3))
    for b in range(B):
        n, m = bounds(b, Tq)
        if m == 0:
            continue
        qh = ko.f64(q[b, :m]).permute(1, 0, 2)
        kh = ko.f64(kc[b, :n]).permute(1, 0, 2).repeat_interleave(rep, 0)
        vh = ko.f64(vc[b, :n]).permute(1, 0, 2).repeat_interleave(rep, 0)
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


def dev_i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("Tq", [1, 2, 3, 19])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_paged_vs_fp64(Hq, Hkv, D, Tq, S):
    q, kc, vc = inputs(Hq, Hkv, D, Tq)
    spec = reference(Hq, Hkv, D, Tq, S)
    if Tq == 19:
        planted_v = vc[0, LENS[0] - QLENS[0] + 3, 0].double()
        assert (spec.ref[0, 3, 0] - planted_v).abs().max() < 0.05
        assert (spec.ref[0, 2, 0] - planted_v).abs().max() > 0.05
    qg, lens, qlens = q.to(DEV), dev_i32(LENS), dev_i32(QLENS)
    kp, vp = pool_of(kc, TABLE).to(DEV), pool_of(vc, TABLE).to(DEV)
    out = ops.attention_paged(qg, kp, vp, dev_i32(TABLE), lens, qlens,
                              num_splits=S)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b in range(B):
        assert (out[b, bounds(b, Tq)[1]:] == 0).all()
    ka.check(f"paged[{Hq}/{Hkv},D={D},Tq={Tq},S={S}]", out, spec)
    again = ops.attention_paged(qg, kp, vp, dev_i32(TABLE), lens, qlens,
                                num_splits=S)
    assert torch.equal(out, again)
    alone = ops.attention_paged(qg[:1], kp, vp, dev_i32(TABLE[:1]), lens[:1],
                                qlens[:1], num_splits=S)
    assert torch.equal(alone[0], out[0])
    moved = ops.attention_paged(qg, pool_of(kc, TABLE2).to(DEV),
                                pool_of(vc, TABLE2).to(DEV), dev_i32(TABLE2),
                                lens, qlens, num_splits=S)
    assert torch.equal(moved, out)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 2])
def test_row_layout_is_bit_equal_to_attention_extend(D, S):
    """Tq * R > 16: over a pool and a shuffled table, attention_paged gives the
    bits attention_extend gives over the contiguous cache holding the same
    rows. The two kernels share their arithmetic and differ only in where a
    tile's bytes come from."""
    Hq, Hkv, Tq, npages, lens, qlens = 8, 2, 19, 3, [130, 83], [19, 7]
    g = torch.Generator().manual_seed(7 * D + S)
    q = ko.q16(torch.randn(2, Tq, Hq, D, generator=g))
    kc = ko.q16(torch.randn(2, 64 * npages, Hkv, D, generator=g))
    vc = ko.q16(torch.randn(2, 64 * npages, Hkv, D, generator=g) * 0.5)
    tab = [[17, 2, 9], [11, 20, P + 5]]   # 83 rows: two pages, one unused
    n, m = dev_i32(lens), dev_i32(qlens)
    want = ops.attention_extend(q.to(DEV), kc.to(DEV), vc.to(DEV), n, m,
                                num_splits=S)
    got = ops.attention_paged(q.to(DEV), pool_of(kc, tab, lens).to(DEV),
                              pool_of(vc, tab, lens).to(DEV), dev_i32(tab), n,
                              m, num_splits=S)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize("Tq", [1, 19])   # key-split, row layout
def test_captured_call_follows_new_table_and_lengths(Tq):
    q, kc, vc = (t.nan_to_num(0.25) for t in inputs(8, 2, 128, Tq))
    full = [TMAX] * B                 # every page of the pool holds data
    q, kp, vp = q.to(DEV), pool_of(kc, table(7, 3, full), full).to(DEV), \
        pool_of(vc, table(7, 3, full), full).to(DEV)
    tab, lens, qlens = dev_i32(table(7, 3, full)), dev_i32(LENS), dev_i32(QLENS)

    def call(t, n, m):
        return ops.attention_paged(q, kp, vp, t, n, m, num_splits=2)

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
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    want = call(dev_i32(new_t), dev_i32(new_l), dev_i32(new_q))
    assert torch.equal(cap, want) and not torch.equal(cap, first)


@pytest.mark.parametrize("Hq,D,page,msg", [(3, 64, 64, "1, 2, 4 or 8"),
                                           (2, 32, 64, "64 or 128"),
                                           (2, 64, 32, "page size")])
def test_unsupported_shape_raises(Hq, D, page, msg):
    q = torch.zeros(1, 2, Hq, D, dtype=torch.bfloat16, device=DEV)
    kp = torch.zeros(2, 1, page, D, dtype=torch.bfloat16, device=DEV)
    one = dev_i32([1])
    with pytest.raises(RuntimeError, match=msg):
        ops.attention_paged(q, kp, kp.clone(), dev_i32([[0]]), one, one)

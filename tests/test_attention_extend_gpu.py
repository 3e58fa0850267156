"""attention_extend vs fp64: Tq new tokens per sequence over a ragged cache.

Rule: kernel_oracle_attention.compare (|got - ref| <= 2^-8 |ref| + 2^-8 mid
+ k 2^-23 scale + 2^-126), mid = sum_j p_ij |v_j| for P's one bf16 rounding
(attn_extend.hip, kt_pack of attn_kv_tile.h in the P repack). The fp32
chains, counted from kt_attn and its segments in attn_kv_tile.h as written
(kt_scores, kt_softmax_step, kt_rescale, kt_pv64, kt_store_*; one rounding =
half a unit), n_t = chunk / 64:
  score      k_score(D): the D-term MFMA chain of S^T = K Q^T and
             c2 = scale * LOG2E with the fma that applies it (units of sabs)
  exp        K_EXP = 1: one fma and a 1-ulp v_exp_f32; the argument is
             s - m_run with m_run <= the row's max (units of 1 + |s - M|)
  o_acc      64 products and one alpha multiply per tile: kred(65 n_t)
  l_run      16 in-lane adds and fma(l, alpha, psum) per tile, then the four
             lanes of a row: kred(17 n_t + 4)
  split fold attn_decode_ragged_combine: one fma into acc and one into L per
             split, two roundings = one unit per split (its exp weight
             multiplies both and cancels, as alpha does); none at one split
  divide     1/l and o * (1/l): two roundings = one unit
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
B, TMAX, TQ = 6, 200, 19
LENS = [200, 19, 129, 37, 5, 64]
QLENS = [19, 19, 1, 0, 19, 7]
NAN = float("nan")


def bounds(b, lens=LENS, qlens=QLENS):
    n = min(max(lens[b], 0), TMAX)
    return n, min(max(qlens[b], 0), TQ, n)


@functools.lru_cache(maxsize=None)
def inputs(Hq, Hkv, D):
    """bf16 q, kcache, vcache. In sequence 0 the key at n - m + 3 of kv head 0
    is 2 * q[0, 2, 0], and q[0, 3, 0] = q[0, 2, 0]: query 3 must see that key
    (it then takes nearly all of row 3's weight) and query 2 must not. NaN in
    every cache row >= n and every q row >= m."""
    g = torch.Generator().manual_seed(D + Hq + Hkv)
    q = ko.q16(torch.randn(B, TQ, Hq, D, generator=g))
    kc = ko.q16(torch.randn(B, TMAX, Hkv, D, generator=g))
    vc = ko.q16(torch.randn(B, TMAX, Hkv, D, generator=g) * 0.5)
    q[0, 3, 0] = q[0, 2, 0]
    kc[0, LENS[0] - QLENS[0] + 3, 0] = ko.q16(2 * q[0, 2, 0].float())
    for b in range(B):
        n, m = bounds(b)
        kc[b, n:], vc[b, n:], q[b, m:] = NAN, NAN, NAN
    return q, kc, vc


def reference(q, kc, vc, lens, qlens, S):
    """Plain fp64 masked softmax per sequence and head -> AttnSpec."""
    Hq, D, rep = q.shape[2], q.shape[3], q.shape[2] // kc.shape[2]
    nt = ops.extend_chunk(TMAX, S) // 64
    KS = ka.k_score(D)
    KA = ko.kred(65 * nt) + ko.kred(17 * nt + 4) + (S if S > 1 else 0) + 1
    ref, mid, w32 = (torch.zeros(q.shape, dtype=torch.float64)
                     for _ in range(3))
    for b in range(q.shape[0]):
        n, m = bounds(b, lens, qlens)
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
            ka.K_EXP * (e + (p * e).sum(-1, keepdim=True)) + KA
        ref[b, :m] = (p @ vh).permute(1, 0, 2)
        mid[b, :m] = (p @ vh.abs()).permute(1, 0, 2)
        w32[b, :m] = ((p * w) @ vh.abs()).permute(1, 0, 2)
    k = KS + ka.K_EXP + KA
    return ka.AttnSpec(ref, mid, w32 / k, k, True)


def dev_i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_extend_vs_fp64(Hq, Hkv, D, S):
    assert ops.extend_chunk(TMAX, S) == 256 // S
    q, kc, vc = inputs(Hq, Hkv, D)
    spec = reference(q, kc, vc, LENS, QLENS, S)
    planted_v = vc[0, LENS[0] - QLENS[0] + 3, 0].double()
    assert (spec.ref[0, 3, 0] - planted_v).abs().max() < 0.05
    assert (spec.ref[0, 2, 0] - planted_v).abs().max() > 0.05
    qg, kg, vg = q.to(DEV), kc.to(DEV), vc.to(DEV)
    out = ops.attention_extend(qg, kg, vg, dev_i32(LENS), dev_i32(QLENS),
                               num_splits=S)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b in range(B):
        assert (out[b, bounds(b)[1]:] == 0).all()
    ka.check(f"extend[{Hq}/{Hkv},D={D},S={S}]", out, spec)
    again = ops.attention_extend(qg, kg, vg, dev_i32(LENS), dev_i32(QLENS),
                                 num_splits=S)
    assert torch.equal(out, again)
    alone = ops.attention_extend(qg[:1], kg[:1], vg[:1], dev_i32(LENS[:1]),
                                 dev_i32(QLENS[:1]), num_splits=S)
    assert torch.equal(alone[0], out[0])


@pytest.mark.parametrize("S", [1, 2])
def test_captured_call_follows_new_lengths(S):
    q, kc, vc = (t.nan_to_num(0.25).to(DEV) for t in inputs(8, 2, 128))
    lens, qlens = dev_i32(LENS), dev_i32(QLENS)
    first = ops.attention_extend(q, kc, vc, lens, qlens, num_splits=S)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_extend(q, kc, vc, lens, qlens, num_splits=S)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.attention_extend(q, kc, vc, lens, qlens, num_splits=S)
    new_l, new_q = [64, 200, 0, 130, 19, 1], [7, 19, 3, 2, 19, 1]
    lens.copy_(dev_i32(new_l))
    qlens.copy_(dev_i32(new_q))
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    want = ops.attention_extend(q, kc, vc, dev_i32(new_l), dev_i32(new_q),
                                num_splits=S)
    assert torch.equal(cap, want) and not torch.equal(cap, first)


@pytest.mark.parametrize("Hq,D,msg", [(3, 64, "1, 2, 4 or 8"),
                                      (2, 32, "64 or 128")])
def test_unsupported_shape_raises(Hq, D, msg):
    q = torch.zeros(1, 2, Hq, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(1, 8, 1, D, dtype=torch.bfloat16, device=DEV)
    one = dev_i32([1])
    with pytest.raises(RuntimeError, match=msg):
        ops.attention_extend(q, kc, kc.clone(), one, one)

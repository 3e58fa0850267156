"""Document-masked attention on the CPU: the per-document fp64 references of
``kernel_oracle_attention_docs.py`` judge the package's CPU path.

 * ops.attention(..., doc_start=...) with autograd (fp32), rounded to bf16
   where the kernels round their outputs, passes the rule on every case the
   GPU test uses, in both regimes, with no violation.
 * The per-document references agree with one fp64 computation over the
   whole row under the document mask.
 * A mask shifted by one key at every document start, rounded the same way,
   violates the rule on all five outputs.
 * ops.doc_bounds against a Python loop; the bounds contract is validated on
   the CPU; causal=False with bounds is refused.
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
import kernel_oracle_attention_docs as kd
from kernel_oracle import q16
from torch_on_k8s_amd import ops

CASES = [(s, tuple(map(tuple, lay)), r) for s, lay in kd.CASES
         for r in kd.REGIMES]
IDS = [f"{i}-{r}" for i in kd.IDS for r in kd.REGIMES]


@functools.lru_cache(maxsize=2)
def problem(shape, layouts, regime):
    qkvd = ka.inputs(*shape, True, regime=regime)
    return qkvd, kd.attention(*qkvd, layouts)


def package_cpu(q, k, v, do, layouts):
    """ops.attention on CPU tensors in fp32 through autograd; LSE, which it
    does not return, as an fp32 logsumexp of the same masked scores."""
    B, S, Hq, D = q.shape
    ds, de = kd.bounds(layouts, S)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qr, kr, vr, causal=True, doc_start=ds, doc_end=de)
    o.backward(do.float())
    rep = Hq // k.shape[2]
    s = torch.matmul(q.float().permute(0, 2, 1, 3),
                     k.float().permute(0, 2, 1, 3).repeat_interleave(
                         rep, dim=1).transpose(-1, -2)) / (D ** 0.5)
    i = torch.arange(S).view(1, 1, S, 1)
    j = torch.arange(S).view(1, 1, 1, S)
    dead = (j > i) | (j < ds.long().view(B, 1, S, 1))
    s = s.masked_fill(dead, float("-inf"))
    return {"o": q16(o.detach()), "lse": torch.logsumexp(s, -1),
            "dq": q16(qr.grad), "dk": q16(kr.grad), "dv": q16(vr.grad)}


@pytest.mark.parametrize("shape,layouts,regime", CASES, ids=IDS)
def test_package_cpu_path_passes(shape, layouts, regime):
    qkvd, specs = problem(shape, layouts, regime)
    ka.check_all(f"cpu_docs[{shape},{regime}]",
                 package_cpu(*qkvd, layouts), specs)


@pytest.mark.parametrize("shape,layouts,regime", CASES, ids=IDS)
def test_whole_row_agrees_and_shifted_mask_fails(shape, layouts, regime):
    qkvd, specs = problem(shape, layouts, regime)
    whole = kd.whole_row(*qkvd, layouts)
    for n, t in whole.items():
        ref = specs[n].ref
        assert t.shape == ref.shape, n
        err = float((t - ref).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (n, err)
    if max(len(lay) for lay in layouts) < 2:
        return
    bad = kd.whole_row(*qkvd, layouts, start_shift=-1)
    got = {n: (t.float() if n == "lse" else q16(t)) for n, t in bad.items()}
    res = {n: ka.compare(n, got[n], specs[n]) for n in got}
    print(f"WRONG doc_start-1 {shape} {regime}: " + " ".join(
        f"{n}={r.ratio:.1f}" for n, r in res.items()))
    passed = sorted(n for n, r in res.items() if not r.violations)
    assert not passed, f"shifted document mask passes on {passed}"


def test_doc_tiles_bind_the_chain_lengths():
    """The adjustment is in force and only ever widens: a 10-token document
    at offset 60 lies across two key tiles where n_tiles(10) is one."""
    assert kd.doc_tiles(60, 10) == 2 and ka.n_tiles(10) == 1
    assert kd.doc_tiles(70, 58) == 1 and kd.doc_tiles(64, 64) == 1
    assert kd.doc_tiles(10, 500) == 8 and kd.doc_tiles(510, 10) == 2
    for a in range(0, 130, 7):
        for L in (1, 31, 64, 65, 200):
            assert kd.doc_tiles(a, L) >= ka.n_tiles(L)
    q, k, v, do = ka.inputs(1, 128, 2, 2, 64, True)
    packed = kd.attention(q, k, v, do, [[60, 10, 58]])
    alone = ka.attention(*(t[:, 60:70].contiguous() for t in (q, k, v, do)),
                         True)
    for n in packed:
        cut = (lambda t: t[..., 60:70]) if n == "lse" else \
            (lambda t: t[:, 60:70])
        assert torch.equal(cut(packed[n].ref), alone[n].ref), n
        assert torch.equal(cut(packed[n].mid), alone[n].mid), n
        wide = cut(packed[n].k * packed[n].scale)
        assert (wide >= alone[n].k * alone[n].scale).all(), n
        assert (wide > alone[n].k * alone[n].scale).any(), n
    assert ka.n_tiles(10) == 1          # the binding does not outlive a call


# --------------------------------------------------------------------------
# ops.doc_bounds and the contract
# --------------------------------------------------------------------------
def loop_bounds(ids, eos):
    B, S = ids.shape
    ds = torch.zeros(B, S, dtype=torch.int32)
    de = torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        start = 0
        for i in range(S):
            ds[b, i] = start
            if int(ids[b, i]) == eos or i == S - 1:
                de[b, start:i + 1] = i + 1
                start = i + 1
    return ds, de


E = 7
ROWS = {
    "eos_at_0": [E, 1, 2, 3, 4, 5],
    "eos_at_last": [1, 2, 3, 4, 5, E],
    "adjacent_eos": [1, E, E, E, 2, 3],
    "no_eos": [1, 2, 3, 4, 5, 6],
    "all_eos": [E] * 6,
    "mixed": [1, 2, E, 3, E, 4],
}


@pytest.mark.parametrize("name", list(ROWS))
def test_doc_bounds_single_rows(name):
    ids = torch.tensor([ROWS[name]])
    ds, de = ops.doc_bounds(ids, E)
    wds, wde = loop_bounds(ids, E)
    assert ds.dtype == torch.int32 and de.dtype == torch.int32
    assert torch.equal(ds, wds) and torch.equal(de, wde), (ds, de, wds, wde)
    ops.validate_doc_bounds(ds, de, *ids.shape)
    assert torch.equal(ops.doc_end_from_start(ds), de)


def test_doc_bounds_batch_random():
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 12, (5, 97), generator=g)
    ds, de = ops.doc_bounds(ids, 3)
    wds, wde = loop_bounds(ids, 3)
    assert torch.equal(ds, wds) and torch.equal(de, wde)
    assert ds.is_contiguous() and de.is_contiguous()
    assert torch.equal(ops.doc_end_from_start(ds), de)
    # the two statements of the mask are the same set of pairs
    i = torch.arange(97).view(1, 97, 1)
    j = torch.arange(97).view(1, 1, 97)
    a = (ds.long().view(5, 97, 1) <= j) & (j <= i)
    b = (j <= i) & (i < de.long().view(5, 1, 97))
    assert torch.equal(a, b)


def test_layout_bounds_match_doc_bounds():
    for (B, S, *_), lay in kd.CASES:
        ids = torch.ones(B, S, dtype=torch.long)
        for b, lengths in enumerate(lay):
            for a, L in kd.offsets(lengths):
                ids[b, a + L - 1] = 0
        ds, de = ops.doc_bounds(ids, 0)
        wds, wde = kd.bounds(lay, S)
        assert torch.equal(ds, wds) and torch.equal(de, wde)


@pytest.mark.parametrize("spoil", ["negative", "above_row", "decreasing",
                                   "not_constant", "dtype", "shape",
                                   "doc_end"])
def test_cpu_path_validates_bounds(spoil):
    q, k, v, _ = ka.inputs(1, 16, 2, 1, 64, True)
    ds, de = kd.bounds([[6, 10]], 16)
    if spoil == "negative":
        ds[0, 2] = -1
    elif spoil == "above_row":
        ds[0, 3] = 5
    elif spoil == "decreasing":
        ds[0, 9] = 0
    elif spoil == "not_constant":
        ds[0, 8:] = 7          # 0 <= . <= i, monotone, but row 7 starts at 6
    elif spoil == "dtype":
        ds = ds.long()
    elif spoil == "shape":
        ds = ds[:, :15]
    elif spoil == "doc_end":
        de[0, 0] = 7
    with pytest.raises(ValueError):
        ops.attention(q.float(), k.float(), v.float(), True, doc_start=ds,
                      doc_end=de)


def test_noncausal_with_bounds_is_refused():
    q, k, v, _ = ka.inputs(1, 16, 2, 1, 64, True)
    ds, de = kd.bounds([[6, 10]], 16)
    with pytest.raises(ValueError):
        ops.attention(q.float(), k.float(), v.float(), causal=False,
                      doc_start=ds, doc_end=de)
    with pytest.raises(ValueError):
        ops.attention(q.float(), k.float(), v.float(), doc_end=de)


def test_doc_end_is_derived_when_omitted():
    q, k, v, _ = ka.inputs(1, 64, 2, 1, 64, True)
    ds, de = kd.bounds([[20, 44]], 64)
    a = ops.attention(q.float(), k.float(), v.float(), doc_start=ds)
    b = ops.attention(q.float(), k.float(), v.float(), doc_start=ds,
                      doc_end=de)
    assert torch.equal(a, b)
    # a document's first row is its own value row
    assert torch.equal(a[0, 20], v[0, 20].float().repeat_interleave(2, 0))

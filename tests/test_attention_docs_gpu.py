"""GPU numerics of document-masked attention and document-relative RoPE.

The three default attention kernels (attn_fwd_kernel_v4, the fused dK+dV
kernel and the 8-wave dQ kernel) with packed-document bounds, against the
per-document fp64 references of ``kernel_oracle_attention_docs.py``, per
element, by the rule of ``kernel_oracle_attention.py`` with no element
excluded. Each case goes through the forward and then the backward on the
forward's own o and lse, in the ``flat`` and ``peaked`` regimes.

Then the checks that need no tolerance:
 * bounds that describe one document per row give the bits of the call
   without bounds;
 * a document's five outputs do not move by a bit when every other
   document's q, k, v and dout rows are replaced (flat inputs, for the reason
   test_attention_oracle_gpu.py gives: the wave-uniform defer branch cannot
   differ between the two runs);
 * a document's first row returns its own value row;
 * qkv_rope with doc_start gives, on each document's rows, the bits the
   plain call gives for that document as a [1, L] batch, forward and
   backward;
 * malformed bounds finish without a GPU error (the kernels clamp every
   value they derive from the tensors into the plain causal kernel's range;
   the outputs are not compared).
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
import kernel_oracle_attention_docs as kd
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

CASES = {i: (s, tuple(map(tuple, lay))) for i, (s, lay) in
         zip(kd.IDS, kd.CASES)}
NAMES = ["o", "lse", "dq", "dk", "dv"]


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def problem(case, regime):
    """bf16 inputs and the specs of all five outputs, once per case."""
    shape, layouts = CASES[case]
    qkvd = ka.inputs(*shape, True, regime=regime)
    return qkvd, kd.attention(*qkvd, layouts)


@functools.lru_cache(maxsize=None)
def on_gpu(case, regime):
    shape, layouts = CASES[case]
    ds, de = kd.bounds(layouts, shape[1])
    return tuple(t.to(dev()) for t in problem(case, regime)[0]) + \
        (ds.to(dev()), de.to(dev()))


def run(q, k, v, do, ds=None, de=None):
    """Forward, then backward on the forward's own o and lse."""
    if ds is None:
        o, lse = ops._C.attn_fwd(q, k, v, True)
        dq, dk, dv = ops._C.attn_bwd(q, k, v, o, lse, do, True)
    else:
        o, lse = ops._C.attn_fwd(q, k, v, True, 0, ds)
        dq, dk, dv = ops._C.attn_bwd(q, k, v, o, lse, do, True, False, 1,
                                     ds, de)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def rows(name, t, a, L):
    return t[..., a:a + L] if name == "lse" else t[:, a:a + L]


@pytest.mark.parametrize("regime", kd.REGIMES)
@pytest.mark.parametrize("case", list(CASES))
def test_against_per_document_oracle(case, regime):
    (q, k, v, _), specs = problem(case, regime)
    shape, layouts = CASES[case]
    got = run(*on_gpu(case, regime))
    ka.check_all(f"docs[{case},{regime}]", got, specs)
    # a document's first row sees one key: p = 1, O is that value row
    hk = torch.arange(shape[2]) // (shape[2] // shape[3])
    o = got["o"].cpu()
    for b, lengths in enumerate(layouts):
        for a, _ in kd.offsets(lengths):
            assert torch.equal(o[b, a], v[b, a][hk]), (b, a)


@pytest.mark.parametrize("case", ["2x576x8x2x128", "1x200x2x1x64"])
def test_one_document_per_row_is_the_plain_kernel_bitwise(case):
    q, k, v, do, ds, _ = on_gpu(case, "peaked")
    S = q.shape[1]
    plain = run(q, k, v, do)
    got = run(q, k, v, do, torch.zeros_like(ds), torch.full_like(ds, S))
    for n in NAMES:
        assert torch.equal(got[n], plain[n]), n


def other(t, seed):
    """Ordinary random values of the same kind as the flat inputs."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(t.shape, generator=g) * 0.5).bfloat16().to(t.device)


@pytest.mark.parametrize("case", ["1x128x2x2x64", "1x320x2x1x128",
                                  "1x520x4x1x128"])
def test_documents_are_isolated_bitwise(case):
    """Both directions at once: for every document, all rows in front of it
    and all rows behind it are replaced, and its own outputs may not move."""
    _, layouts = CASES[case]
    q, k, v, do, ds, de = on_gpu(case, "flat")
    base = run(q, k, v, do, ds, de)
    for a, L in kd.offsets(layouts[0]):
        moved = []
        for i, t in enumerate((q, k, v, do)):
            t2 = other(t, 90 + i)
            t2[:, a:a + L] = t[:, a:a + L]
            moved.append(t2)
        got = run(*moved, ds, de)
        for n in NAMES:
            assert torch.equal(rows(n, got[n], a, L),
                               rows(n, base[n], a, L)), (n, a, L)
        # the replaced rows did move
        assert not torch.equal(got["o"], base["o"])
        assert not torch.equal(got["dk"], base["dk"])


def _rope_table(S, D):
    half = D // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, half, dtype=torch.float64)
                             / half))
    ang = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return (ang.cos().float().contiguous().to(dev()),
            ang.sin().float().contiguous().to(dev()))


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (2, 1, 128)])
def test_qkv_rope_restarts_per_document_bitwise(Hq, Hkv, D):
    B, S = 2, 200
    layouts = [[33, 31, 72, 64], [200]]
    ds, _ = kd.bounds(layouts, S)
    ds = ds.to(dev())
    cos, sin = _rope_table(S, D)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    qkv = qkv.to(dev())
    grads = [torch.randn(B, S, h, D, generator=g).bfloat16().to(dev())
             for h in (Hq, Hkv, Hkv)]
    fwd = ops._C.qkv_rope_fwd(qkv, cos, sin, Hq, Hkv, D, ds)
    bwd = ops._C.qkv_rope_bwd(*grads, cos, sin, ds)
    plain = ops._C.qkv_rope_fwd(qkv, cos, sin, Hq, Hkv, D)
    moved = False
    for b, lengths in enumerate(layouts):
        for a, L in kd.offsets(lengths):
            alone = ops._C.qkv_rope_fwd(qkv[b:b + 1, a:a + L].contiguous(),
                                        cos, sin, Hq, Hkv, D)
            for got, want in zip(fwd, alone):
                assert torch.equal(got[b:b + 1, a:a + L], want), (b, a)
            alone = ops._C.qkv_rope_bwd(
                *(t[b:b + 1, a:a + L].contiguous() for t in grads), cos, sin)
            assert torch.equal(bwd[b:b + 1, a:a + L], alone), (b, a)
            if a:
                moved |= not torch.equal(fwd[0][b, a:a + L],
                                         plain[0][b, a:a + L])
    assert moved     # positions really restarted
    # the public op, through autograd
    x = qkv.clone().requires_grad_(True)
    q, k, v = ops.qkv_rope(x, cos, sin, Hq, Hkv, D, doc_start=ds)
    for got, want in zip((q, k, v), fwd):
        assert torch.equal(got, want)
    torch.autograd.backward((q, k, v), grads)
    assert torch.equal(x.grad, bwd)


def test_public_attention_matches_the_binding_and_derives_doc_end():
    case = "1x200x2x1x64"
    q, k, v, do, ds, de = on_gpu(case, "flat")
    want = run(q, k, v, do, ds, de)
    for end in (de, None):
        qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qr, kr, vr, causal=True, doc_start=ds, doc_end=end)
        o.backward(do)
        assert torch.equal(o, want["o"])
        for n, t in (("dq", qr), ("dk", kr), ("dv", vr)):
            assert torch.equal(t.grad, want[n]), n


def test_other_variants_and_noncausal_refuse_bounds():
    q, k, v, do, ds, de = on_gpu("1x128x2x2x64", "flat")
    o, lse = ops._C.attn_fwd(q, k, v, True, 0, ds)
    with pytest.raises(RuntimeError):
        ops._C.attn_fwd(q, k, v, True, 1, ds)
    with pytest.raises(RuntimeError):
        ops._C.attn_fwd(q, k, v, False, 0, ds)
    for causal, split, dqv in ((False, False, 1), (True, True, 1),
                               (True, False, 0), (True, False, 2)):
        with pytest.raises(RuntimeError):
            ops._C.attn_bwd(q, k, v, o, lse, do, causal, split, dqv, ds, de)
    with pytest.raises(RuntimeError):
        ops._C.attn_bwd(q, k, v, o, lse, do, True, False, 1, ds, None)
    with pytest.raises(RuntimeError):
        ops._C.attn_fwd(q, k, v, True, 0, ds.long())
    with pytest.raises(ValueError):
        ops.attention(q, k, v, causal=False, doc_start=ds)


@pytest.mark.parametrize("kind", ["negative", "above_row", "decreasing",
                                  "huge"])
def test_malformed_bounds_stay_in_bounds(kind):
    """Nothing reads the tensors on the host, so malformed bounds reach the
    kernels; every value derived from them is clamped into the range the
    plain causal kernel touches. The run must finish; outputs are not
    compared."""
    q, k, v, do, ds, de = on_gpu("1x128x2x2x64", "flat")
    S = q.shape[1]
    idx = torch.arange(S, dtype=torch.int32, device=dev()).unsqueeze(0)
    if kind == "negative":
        ds2, de2 = -1 - idx, -idx
    elif kind == "above_row":
        ds2, de2 = idx + 37, idx - 5
    elif kind == "decreasing":
        ds2, de2 = (S - 1 - idx).contiguous(), (S - idx).contiguous()
    else:
        ds2 = torch.full_like(idx, 2 ** 31 - 1)
        de2 = torch.full_like(idx, -2 ** 31)
    got = run(q, k, v, do, ds2.contiguous(), de2.contiguous())
    torch.cuda.synchronize()
    specs = problem("1x128x2x2x64", "flat")[1]
    for n, t in got.items():
        assert t.shape == specs[n].ref.shape, n
    # and the device still computes: the valid bounds give the valid result
    ka.check_all("after_malformed", run(q, k, v, do, ds, de), specs)

"""GPU numerics: every training attention kernel against the fp64
references of ``kernel_oracle_attention.py``, per element, by its rule.

Every shape goes through every kernel, in two regimes (``flat``: near-
uniform softmax; ``peaked``: scaled scores of std 3, which puts both the
defer and the rescale branch of the online softmax in play - asserted from
the fp64 scores before a kernel runs). Seven launches per (shape, regime):
attn_fwd variants 0 (v4) and 1 (v3); attn_bwd fused and split at the default
dQ kernel, and dQ variants 0 and 2 with the fused kernel. Every backward is
fed the variant-0 forward's o and lse.

Then the checks that need no tolerance: row 0 of a causal case is its one
value row, and outputs must not move by a bit when data they may not read
changes (keys past a causal cut, the other batch, the other kv head). A
masked element contributes an exact zero, so any difference there is a read
past the mask. These use the flat inputs: there every tile after a row's
first takes the defer branch, whatever the rows that share its wave hold, so
the wave-uniform branch cannot differ between the two runs.
"""
import functools

import pytest
import torch

import kernel_oracle_attention as ka
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

CASES = [(s, r) for s in ka.SHAPES for r in ka.REGIMES] + \
    [(s, r) for r, s in ka.SPECIAL]
IDS = [f"{'x'.join(map(str, s[:5]))}{'c' if s[5] else 'n'}-{r}"
       for s, r in CASES]
# name -> (split, dq_variant)
BWD_PATHS = {"fused": (False, 1), "split": (True, 1), "dq_v2": (False, 0),
             "dq_plain": (False, 2)}


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def problem(shape, regime):
    """bf16 inputs and the specs of all five outputs, once per case."""
    qkvd = ka.inputs(*shape, regime=regime)
    if regime == "peaked" and shape[1] > ka.BN + 1:
        rise = ka.tile_max_raises(ka.scores(qkvd[0], qkvd[1], shape[5]))
        assert (rise > ka.DEFER_THR).any() and (rise < ka.DEFER_THR).any()
    return qkvd, ka.attention(*qkvd, shape[5])


@functools.lru_cache(maxsize=None)
def on_gpu(shape, regime):
    return tuple(t.to(dev()) for t in problem(shape, regime)[0])


@functools.lru_cache(maxsize=None)
def forward(shape, regime, variant):
    q, k, v, _ = on_gpu(shape, regime)
    return ops._C.attn_fwd(q, k, v, shape[5], variant)


@pytest.mark.parametrize("variant", [0, 1], ids=["v4", "v3"])
@pytest.mark.parametrize("shape,regime", CASES, ids=IDS)
def test_forward(shape, regime, variant):
    (q, k, v, _), specs = problem(shape, regime)
    o, lse = forward(shape, regime, variant)
    ka.check_all(f"fwd_v{4 - variant}[{IDS[CASES.index((shape, regime))]}]",
                 {"o": o, "lse": lse}, specs)
    if shape[5]:
        # row 0 sees one key: p = 1 exactly, O is that value row, bitwise
        # (its LSE, s_00, is judged by the rule above like every other)
        hk = torch.arange(shape[2]) // (shape[2] // shape[3])
        assert torch.equal(o[:, 0].cpu(), v[:, 0][:, hk])


@pytest.mark.parametrize("path", list(BWD_PATHS))
@pytest.mark.parametrize("shape,regime", CASES, ids=IDS)
def test_backward(shape, regime, path):
    _, specs = problem(shape, regime)
    q, k, v, do = on_gpu(shape, regime)
    o, lse = forward(shape, regime, 0)
    split, dq_variant = BWD_PATHS[path]
    dq, dk, dv = ops._C.attn_bwd(q, k, v, o, lse, do, shape[5], split,
                                 dq_variant)
    ka.check_all(f"bwd_{path}[{IDS[CASES.index((shape, regime))]}]",
                 {"dq": dq, "dk": dk, "dv": dv}, specs)


# --------------------------------------------------------------------------
# Exact checks
# --------------------------------------------------------------------------
def run_all(q, k, v, do, causal):
    """Every kernel's outputs, keyed by kernel; backward fed by forward 0."""
    out = {}
    for variant in (0, 1):
        o, lse = ops._C.attn_fwd(q, k, v, causal, variant)
        out[f"o_v{variant}"], out[f"lse_v{variant}"] = o, lse
    o, lse = out["o_v0"], out["lse_v0"]
    for path, (split, dq_variant) in BWD_PATHS.items():
        dq, dk, dv = ops._C.attn_bwd(q, k, v, o, lse, do, causal, split,
                                     dq_variant)
        out[f"dq_{path}"], out[f"dk_{path}"], out[f"dv_{path}"] = dq, dk, dv
    return out


def other(t, seed):
    """Ordinary random values of the same kind as the flat inputs."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(t.shape, generator=g) * 0.5).bfloat16().to(t.device)


@pytest.mark.parametrize("shape,cut", [((1, 328, 4, 1, 128, True), 173),
                                       ((2, 576, 8, 2, 128, True), 301)],
                         ids=["328", "576"])
def test_causal_isolation(shape, cut):
    assert cut % 32 and cut % ka.BN
    q, k, v, do = on_gpu(shape, "flat")
    base = run_all(q, k, v, do, True)
    # keys and values from the cut on change: rows before it may not move
    k2, v2 = k.clone(), v.clone()
    k2[:, cut:], v2[:, cut:] = other(k[:, cut:], 91), other(v[:, cut:], 92)
    got = run_all(q, k2, v2, do, True)
    for name in got:
        if name.startswith("o_") or name.startswith("dq_"):
            assert torch.equal(got[name][:, :cut], base[name][:, :cut]), name
        elif name.startswith("lse_"):
            assert torch.equal(got[name][..., :cut], base[name][..., :cut]), \
                name
    assert not torch.equal(got["o_v0"][:, cut:], base["o_v0"][:, cut:])
    # queries and dO before the cut change: dK, dV from the cut on may not
    q2, do2 = q.clone(), do.clone()
    q2[:, :cut], do2[:, :cut] = other(q[:, :cut], 93), other(do[:, :cut], 94)
    got = run_all(q2, k, v, do2, True)
    for name in got:
        if name.startswith("dk_") or name.startswith("dv_"):
            assert torch.equal(got[name][:, cut:], base[name][:, cut:]), name
    assert not torch.equal(got["dk_fused"][:, :cut], base["dk_fused"][:, :cut])


def test_batch_and_head_isolation():
    """S = 264 is ragged: batch 0's last tile overlaps batch 1's rows in
    memory, and the fused dK+dV grid of 8 blocks is reordered."""
    shape = (2, 264, 4, 2, 64, True)
    q, k, v, do = on_gpu(shape, "flat")
    base = run_all(q, k, v, do, True)
    one = run_all(q[:1].contiguous(), k[:1].contiguous(),
                  v[:1].contiguous(), do[:1].contiguous(), True)
    for name in base:
        assert torch.equal(base[name][:1], one[name]), name
    # kv head 1's keys and values change: kv head 0 and its q heads may not
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 1], v2[:, :, 1] = other(k[:, :, 1], 95), other(v[:, :, 1], 96)
    got = run_all(q, k2, v2, do, True)
    rep = shape[2] // shape[3]
    for name in base:
        if name.startswith("lse_"):
            same = torch.equal(got[name][:, :rep], base[name][:, :rep])
        elif name.startswith("dk_") or name.startswith("dv_"):
            same = torch.equal(got[name][:, :, 0], base[name][:, :, 0])
        else:
            same = torch.equal(got[name][:, :, :rep], base[name][:, :, :rep])
        assert same, name
    assert not torch.equal(got["o_v0"][:, :, rep:], base["o_v0"][:, :, rep:])

"""fp64 references for document-masked attention (packed documents).

A document-masked row is, exactly, each document run through causal
attention on its own: query i sees the keys doc_start[i] .. i and nothing
else, so no term crosses a document boundary in O, LSE, dQ, dK or dV. The
reference is therefore ``kernel_oracle_attention.attention`` (imported, not
changed), applied per (batch, document) to that document's rows of q, k, v
and dout, concatenated along S and judged by that module's per-element rule
with no element excluded.

ONE adjustment, derived, not fitted. The oracle counts its fp32 chain lengths
from ``n_tiles(S)``, the number of 64-key tiles of a row that starts at a
tile edge. A document of L tokens that starts at row offset a of the packed
row lies across up to

    ceil(((a mod 64) + L) / 64)

key tiles of the forward and dQ kernels, and as many 64-row groups of q rows
in dK+dV, one more than n_tiles(L) when it straddles an edge. Each
document's specs are built with the oracle's module-level ``n_tiles`` bound
to that count for the duration of the call. ``kred`` is monotone, so this
only widens the fp32 term, which is the small one.

A concatenated spec holds k = 1 and scale = k_d * scale_d of its documents:
the rule uses only the product k * 2^-23 * scale.

``whole_row`` is a second, independent route to the same numbers: the
oracle's plain fp64 computation over the whole row with its mask replaced by
the document mask. The CPU test holds the two against each other, and uses
its ``start_shift`` for the deliberately wrong mask.
"""
from __future__ import annotations

import math

import torch

import kernel_oracle_attention as ka

BN = ka.BN


def doc_tiles(a: int, L: int) -> int:
    return math.ceil(((a % BN) + L) / BN)


def offsets(lengths):
    out, a = [], 0
    for L in lengths:
        out.append((a, L))
        a += L
    return out


def bounds(layouts, S: int):
    """layouts: per batch, the list of document lengths (summing to S).
    Returns int32 doc_start, doc_end of shape [B, S]."""
    ds = torch.empty(len(layouts), S, dtype=torch.int32)
    de = torch.empty(len(layouts), S, dtype=torch.int32)
    for b, lengths in enumerate(layouts):
        assert sum(lengths) == S and min(lengths) >= 1, (lengths, S)
        for a, L in offsets(lengths):
            ds[b, a:a + L] = a
            de[b, a:a + L] = a + L
    return ds, de


class _bound:
    """Replace a module-level name of the oracle for the duration of a
    call."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.saved = getattr(ka, self.name)
        setattr(ka, self.name, self.value)

    def __exit__(self, *exc):
        setattr(ka, self.name, self.saved)


def _cat(specs, dim):
    return ka.AttnSpec(torch.cat([s.ref for s in specs], dim),
                       torch.cat([s.mid for s in specs], dim),
                       torch.cat([s.k * s.scale for s in specs], dim),
                       1.0, specs[0].bf16)


def attention(q, k, v, dout, layouts) -> dict:
    """Specs of o, lse, dq, dk, dv for the packed rows, as
    ``kernel_oracle_attention.attention`` returns them for plain ones."""
    names = ["o", "lse", "dq", "dk", "dv"]
    rows = []
    for b, lengths in enumerate(layouts):
        docs = []
        for a, L in offsets(lengths):
            sl = [t[b:b + 1, a:a + L].contiguous() for t in (q, k, v, dout)]
            nt = doc_tiles(a, L)
            with _bound("n_tiles", lambda S, nt=nt: nt):
                docs.append(ka.attention(*sl, True))
        # lse is [B, Hq, S]; the others [B, S, H, D]
        rows.append({n: _cat([d[n] for d in docs], 2 if n == "lse" else 1)
                     for n in names})
    return {n: _cat([r[n] for r in rows], 0) for n in names}


def whole_row(q, k, v, dout, layouts, start_shift: int = 0) -> dict:
    """The five outputs (fp64) from one computation over the whole row under
    the document mask. start_shift = -1 lets every document but a row's
    first see one key of the document in front of it: the wrong mask."""
    S = q.shape[1]
    ds, _ = bounds(layouts, S)
    i = torch.arange(S).view(S, 1)
    j = torch.arange(S).view(1, S)
    outs = []
    for b in range(len(layouts)):
        lo = (ds[b].long() + start_shift).clamp(min=0).view(S, 1)
        ok = (j <= i) & (j >= lo)
        sl = [t[b:b + 1].contiguous() for t in (q, k, v, dout)]
        with _bound("_allowed", lambda *a, ok=ok, **kw: ok):
            outs.append(ka.wrong_reference(*sl, True))
    return {n: torch.cat([o[n] for o in outs], 0) for n in outs[0]}


# (B, S, Hq, Hkv, D), document lengths per batch: the smallest rows at which
# each kernel can go wrong.
CASES = [
    # boundary mid-tile and inside one wave's 32 rows (64-69 | 70-95): tile 0
    # is live for the wave and all -inf for the second document's rows
    ((1, 128, 2, 2, 64), [[70, 58]]),
    # boundaries on tile edges: off-by-one in the uniform flags, loop start
    ((1, 256, 2, 1, 128), [[64, 64, 128]]),
    # a one-token document at row 0; a boundary on the 256-row block edge:
    # the second q block starts its key loop at tile 4, key block 0's q loop
    # ends at 256 (the "next head" step with m_end < S)
    ((1, 320, 2, 1, 128), [[1, 255, 64]]),
    # per-batch indexing; rep = 4 in the dK+dV head loop with an early
    # m_end; batch 1 is one document
    ((2, 576, 8, 2, 128), [[300, 276], [576]]),
    # several documents inside one wave's rows, ragged row tail
    ((1, 200, 2, 1, 64), [[33, 31, 72, 64]]),
    # one document across three 256-row blocks, short neighbours
    ((1, 520, 4, 1, 128), [[10, 500, 10]]),
]
IDS = ["x".join(map(str, s)) for s, _ in CASES]
REGIMES = ka.REGIMES

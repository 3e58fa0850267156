"""fp64 reference of ``ops.sample_tokens`` and its comparison rule, by the
ONE rule of ``kernel_oracle.py`` (imported, not changed). Nothing here is
imported from ``torch_on_k8s_amd.ops``; the Philox below is this module's
own and is checked against the Random123 known answers by
``test_sampler_oracle.py``.

Semantics, per row (T, k, p, u; u from Philox4x32-10 unless given):

  T <= 0      the lowest index of the maximum logit
  softmax     z_i = (l_i - max l) / T, e_i = exp(z_i); exp(-inf) = 0
  top-k       0 < k < V: keep l_i >= the k-th largest logit (ties kept)
  top-p       p < 1: over the distinct surviving values, descending, the
              first at which the cumulative mass reaches p * M (M the
              surviving mass) is the cut; keep l_i >= cut. p <= 0: the top
              tie group only
  draw        C = running sum of the kept e_i in ascending index, M its
              total: the first kept index with C_i > u * M, else the last
              kept index with e_i > 0

A sampler does not return a number but an index, so the rule is applied to
the quantity the index is decided by: token t is ACCEPTED iff it is kept,
e_t > 0 and

    C_{t-1} - delta <= u * M < C_t + delta,   delta = k * 2^-23 * S,
    S = sum over kept i of e_i * (1 + |z_i|)

(the factor 1 + |z| as for every exp-based output of kernel_oracle), or it
is the last kept index with e_t > 0 and u * M >= M - delta (the fallback).
``k`` is counted from the chains of ``sample.hip`` as written, see
``k_sample``.

Two conditions keep the rule from hiding a failure; ``row_spec`` reports
both and the tests assert them on the reference alone:

  * top-p: the cumulative mass on either side of the cut differs from
    p * M by at least 8 * delta (delta over the top-k survivors), so the
    kept set is unambiguous and only one is accepted;
  * at most 25 % of the rows of a case may accept more than one token.

The ``*_shift`` / ``cdf_desc`` arguments build deliberately wrong
references.
"""
from __future__ import annotations

import functools
import math

import torch

import kernel_oracle as ko

M32 = 0xFFFFFFFF
TILE = 512       # elements per draw tile of sample_tokens_kernel (64 x 8)
GAP = 8.0        # top-p cut must clear p*M by GAP * delta
AMBIGUOUS_CAP = 0.25


# --------------------------------------------------------------------------
# Philox4x32-10
# --------------------------------------------------------------------------
def philox4x32_10(counter, key):
    c = [int(x) & M32 for x in counter]
    k = [int(x) & M32 for x in key]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32,
             (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return tuple(c)


def uniform(seed: int, counter: int) -> float:
    s = int(seed) & (2 ** 64 - 1)
    c = int(counter) & (2 ** 64 - 1)
    out = philox4x32_10((c & M32, c >> 32, 0, 0), (s & M32, s >> 32))
    return (out[0] >> 8) * 2.0 ** -24


# --------------------------------------------------------------------------
# k, counted from sample.hip
# --------------------------------------------------------------------------
K_EXP = 3   # units of e*(1+|z|) per mass: __expf is 1 unit on e; on z the
#             subtraction (0.5), 1/T (1), the product (0.5) and __expf's own
#             a*log2(e) (0.5) are 2.5 units of |z|*e


def k_sample(V: int) -> float:
    """Budget of the comparison C_t > u*M for a row of V logits.

    A lane sums its 8 masses serially (8), a wave scan adds 6 levels; a
    tile's mass is the last lane of that scan. Wave 0 gives lane l the
    tiles [l*per, (l+1)*per), per = ceil(ntiles / 64): per serial adds, 6
    scan levels. So M has 8 + 6 + per + 6 roundings on its longest chain.
    C_t is tile prefix (per + 6, then up to per more to reach the tile) +
    lane prefix (8 + 6) + the own-lane serial walk (8) + the two joins (2).
    u*M is one more rounding. Each mass carries K_EXP units, in C and in M.
    """
    ntiles = math.ceil((V + 7) / TILE)
    per = math.ceil(ntiles / 64)
    d_m = 8 + 6 + per + 6
    d_c = (per + 6 + per) + (8 + 6) + 8 + 2
    return ko.kred(d_c) + ko.kred(d_m) + 1 + 2 * K_EXP


def k_top_p(V: int) -> float:
    """Budget of the top-p comparison cum >= p*M in sample.hip. cum: a
    thread folds its 32 keys serially (32 fma), 6 scan levels, 16 waves in
    order, the carry of the first half (1), then the walk inside the group
    (32). M is such a chain too when top-k is on; without top-k it is the
    row sum: 8 serial adds per 16-byte vector of a thread, ceil(V / 8192)
    vectors, 2 for the row's ends, a 6-level butterfly and 16 waves in
    order. p*M is one rounding. It must stay below GAP * k_sample(V) for
    the gap condition to cover it (asserted by the tests)."""
    d_cum = 32 + 6 + 16 + 1 + 32
    d_row = 8 * math.ceil(V / 8192) + 2 + 6 + 16
    return ko.kred(d_cum) + ko.kred(max(d_cum, d_row)) + 1 + 2 * K_EXP


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
def row_spec(l, T, k, p, u, *, k_shift=0, cdf_desc=False) -> dict:
    """l: 1-D logits (any dtype; the bf16 values the kernel sees).
    Returns accept (bool [V]), kept (bool [V]), gap_ok, n_accept."""
    l = ko.f64(l).reshape(-1)
    V = l.numel()
    acc = torch.zeros(V, dtype=torch.bool)
    if not T > 0:
        acc[int(torch.argmax(l))] = True
        return {"accept": acc, "kept": acc.clone(), "gap_ok": True,
                "n_accept": 1, "greedy": True}
    budget = k_sample(V) * ko.U
    z = (l - l.max()) / T
    e = torch.exp(z)
    w = e * (1 + z.abs().masked_fill(e == 0, 0.0))
    # Both thresholds are read off ONE descending sort of the row (the op's
    # CPU path is built from topk / unique / index_add_ instead): the k-th
    # value is the k-th entry; a tie group ends where the next entry is
    # smaller, and the cumulative mass at a group's end is the running sum
    # over the sorted entries there.
    ls, order = torch.sort(l, descending=True, stable=True)
    es = e[order]
    kk = k + k_shift if 0 < k < V else k
    n = V
    if 0 < kk < V:
        n = int((ls >= ls[kk - 1]).sum())         # survivors, ties included
    cut = ls[n - 1]
    gap_ok = True
    if p < 1:
        run = torch.cumsum(es[:n], 0)
        last = torch.ones(n, dtype=torch.bool)    # last entry of a tie group
        last[:-1] = ls[1:n] < ls[:n - 1]
        ends = torch.nonzero(last).flatten()
        cum = run[ends]
        target = p * cum[-1]
        at = 0
        if p > 0:
            at = int(torch.nonzero(cum >= target).flatten()[0])
            delta_p = budget * float(w[order[:n]].sum())
            below = float(cum[at - 1]) if at > 0 else -math.inf
            gap_ok = (float(cum[at]) - float(target) >= GAP * delta_p and
                      float(target) - below >= GAP * delta_p)
        cut = ls[ends[at]]
    kept = l >= cut
    ek = torch.where(kept, e, torch.zeros_like(e))
    if cdf_desc:      # a wrong CDF order: descending logit instead of index
        order = torch.argsort(l, descending=True, stable=True)
        C = torch.empty_like(ek)
        C[order] = torch.cumsum(ek[order], 0)
        Cprev = C - ek
    else:
        C = torch.cumsum(ek, 0)
        Cprev = C - ek
    M = float(ek.sum())
    delta = budget * float(w[kept].sum())
    t = u * M
    live = kept & (e > 0)             # a logit of -inf is never returned
    acc = live & (Cprev - delta <= t) & (t < C + delta)
    if t >= M - delta:
        acc[int(torch.nonzero(live).flatten()[-1])] = True
    return {"accept": acc, "kept": kept, "gap_ok": gap_ok,
            "n_accept": int(acc.sum()), "greedy": False}


def specs(logits, temperature, top_k, top_p, seed, counter, u=None, *,
          counter_shift=0, k_shift=0, cdf_desc=False) -> list:
    """One row_spec per row of logits [B, V]; parameters are sequences."""
    out = []
    for b in range(logits.shape[0]):
        ub = (float(u[b]) if u is not None
              else uniform(int(seed[b]), int(counter[b]) + counter_shift))
        out.append(row_spec(logits[b], float(temperature[b]), int(top_k[b]),
                            float(top_p[b]), ub, k_shift=k_shift,
                            cdf_desc=cdf_desc))
    return out


def rejected(tokens, specs_) -> list:
    """Rows whose token the reference does not accept."""
    toks = [int(t) for t in tokens]
    return [b for b, (t, s) in enumerate(zip(toks, specs_))
            if not (0 <= t < s["accept"].numel() and bool(s["accept"][t]))]


def check(name: str, tokens, specs_) -> None:
    """Print what was measured, then fail on any rejected row and on either
    condition that would let the rule hide a failure."""
    bad = rejected(tokens, specs_)
    n = len(specs_)
    amb = sum(s["n_accept"] > 1 for s in specs_)
    gaps = [b for b, s in enumerate(specs_) if not s["gap_ok"]]
    print(f"SAMPLER {name}: rows={n} rejected={len(bad)} ambiguous={amb} "
          f"max_accept={max(s['n_accept'] for s in specs_)} "
          f"gap_fail={len(gaps)}")
    assert not gaps, f"{name}: top-p cut within {GAP} delta in rows {gaps}"
    assert amb <= AMBIGUOUS_CAP * n, (
        f"{name}: {amb}/{n} rows accept more than one token")
    assert not bad, f"{name}: rows {bad} returned a token outside the " \
                    f"accepted set"


# --------------------------------------------------------------------------
# the cases shared by the CPU and the GPU tests
# --------------------------------------------------------------------------
VOCABS = (512, 1001, 32000, 50257, 128256)
TEMPS = (0.5, 1.0, 1.5)
TOP_PS = (1.0, 0.9, 0.5, 0.0)


def mixes(V: int) -> list:
    """Every (T, top_k, top_p) of the grid, 60 of them."""
    return [(T, k, p) for T in TEMPS for k in (0, 1, 50, V, V + 5)
            for p in TOP_PS]


def make_logits(B: int, V: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return ko.q16(4.0 * torch.randn(B, V, generator=g))


def make_case(V: int, B: int, base: int, seed: int) -> dict:
    """B rows: rows 1, 5, ... are greedy when B >= 3, the others take the
    mixes base, base+1, ... in order. All parameters as CPU tensors, and
    "specs", the reference of every row, computed once.

    A row whose top-p cut lies within GAP * delta of p * M (decided on the
    reference alone) cannot be judged exactly; its logits are drawn again
    from the next seed until the cut is clear."""
    mx = mixes(V)
    T, K, P = [], [], []
    n = base
    for r in range(B):
        if B >= 3 and r % 4 == 1:
            t, k, p = 0.0, 7, 0.3        # ignored by a greedy row
        else:
            t, k, p = mx[n % len(mx)]
            n += 1
        T.append(t), K.append(k), P.append(p)
    c = {
        "temperature": torch.tensor(T, dtype=torch.float32),
        "top_k": torch.tensor(K, dtype=torch.int32),
        "top_p": torch.tensor(P, dtype=torch.float32),
        "seed": torch.arange(B, dtype=torch.long) * 7919 + seed,
        "counter": torch.arange(B, dtype=torch.int32) + 3 * base,
        "next": n,
    }
    rows, ref, redrawn = [], [], 0
    for r in range(B):
        u = uniform(int(c["seed"][r]), int(c["counter"][r]))
        for attempt in range(64):
            l = make_logits(1, V, seed * 64 + r * 4099 + attempt * 104729)[0]
            s = row_spec(l, float(c["temperature"][r]), int(c["top_k"][r]),
                         float(c["top_p"][r]), u)
            if s["gap_ok"]:
                break
        rows.append(l), ref.append(s)
        redrawn += attempt > 0
    c["redrawn"] = redrawn
    c["logits"] = torch.stack(rows)
    c["specs"] = ref
    return c


@functools.lru_cache(maxsize=None)
def grid_cases(V: int) -> list:
    """B = 1 and B = 3 once, then B = 8 until all 60 mixes were drawn."""
    cases = [make_case(V, 1, 17, CASE_SEED + V),
             make_case(V, 3, 41, CASE_SEED + V + 1)]
    n, i = 0, 0
    while n < len(mixes(V)):
        c = make_case(V, 8, n, CASE_SEED + V + 2 + i)
        cases.append(c)
        n, i = c["next"], i + 1
    return cases


CASE_SEED = 20240


def _finish(c: dict) -> dict:
    """Fill in the defaults of a planted case and its reference."""
    B = c["logits"].shape[0]
    c.setdefault("seed", torch.arange(B, dtype=torch.long) + 99)
    c.setdefault("counter", torch.arange(B, dtype=torch.int32))
    c["temperature"] = torch.tensor(c["temperature"], dtype=torch.float32)
    c["top_k"] = torch.tensor(c["top_k"], dtype=torch.int32)
    c["top_p"] = torch.tensor(c["top_p"], dtype=torch.float32)
    if c.get("u") is not None:
        c["u"] = torch.tensor(c["u"], dtype=torch.float32)
    c["specs"] = specs(c["logits"], c["temperature"], c["top_k"], c["top_p"],
                       c["seed"], c["counter"], c.get("u"))
    return c


@functools.lru_cache(maxsize=None)
def planted_cases() -> dict:
    """name -> case. V = 1001: misaligned rows, a tail, two draw tiles."""
    V = 1001
    NEG = float("-inf")
    out = {}

    # a tie group of 7 straddling the 50th place: ranks 47..53 share a value
    l = make_logits(4, V, 7)
    for b in range(4):
        order = torch.argsort(l[b].double(), descending=True, stable=True)
        l[b, order[47:54]] = l[b, order[47]].clone()
    out["tie_at_k"] = _finish({
        "logits": l, "temperature": [1.0, 0.5, 1.5, 1.0],
        "top_k": [50, 50, 50, 50], "top_p": [1.0, 1.0, 0.9, 0.5]})
    assert all(int(s["kept"].sum()) == 54
               for s in out["tie_at_k"]["specs"][:2])

    # -inf logits: every second token, and all but one
    l = make_logits(6, V, 8)
    l[:4, ::2] = NEG
    l[4:] = NEG
    l[4, 777] = 1.5
    l[5, 0] = -3.0
    out["neg_inf"] = _finish({
        "logits": l, "temperature": [1.0, 0.5, 1.5, 0.0, 1.0, 0.0],
        "top_k": [0, 50, 0, 0, 0, 3], "top_p": [1.0, 1.0, 0.9, 1.0, 0.5, 1.0]})
    assert [int(s["accept"].nonzero()[0]) for s in
            out["neg_inf"]["specs"][4:]] == [777, 0]

    # no filter, u one step below 1 and a tail of -inf: whatever rounding
    # does to u * M, the token is the last one with mass, not the last one.
    # 40 unit-scale logits, so that token's mass is far above delta
    g = torch.Generator().manual_seed(10)
    l = ko.q16(torch.randn(4, 40, generator=g))
    l[:, 32:] = NEG
    l[:, 5] = NEG
    out["neg_inf_tail"] = _finish({
        "logits": l, "temperature": [1.0, 0.5, 1.5, 1.0],
        "top_k": [0, 0, 0, 40], "top_p": [1.0, 1.0, 1.0, 1.0],
        "u": [1.0 - 2.0 ** -24] * 4})
    assert all(s["accept"].nonzero().flatten().tolist() == [31]
               for s in out["neg_inf_tail"]["specs"])

    # a subnormal temperature (1/T overflows fp32) is the greedy limit
    l = make_logits(3, V, 12)
    l[:, 123] = 30.0
    out["tiny_T"] = _finish({
        "logits": l, "temperature": [1e-40, 1e-40, 1e-40],
        "top_k": [0, 50, 0], "top_p": [1.0, 1.0, 0.9]})
    assert all(s["accept"].nonzero().flatten().tolist() == [123]
               for s in out["tiny_T"]["specs"])

    # explicit u at both ends of [0, 1); top-k keeps the first and the last
    # kept mass well above delta, so one token is accepted
    l = make_logits(6, V, 9)
    top = 1.0 - 2.0 ** -24
    out["explicit_u"] = _finish({
        "logits": l, "temperature": [1.0, 1.0, 0.5, 0.5, 1.5, 1.5],
        "top_k": [50, 50, 20, 20, 50, 50],
        "top_p": [1.0, 1.0, 1.0, 1.0, 0.5, 0.5],
        "u": [0.0, top, 0.0, top, 0.0, top]})
    return out


def bad_input_case() -> dict:
    """Rows with NaN, +inf, only NaN, only -inf and only +inf under every
    kind of filter. No reference: the token is unspecified, only its range
    and the call's return are checked."""
    V = 1001
    kinds = 5
    settings = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0), (1.5, 0, 0.9),
                (1.0, 50, 0.5), (1.0, 0, 0.0)]
    l = make_logits(kinds * len(settings), V, 11)
    T, K, P = [], [], []
    for i, (t, k, p) in enumerate(settings):
        r = i * kinds
        l[r, 5::97] = float("nan")
        l[r + 1, 3::211] = float("inf")
        l[r + 2] = float("nan")
        l[r + 3] = float("-inf")
        l[r + 4] = float("inf")
        T += [t] * kinds
        K += [k] * kinds
        P += [p] * kinds
    B = l.shape[0]
    return {"logits": l,
            "temperature": torch.tensor(T, dtype=torch.float32),
            "top_k": torch.tensor(K, dtype=torch.int32),
            "top_p": torch.tensor(P, dtype=torch.float32),
            "seed": torch.arange(B, dtype=torch.long) + 5,
            "counter": torch.arange(B, dtype=torch.int32)}

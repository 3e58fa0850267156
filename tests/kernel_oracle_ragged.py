"""fp64 references for the ragged-batch decode ops, judged by the ONE rule
of ``kernel_oracle.py`` (imported, not changed).

``attention_decode_ragged``: the reference is ``kernel_oracle.
attention_decode`` applied to each sequence alone with that sequence's own
length; its ``ref`` and ``scale`` do not depend on how a kernel is built.
Only ``k`` does, and it is counted here from the chains of
``decode_ragged.hip`` as written (see ``k_decode_ragged``), by the rule of
that module's docstring. Nothing is fitted to a kernel's output.

``qkv_rope_append_``: ``kernel_oracle.rope`` with ``K_ROPE``, the B token
rows viewed as [1,B,H,D] against the table gathered at ``pos``.

The ``*_shift`` / ``roll`` arguments build deliberately wrong references.
"""
from __future__ import annotations

import math

import torch

import kernel_oracle as ko
from torch_on_k8s_amd.ops import decode_ragged_chunk

NW = 4  # waves per block of attn_decode_ragged_kernel


def ragged_inputs(B, Tmax, Hq, Hkv, D, lens, seed=0, nan_fill=True):
    """As kernel_oracle.decode_inputs, per sequence: one planted dominant
    key at len_b // 2 on kv head 0, NaN in every cache row >= len_b."""
    q = ko.bf(B, Hq, D, seed=seed)
    kc = ko.bf(B, Tmax, Hkv, D, seed=seed + 1)
    vc = ko.bf(B, Tmax, Hkv, D, seed=seed + 2)
    for b, n in enumerate(lens):
        if n > 0:
            kc[b, n // 2, 0] = ko.q16(q[b, 0] * 2.0)
        if nan_fill:
            kc[b, n:] = float("nan")
            vc[b, n:] = float("nan")
    return q, kc, vc


def k_decode_ragged(T: int, Tmax: int, num_splits: int, D: int) -> float:
    """fp32 budget of one sequence of length T.

    lpr = D/8 lanes hold a row, a wave holds g = 64/lpr lane groups, a
    block NW*g, and a block owns min(chunk, T) keys at most, so the longest
    serial chain of a lane group within a chunk has
        n = ceil(min(chunk, T) / (NW*g)) keys,
    3 roundings each (rescale, extend l, extend o; the kernel's 4-key batch
    spends 5 per 4 keys, which is within that). Then 2 roundings per merge
    level: log2(g) butterfly levels over the lane groups, NW serial folds
    over the waves, num_splits serial folds over the splits (none when the
    block writes the output itself), and the final divide:
        depth = 3n + 2*(log2 g + NW + splits) + 1.
    (l, o) are a quotient, hence the factor 2. A score is 8 serial fma, log2
    (lpr) shuffle adds and the scale: kred(8 + log2 lpr + 1). The +4 is the
    exps' ulps and the running max, as in kernel_oracle.attention_decode."""
    lpr = D // 8
    g = 64 // lpr
    chunk = decode_ragged_chunk(Tmax, num_splits)
    n = math.ceil(min(chunk, max(T, 1)) / (NW * g))
    levels = int(math.log2(g)) + NW + (num_splits if num_splits > 1 else 0)
    depth = 3 * n + 2 * levels + 1
    return 2 * ko.kred(depth) + ko.kred(8 + int(math.log2(lpr)) + 1) + 4


def attention_decode_ragged(q, kcache, vcache, lens, num_splits,
                            len_shift=0, roll=0, kv_head_shift=0) -> dict:
    """One Spec per sequence, named seq0..seq{B-1}; each covers [1,Hq,D]."""
    B, Hq, D = q.shape
    Tmax = kcache.shape[1]
    lens = [int(n) for n in lens]
    if roll:
        lens = lens[-roll:] + lens[:-roll]
    specs = {}
    for b in range(B):
        T = min(max(lens[b] + len_shift, 0), Tmax)
        if T == 0:
            z = torch.zeros(1, Hq, D, dtype=torch.float64)
            specs[f"seq{b}"] = ko.Spec(z, z.clone(), 1, True)
            continue
        s = ko.attention_decode(q[b:b + 1], kcache[b:b + 1], vcache[b:b + 1],
                                T, kv_head_shift=kv_head_shift)
        s.k = k_decode_ragged(T, Tmax, num_splits, D)
        specs[f"seq{b}"] = s
    return specs


def split_rows(out) -> dict:
    return {f"seq{b}": out[b:b + 1] for b in range(out.shape[0])}


def qkv_rope_append(qkv, cos, sin, pos, Tmax, Hq, Hkv, D, pos_shift=0):
    """Returns (specs, live). specs["q"] covers [B,Hq,D] (a zero row where
    pos is outside [0, Tmax)); specs["k"] covers the roped k rows of the
    live sequences only, [n_live,Hkv,D], in sequence order. v is a copy and
    is compared bitwise by the tests."""
    B = qkv.shape[0]
    pos = torch.as_tensor(pos).long()
    live = (pos >= 0) & (pos < Tmax)
    at = (pos.clamp(0, Tmax - 1) + pos_shift) % cos.shape[0]
    parts = qkv.view(1, B, Hq + 2 * Hkv, D)
    cg, sg = cos[at], sin[at]
    sq = ko.rope(parts[:, :, :Hq], cg, sg)
    sk = ko.rope(parts[:, :, Hq:Hq + Hkv], cg, sg)
    dead = ~live.view(B, 1, 1)
    q_ref = sq.ref[0].masked_fill(dead, 0.0)
    q_scale = sq.scale[0].masked_fill(dead, 0.0)
    specs = {"q": ko.Spec(q_ref, q_scale, ko.K_ROPE, True),
             "k": ko.Spec(sk.ref[0][live], sk.scale[0][live], ko.K_ROPE,
                          True)}
    return specs, live

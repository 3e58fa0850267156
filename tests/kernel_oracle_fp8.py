"""Inputs, fp64 reference and bounds for the FP8 (e4m3) KV cache, judged by
the ONE rule of ``kernel_oracle.py`` (imported, not changed).

A stored element means ``float(code) * scale``; the reference of the decode
is ``kernel_oracle.attention_decode`` over the exactly dequantized caches in
fp64, per sequence with its own length. ``k`` is counted from the chains of
``attn_decode_ragged_fp8_kernel`` as its header writes them down; nothing is
fitted to an output.
"""
from __future__ import annotations

import math

import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

NW = 4  # waves per block
F8 = torch.float8_e4m3fn


def k_decode_fp8(T: int, Tmax: int, num_splits: int, D: int) -> float:
    """As kernel_oracle_ragged.k_decode_ragged (same lane groups, same 4-key
    batches, same merges): n = ceil(min(chunk, T) / (NW*g)) keys per lane
    group at 3 roundings, 2 per merge level, the divide. A score is 8 fma,
    log2(lpr) adds, and TWO roundings instead of one: kscale * softmax_scale
    and its product with the sum. p * vscale is one rounding of every term of
    o: 0.5 unit of the scale, counted as 1. +4 as in attention_decode."""
    lpr = D // 8
    g = 64 // lpr
    chunk = ops.decode_ragged_chunk(Tmax, num_splits)
    n = math.ceil(min(chunk, max(T, 1)) / (NW * g))
    levels = int(math.log2(g)) + NW + (num_splits if num_splits > 1 else 0)
    depth = 3 * n + 2 * levels + 1
    return (2 * ko.kred(depth) + ko.kred(8 + int(math.log2(lpr)) + 2) + 1 + 4)


def fp8_inputs(B, Tmax, Hq, Hkv, D, lens, seed=0, poison=True):
    """q bf16; random codes (no NaN code in a live row); scales that are no
    powers of two; one planted dominant key per sequence at len_b // 2 on kv
    head 0; code 0x7F and a NaN scale in every row >= len_b."""
    g = torch.Generator().manual_seed(seed)
    q = ko.bf(B, Hq, D, seed=seed)
    codes = torch.randint(0, 256, (2, B, Tmax, Hkv, D), generator=g,
                          dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x3A
    ks = (0.5 + torch.rand(B, Tmax, Hkv, generator=g)) / 96
    vs = (0.5 + torch.rand(B, Tmax, Hkv, generator=g)) / 7
    kc, vc = codes[0].view(F8), codes[1].view(F8)
    for b, n in enumerate(lens):
        if n > 0:
            c, s = ops.quantize_rows_fp8(ko.q16(q[b, 0] * 2.0))
            kc.view(torch.uint8)[b, n // 2, 0] = c.view(torch.uint8)
            ks[b, n // 2, 0] = s
        if poison:
            kc.view(torch.uint8)[b, n:] = 0x7F
            vc.view(torch.uint8)[b, n:] = 0x7F
            ks[b, n:] = float("nan")
            vs[b, n:] = float("nan")
    return q, kc, vc, ks, vs


def decode_specs(q, kc, vc, ks, vs, lens, num_splits) -> dict:
    """One Spec per sequence, seq0..seq{B-1}, each over [1,Hq,D]."""
    B, Hq, D = q.shape
    Tmax = kc.shape[1]
    kd = kc.float().double() * ks.double().unsqueeze(-1)
    vd = vc.float().double() * vs.double().unsqueeze(-1)
    specs = {}
    for b in range(B):
        T = min(max(int(lens[b]), 0), Tmax)
        if T == 0:
            z = torch.zeros(1, Hq, D, dtype=torch.float64)
            specs[f"seq{b}"] = ko.Spec(z, z.clone(), 1, True)
            continue
        s = ko.attention_decode(q[b:b + 1], kd[b:b + 1], vd[b:b + 1], T)
        s.k = k_decode_fp8(T, Tmax, num_splits, D)
        specs[f"seq{b}"] = s
    return specs


def check_quantizer(x, codes, scale):
    """x [N,D] bf16 rows, codes [N,D] e4m3, scale [N] fp32. The scale lies
    within 2^-22 of amax/448; an element is off by at most half an e4m3 ulp
    (3 mantissa bits; subnormal step 2^-9) of the scaled value, widened by
    the two fp32 roundings of the scaling; a zero row is scale 0, codes 0."""
    x, s = ko.f64(x), ko.f64(scale)
    code_bytes = codes.cpu().view(torch.uint8)
    amax = x.abs().amax(-1)
    zero = amax == 0
    assert (s[zero] == 0).all() and (code_bytes[zero] == 0).all()
    want = amax / 448
    assert ((s >= want * (1 - 2.0 ** -22)) & (s <= want * (1 + 2.0 ** -22))).all()
    x, s = x[~zero], s[~zero].unsqueeze(-1)
    deq = codes.cpu().float().double()[~zero] * s
    bound = s * torch.clamp(2.0 ** -4 * x.abs() / s, min=2.0 ** -10) \
        * (1 + 2.0 ** -16)
    err = (deq - x).abs()
    print(f"QUANT rows={x.shape[0]} max err/bound={float((err / bound).max()):.3f}")
    assert (err <= bound).all()

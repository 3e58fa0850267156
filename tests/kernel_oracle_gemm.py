"""fp64 reference for the weight-gradient GEMM, judged by the ONE rule of
``kernel_oracle.py`` (imported, not changed).

    out[N,K] = (old if accumulate else 0) + dy[M,N]^T @ x[M,K]      (bf16 out)

    ref    old + dy^T x in float64, from the bf16 values the kernel reads
    scale  |old| + |dy|^T |x|: what the output is formed from
    k      kred(M + 1)

How k is counted. The bf16 products are exact in fp32 (8 x 8 significand
bits). wgrad_gemm_kernel sums one output's M products in a single fp32
chain: M/32 chained mfma_f32_16x16x32_bf16, each folding 32 products into
the running value, counted as the f32 MFMA is documented, one rounding per
product: M roundings. Adding the old value in fp32 is one more: M + 1.
There is no split over tokens, so no second chain. The library path
(torch.mm, any blocking) never has a longer chain than M, so the same k
serves it. Nothing here is fitted to a kernel's output.

``rounded_twice``: torch.mm followed by add_ rounds dy^T x to bf16 BEFORE
the old value is added, which the one-rounding rule does not allow for when
the sum cancels. For that path alone the worst-case half ulp of the bf16
intermediate, 2^-8 |dy^T x| (the rule's own bf16 term, applied to the
intermediate), is allowed per element on top, through ``Spec.tiny``.

The keyword flags build deliberately wrong references.
"""
from __future__ import annotations

import torch

import kernel_oracle as ko

TILE = 256     # output tile edge of wgrad_gemm_kernel
TOKENS = 64    # tokens per step


def wgrad_inputs(M, N, K, seed=0):
    """dy, x ~ N(0,1) and an old value of the size of the product's spread
    (sqrt(M)), all bf16 and all asymmetric."""
    dy = ko.bf(M, N, seed=seed)
    x = ko.bf(M, K, seed=seed + 1)
    old = ko.bf(N, K, scale=float(M) ** 0.5, seed=seed + 2)
    return dy, x, old


def wgrad(dy, x, old=None, *, drop_last_step=False, transposed=False,
          ignore_old=False, swap_blocks=False, rounded_twice=False) -> ko.Spec:
    """Spec of out[N,K]. old=None means accumulate=False."""
    dy, x = ko.f64(dy), ko.f64(x)
    M, N = dy.shape
    K = x.shape[1]
    if drop_last_step:
        dy, x = dy[:M - TOKENS], x[:M - TOKENS]
    g = dy.t() @ x
    s = dy.abs().t() @ x.abs()
    if transposed:
        # what a kernel with rows and columns of its tile exchanged writes
        g = (x.t() @ dy).contiguous().view(N, K) if N != K else g.t()
        g = g.contiguous()
    if swap_blocks:
        g = g.clone()
        if K >= 2 * TILE:
            g[:, :TILE], g[:, TILE:2 * TILE] = \
                g[:, TILE:2 * TILE].clone(), g[:, :TILE].clone()
        elif N >= 2 * TILE:
            g[:TILE], g[TILE:2 * TILE] = \
                g[TILE:2 * TILE].clone(), g[:TILE].clone()
        else:  # one tile: its two 128-column staging units
            h = TILE // 2
            g[:, :h], g[:, h:TILE] = g[:, h:TILE].clone(), g[:, :h].clone()
    ref, scale = g, s
    if old is not None:
        o = ko.f64(old)
        scale = scale + o.abs()
        if not ignore_old:
            ref = ref + o
    spec = ko.Spec(ref, scale, ko.kred(M + 1), True)
    if rounded_twice:
        spec.tiny = spec.tiny + ko.BF16_HALF_ULP * g.abs().reshape(-1)
    return spec

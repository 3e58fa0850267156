"""fp64 reference for the input-gradient GEMM, judged by the ONE rule of
``kernel_oracle.py`` (imported, not changed).

    dx[M,K] = dy[M,N] @ W[N,K]                                      (bf16 out)

    ref    dy W in float64, from the bf16 values the GEMM reads
    scale  |dy| |W|: what the output is formed from
    k      kred(N)

How k is counted. The bf16 products are exact in fp32 (8 x 8 significand
bits). One output sums N of them. A single fp32 chain, counted as the f32
MFMA is documented, makes one rounding per product folded in: N roundings.
Any blocking of the same sum makes no more: s partial chains hold N
products between them, the first product of a chain costs nothing to
"add", and joining the chains takes s - 1 adds, so at most N roundings in
all and a longest path below N. So kred(N) serves the library's NN call, its
TN call on a transposed copy of W, and a split-K variant of either. The
transposition itself moves bits and adds nothing. Nothing here is fitted to
a GEMM's output.

The keyword flags build deliberately wrong references.
"""
from __future__ import annotations

import kernel_oracle as ko

BLOCK = 64     # columns of dx exchanged by swap_blocks
DROP = 8       # rows of the contraction left out by drop_last_rows


def dgrad_inputs(M, N, K, seed=0):
    """dy, W ~ N(0,1), bf16, both asymmetric (W also where N == K)."""
    return ko.bf(M, N, seed=seed), ko.bf(N, K, seed=seed + 1)


def dgrad(dy, w, *, untransposed=False, drop_last_rows=False,
          swap_blocks=False) -> ko.Spec:
    """Spec of dx[M,K]."""
    dy, w = ko.f64(dy), ko.f64(w)
    N, K = w.shape
    s = dy.abs() @ w.abs()
    if untransposed:
        # what F.linear(dy, W) gives: the copy was never transposed
        assert N == K, "only a square W can be used untransposed"
        w = w.t()
    if drop_last_rows:
        dy, w = dy[:, :N - DROP], w[:N - DROP]
    g = dy @ w
    if swap_blocks:
        assert K >= 2 * BLOCK
        g = g.clone()
        g[:, :BLOCK], g[:, BLOCK:2 * BLOCK] = \
            g[:, BLOCK:2 * BLOCK].clone(), g[:, :BLOCK].clone()
    return ko.Spec(g, s, ko.kred(N), True)

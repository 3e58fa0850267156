"""ops.linear_w4 on the GPU against fp64 by the one rule of kernel_oracle.py.

k is counted from the chains linear_w4.hip's header writes down: one MFMA
chain over the split's products, at most 128 * ceil(steps / S) terms at one
rounding each (kred of that depth); one add per split in the combine
(kred(S) for S > 1). There is no scale unit: the block scale is folded into
the exact widening. Nothing is fitted to an output."""
import math

import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def k_w4(K, S):
    depth = 128 * math.ceil((K // 128) / S)
    return ko.kred(depth) + (ko.kred(S) if S > 1 else 0)


def w4_inputs(M, N, K, seed=0):
    """Codes over all 16 nibbles, scale bytes in 110..125."""
    g = torch.Generator().manual_seed(seed + 23)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(110, 126, (N, K // 32), generator=g,
                           dtype=torch.uint8)
    return ko.bf(M, K, seed=seed), codes, scales


def w4_spec(x, codes, scales, S):
    w = ops.dequant_mxfp4(codes, scales).double()
    return ko.Spec(ko.f64(x) @ w.T, ko.f64(x).abs() @ w.abs().T,
                   k_w4(x.shape[1], S), True)


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("N,K", [(16, 128), (80, 384), (272, 1408)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
def test_linear_w4_vs_fp64(M, N, K, S):
    x, codes, scales = w4_inputs(M, N, K)
    xd, cd, sd = x.to(DEV), codes.to(DEV), scales.to(DEV)
    y = ops.linear_w4(xd, cd, sd, num_splits=S)
    ko.check(f"linear_w4 M={M} N={N} K={K} S={S}", y,
             w4_spec(x, codes, scales, S))
    assert torch.equal(y, ops.linear_w4(xd, cd, sd, num_splits=S))
    if M == 5:  # a token's row does not depend on its batch slot
        assert torch.equal(ops.linear_w4(xd[:1], cd, sd, num_splits=S)[0], y[0])


@pytest.mark.parametrize("byte", [101, 134])
def test_code_table_and_k_order(byte):
    """One-hot rows pick single elements: the output is exactly the host
    dequantization at (n, 37 m mod 256), bitwise except -0 -> +0. Row n has
    nibble (n + k) % 16 at k: every code under every k residue, which pins the
    nibble order and the k map."""
    M, N, K = 64, 16, 256
    cols = (37 * torch.arange(M)) % K
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), cols] = 1.0
    nib = ((torch.arange(N)[:, None] + torch.arange(K)[None]) % 16).to(torch.uint8)
    codes = nib[:, 0::2] | (nib[:, 1::2] << 4)
    scales = torch.full((N, K // 32), byte, dtype=torch.uint8)
    scales[:, 1::2] += 3
    y = ops.linear_w4(x.to(DEV), codes.to(DEV), scales.to(DEV),
                      num_splits=1).cpu()
    want = ops.dequant_mxfp4(codes, scales)[:, cols].T.to(torch.bfloat16)
    assert torch.equal((y + 0.0).view(torch.int16), (want + 0.0).view(torch.int16))


@pytest.mark.parametrize("S", [1, 3])
def test_linear_w4_captures(S):
    x, codes, scales = w4_inputs(8, 80, 384, seed=1)
    xd, cd, sd = x.to(DEV), codes.to(DEV), scales.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.linear_w4(xd, cd, sd, num_splits=S)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.linear_w4(xd, cd, sd, num_splits=S)
    xd.copy_(ko.bf(8, 384, seed=2))
    want = ops.linear_w4(xd.clone(), cd, sd, num_splits=S)
    for _ in range(2):
        graph.replay()
        assert torch.equal(y, want)


def test_w4_dequant_bitwise():
    _, codes, scales = w4_inputs(1, 48, 384, seed=3)
    got = ops.w4_dequant(codes.to(DEV), scales.to(DEV)).cpu()
    want = ops.dequant_mxfp4(codes, scales).to(torch.bfloat16)
    assert torch.equal((got + 0.0).view(torch.int16),
                       (want + 0.0).view(torch.int16))


def test_prefill_rows_dequantize_and_contract_is_named():
    """M = 65 takes w4_dequant + the library GEMM: the same fp64 Spec, no
    extra rounding term, since the bf16 weight is exact."""
    x, codes, scales = w4_inputs(65, 80, 384, seed=4)
    xd, cd, sd = x.to(DEV), codes.to(DEV), scales.to(DEV)
    ko.check("linear_w4 M=65", ops.linear_w4(xd, cd, sd),
             w4_spec(x, codes, scales, 1))
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ops.linear_w4(xd[:4, :192].contiguous(), cd[:, :96].contiguous(),
                      sd[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.linear_w4(xd[:4], cd[:24], sd[:24])

"""ops.linear_w8 on the GPU against fp64 by the one rule of kernel_oracle.py.

k is counted from the chains linear_w8.hip's header writes down: one MFMA
chain over the split's products, at most 128 * ceil(steps / S) terms at one
rounding each (kred of that depth); the channel-scale multiply, applied before
the split fold (half a unit, counted as 1); one add per split in the combine
(kred(S) for S > 1). Nothing is fitted to an output."""
import math

import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
DEV = "cuda"


def k_w8(K, S):
    depth = 128 * math.ceil((K // 128) / S)
    return ko.kred(depth) + 1 + (ko.kred(S) if S > 1 else 0)


def w8_inputs(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed + 17)
    x = ko.bf(M, K, seed=seed)
    codes = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x3A
    return x, codes.view(F8), (0.5 + torch.rand(N, generator=g)) / 96


def w8_spec(x, codes, ws, S, weight=None):
    w = (codes.float().double() * ws.double()[:, None] if weight is None
         else ko.f64(weight))
    return ko.Spec(ko.f64(x) @ w.T, ko.f64(x).abs() @ w.abs().T,
                   k_w8(x.shape[1], S), True)


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("N,K", [(16, 128), (80, 384), (272, 1408)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
def test_linear_w8_vs_fp64(M, N, K, S):
    x, codes, ws = w8_inputs(M, N, K)
    xd, cd, wd = x.to(DEV), codes.to(DEV), ws.to(DEV)
    y = ops.linear_w8(xd, cd, wd, num_splits=S)
    ko.check(f"linear_w8 M={M} N={N} K={K} S={S}", y, w8_spec(x, codes, ws, S))
    assert torch.equal(y, ops.linear_w8(xd, cd, wd, num_splits=S))
    if M == 5:  # a token's row does not depend on its batch slot
        assert torch.equal(ops.linear_w8(xd[:1], cd, wd, num_splits=S)[0], y[0])


def test_code_table_and_k_order():
    """One-hot rows pick single codes: the output is exactly the decoded code
    at (n, 37 m mod 256), bitwise except -0 -> +0."""
    M, N, K = 64, 16, 256
    cols = (37 * torch.arange(M)) % K
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), cols] = 1.0
    codes = ((torch.arange(N)[:, None] * 67 + torch.arange(K)[None]) % 254)
    codes = codes + (codes >= 0x7F).long()           # skips 0x7F; 0xFF unreached
    assert not ((codes & 0x7F) == 0x7F).any() and codes.unique().numel() == 254
    codes = codes.to(torch.uint8).view(F8)
    y = ops.linear_w8(x.to(DEV), codes.to(DEV), torch.ones(N, device=DEV),
                      num_splits=1).cpu()
    want = codes.float()[:, cols].T.to(torch.bfloat16)       # [M, N], exact
    assert torch.equal((y + 0.0).view(torch.int16), (want + 0.0).view(torch.int16))


@pytest.mark.parametrize("S", [1, 3])
def test_linear_w8_captures(S):
    x, codes, ws = w8_inputs(8, 80, 384, seed=1)
    xd, cd, wd = x.to(DEV), codes.to(DEV), ws.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.linear_w8(xd, cd, wd, num_splits=S)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.linear_w8(xd, cd, wd, num_splits=S)
    xd.copy_(ko.bf(8, 384, seed=2))
    want = ops.linear_w8(xd.clone(), cd, wd, num_splits=S)
    for _ in range(2):
        graph.replay()
        assert torch.equal(y, want)


def test_w8_dequant_bitwise():
    _, codes, ws = w8_inputs(1, 48, 384, seed=3)
    got = ops.w8_dequant(codes.to(DEV), ws.to(DEV)).cpu()
    want = (codes.float() * ws[:, None]).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_prefill_rows_dequantize_and_contract_is_named():
    """M = 65 takes w8_dequant + the library GEMM: the same fp64 Spec over the
    bf16-rounded weight's own error, added through Spec.tiny as
    kernel_oracle_gemm.rounded_twice does (2^-8 of sum|x||w| per output)."""
    x, codes, ws = w8_inputs(65, 80, 384, seed=4)
    xd, cd, wd = x.to(DEV), codes.to(DEV), ws.to(DEV)
    spec = w8_spec(x, codes, ws, 1)
    spec.tiny = spec.tiny + ko.BF16_HALF_ULP * spec.scale.reshape(-1)
    ko.check("linear_w8 M=65", ops.linear_w8(xd, cd, wd), spec)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ops.linear_w8(xd[:4, :192].contiguous(), cd[:, :192].contiguous(), wd)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.linear_w8(xd[:4], cd[:24], wd[:24])

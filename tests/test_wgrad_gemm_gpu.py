"""wgrad_gemm_kernel against the fp64 reference of kernel_oracle_gemm, per
element, plus the contract of ops.wgrad_gemm_: fallback shapes, writes
confined to `out`, bitwise repeatability, graph capture."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_gemm as kg
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

# prologue only; one pass of the two-tile loop; odd tile counts, which end
# in the single-tile tail; longer even and odd runs for the drain
MS = (64, 128, 192, 256, 320, 448)
# one tile; fewer than 8 blocks; 9 blocks (XCD shares of unequal size);
# both rectangular orientations
NKS = ((256, 256), (512, 768), (768, 768), (2304, 256), (256, 2304))

_inputs = {}


@pytest.fixture(autouse=True)
def kernel_everywhere(monkeypatch):
    """These shapes are not in the dispatch table; run the kernel anyway."""
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")


def inputs(M, N, K):
    """(dy, x, old) on the GPU and the two Specs, computed once per shape."""
    key = (M, N, K)
    if key not in _inputs:
        dy, x, old = kg.wgrad_inputs(M, N, K, seed=M + N + 3 * K)
        _inputs[key] = (dy.cuda(), x.cuda(), old.cuda(),
                        kg.wgrad(dy, x), kg.wgrad(dy, x, old))
    return _inputs[key]


@pytest.mark.parametrize("NK", NKS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", MS)
def test_wgrad_matches_fp64(M, NK):
    N, K = NK
    dy, x, old, spec0, spec1 = inputs(M, N, K)
    assert ops.wgrad_fast_path(dy, x, old)
    out = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.wgrad_gemm_(dy, x, out, False)
    ko.check(f"wgrad[{M},{N},{K}].overwrite", out, spec0)
    out = old.clone()
    ops.wgrad_gemm_(dy, x, out, True)
    ko.check(f"wgrad[{M},{N},{K}].accumulate", out, spec1)


@pytest.mark.parametrize("group", (1, 3, 8))
def test_wgrad_rasters_agree(group):
    """Every raster visits every tile once: 9 x 3 tiles, bands of 1, 3 and 8
    slabs (8 leaves a short last band)."""
    M, N, K = 128, 2304, 768
    dy, x, old, _, spec1 = inputs(M, N, K)
    out = old.clone()
    ops.wgrad_gemm_(dy, x, out, True, group=group)
    ko.check(f"wgrad.group{group}", out, spec1)


def test_fallback_shape_equals_torch_bitwise():
    dy, x, old = (t.cuda() for t in kg.wgrad_inputs(100, 320, 256, seed=5))
    assert not ops.wgrad_fast_path(dy, x, old)
    out = old.clone()
    ops.wgrad_gemm_(dy, x, out, True)
    assert torch.equal(out, old + torch.mm(dy.t(), x))
    ops.wgrad_gemm_(dy, x, out, False)
    assert torch.equal(out, torch.mm(dy.t(), x))


def test_unlisted_shape_defaults_to_library(monkeypatch):
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip")
    dy, x, old, _, _ = inputs(128, 512, 768)
    assert ops.wgrad_fast_path(dy, x, old) and ops.wgrad_band(512, 768) is None
    out = old.clone()
    ops.wgrad_gemm_(dy, x, out, True)
    assert torch.equal(out, old + torch.mm(dy.t(), x))


def test_out_view_in_flat_buffer_keeps_neighbours():
    M, N, K = 192, 512, 768
    dy, x, old, _, spec1 = inputs(M, N, K)
    pad = 64    # elements: keeps the view 16-byte aligned
    flat = torch.full((pad + N * K + pad,), 7.0, dtype=torch.bfloat16,
                      device="cuda")
    view = flat[pad:pad + N * K].view(N, K)
    view.copy_(old)
    ops.wgrad_gemm_(dy, x, view, True)
    ko.check("wgrad.flat_view", view, spec1)
    assert bool((flat[:pad] == 7.0).all()) and bool((flat[-pad:] == 7.0).all())


def test_three_calls_bitwise_equal():
    M, N, K = 448, 768, 768
    dy, x, old, _, _ = inputs(M, N, K)
    outs = []
    for _ in range(3):
        out = old.clone()
        ops.wgrad_gemm_(dy, x, out, True)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_captured_call_follows_new_contents():
    M, N, K = 128, 512, 768
    dy, x, old, _, _ = inputs(M, N, K)
    dy2, x2, old2 = kg.wgrad_inputs(M, N, K, seed=99)
    sdy, sx, sout = dy.clone(), x.clone(), old.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.wgrad_gemm_(sdy, sx, sout, True)       # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.wgrad_gemm_(sdy, sx, sout, True)
    sdy.copy_(dy2.cuda())
    sx.copy_(x2.cuda())
    sout.copy_(old2.cuda())
    graph.replay()
    ko.check("wgrad.graph_replay", sout, kg.wgrad(dy2, x2, old2))

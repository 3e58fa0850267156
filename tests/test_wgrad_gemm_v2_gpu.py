"""The wgrad kernel's second schedule (variant 1: fragment reads under the
MFMAs, one barrier per phase) and its half blocks (`split`) against variant
0 with split 0, bit for bit: both keep every output element's fp32 chain.
The 9-tile grids are also held to the fp64 reference of kernel_oracle_gemm."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_gemm as kg
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

# prologue only; one pass of the two-tile loop; odd tile counts, which end in
# the single-tile tail; steady state (32 token tiles)
MS = (64, 128, 192, 256, 320, 448, 2048)
NKS = ((256, 256), (512, 768), (768, 768), (2304, 256), (256, 2304))
NINE = ((2304, 256), (256, 2304), (768, 768))     # 9 tiles each
BIG = (1024, 4352, 4096)     # 17 x 16 = 272 tiles: r = 16 on 256 units

_inputs = {}
_specs = {}
_base = {}


def inputs(M, N, K):
    """(dy, x, old) on the GPU, made once per shape."""
    key = (M, N, K)
    if key not in _inputs:
        if M * (N + K) > (1 << 23):       # large: drawn on the device
            gen = torch.Generator(device="cuda").manual_seed(M + N + 3 * K)
            dy, x, old = (
                (torch.randn(*s, device="cuda", generator=gen) * sc).bfloat16()
                for s, sc in (((M, N), 1.0), ((M, K), 1.0),
                              ((N, K), float(M) ** 0.5)))
            _inputs[key] = (dy, x, old)
        else:
            _inputs[key] = tuple(
                t.cuda() for t in kg.wgrad_inputs(M, N, K, seed=M + N + 3 * K))
    return _inputs[key]


def specs(M, N, K):
    key = (M, N, K)
    if key not in _specs:
        dy, x, old = (t.cpu() for t in inputs(M, N, K))
        _specs[key] = (kg.wgrad(dy, x), kg.wgrad(dy, x, old))
    return _specs[key]


def run(M, N, K, accumulate, variant, split, group=4):
    dy, x, old = inputs(M, N, K)
    out = old.clone() if accumulate else torch.full(
        (N, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.wgrad_gemm_(dy, x, out, accumulate, group=group, variant=variant,
                    split=split)
    return out


def base(M, N, K, accumulate):
    """Variant 0 without half blocks: the parent's kernel, launched once."""
    key = (M, N, K, accumulate)
    if key not in _base:
        _base[key] = run(M, N, K, accumulate, 0, 0)
    return _base[key]


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("NK", NKS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", MS)
def test_variant1_bitwise_equals_variant0(M, NK):
    N, K = NK
    for accumulate in (False, True):
        out = run(M, N, K, accumulate, 1, 0)
        assert same_bits(out, base(M, N, K, accumulate)), (M, N, K, accumulate)


@pytest.mark.parametrize("NK", NINE, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", MS)
def test_forced_split_bitwise_and_fp64(M, NK):
    """0, 1, 3 and all 9 tiles as half blocks (2, 6 and 18 halves: the paired
    run of 16 and the short last run), under both schedules of the full
    blocks."""
    N, K = NK
    for accumulate in (False, True):
        ref = base(M, N, K, accumulate)
        for variant in (0, 1):
            for split in (0, 1, 3, 9):
                out = run(M, N, K, accumulate, variant, split)
                assert same_bits(out, ref), (M, N, K, accumulate, variant,
                                             split)
                if M <= 448 and split in (3, 9) and variant == 1:
                    ko.check(f"wgrad[{M},{N},{K}].split{split}.acc"
                             f"{int(accumulate)}", out,
                             specs(M, N, K)[int(accumulate)])


def test_split_rasters_agree():
    """Half blocks find their tiles under every band height."""
    M, N, K = 128, 2304, 768      # 9 x 3 tiles
    ref = base(M, N, K, True)
    for group in (1, 3, 8):
        for split in (5, 27):
            assert same_bits(run(M, N, K, True, 1, split, group), ref)


def test_automatic_rule_above_the_cu_count():
    M, N, K = BIG
    cus = ops._C.wgrad_cus()
    assert ops._C.wgrad_split(N, K, cus) == ops.wgrad_split(N, K, cus)
    if cus == 256:
        assert ops.wgrad_split(N, K, cus) == 16
    for accumulate in (False, True):
        ref = base(M, N, K, accumulate)
        out = run(M, N, K, accumulate, None, None)      # the defaults
        assert bool(torch.isfinite(out).all())
        assert same_bits(out, ref)
        out = run(M, N, K, accumulate, 1, 16)       # r of 256 units, forced
        assert bool(torch.isfinite(out).all())
        assert same_bits(out, ref)


def test_env_variant_is_read_per_call(monkeypatch):
    M, N, K = 192, 768, 768
    ref = base(M, N, K, True)
    for v in ("0", "1"):
        monkeypatch.setenv("TOK_WGRAD_VARIANT", v)
        assert ops.wgrad_variant() == int(v)
        assert same_bits(run(M, N, K, True, None, None), ref)
    monkeypatch.setenv("TOK_WGRAD_VARIANT", "7")
    with pytest.raises(ValueError):
        run(M, N, K, True, None, None)


def test_bad_arguments_raise():
    dy, x, old = inputs(64, 256, 256)
    with pytest.raises(ValueError):
        ops.wgrad_gemm_(dy, x, old.clone(), True, group=4, split=2)
    with pytest.raises(ValueError):
        ops.wgrad_gemm_(dy, x, old.clone(), True, group=4, variant=2)


@pytest.mark.parametrize("shape", ((2048, 768, 768), (4096, 2304, 2304), BIG),
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("loaded", (False, True), ids=("alone", "copies"))
def test_thirty_launches_same_bits(shape, loaded):
    """Value screen of the counted waits: 30 launches of the default kernel
    (and of forced halves), alone and while a side stream streams copies of
    a 1 GiB buffer so that the DMAs land late; every output is variant 0's."""
    M, N, K = shape
    tiles = (N // 256) * (K // 256)
    ref = base(M, N, K, True)
    side = torch.cuda.Stream()
    if loaded:
        src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        side.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(30):
        if loaded:
            with torch.cuda.stream(side):
                dst.copy_(src)
        split = None if i % 2 == 0 else min(tiles, 16 + i)
        outs.append(run(M, N, K, True, None, split))
    torch.cuda.current_stream().wait_stream(side)
    bad = [i for i, o in enumerate(outs) if not same_bits(o, ref)]
    assert not bad, f"launches {bad} differ from variant 0"


def test_captured_split_call_follows_new_contents():
    M, N, K = 128, 768, 768
    dy, x, old = inputs(M, N, K)
    dy2, x2, old2 = kg.wgrad_inputs(M, N, K, seed=99)
    sdy, sx, sout = dy.clone(), x.clone(), old.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # warm-up outside capture
        ops.wgrad_gemm_(sdy, sx, sout, True, group=4, variant=1, split=None)
        ops.wgrad_gemm_(sdy, sx, sout, True, group=4, variant=1, split=3)
    torch.cuda.current_stream().wait_stream(side)
    sout.copy_(old)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        # the automatic rule asks for the device's unit count while capturing
        ops.wgrad_gemm_(sdy, sx, sout, True, group=4, variant=1, split=None)
        ops.wgrad_gemm_(sdy, sx, sout, True, group=4, variant=1, split=3)
    sdy.copy_(dy2.cuda())
    sx.copy_(x2.cuda())
    sout.copy_(old2.cuda())
    graph.replay()
    want = old2.cuda().clone()
    ops.wgrad_gemm_(dy2.cuda(), x2.cuda(), want, True, group=4, variant=0,
                    split=0)
    ops.wgrad_gemm_(dy2.cuda(), x2.cuda(), want, True, group=4, variant=0,
                    split=0)
    assert same_bits(sout, want)
    once = old2.cuda().clone()
    ops.wgrad_gemm_(dy2.cuda(), x2.cuda(), once, True, group=4, variant=1,
                    split=3)
    ko.check("wgrad.split.graph", once, kg.wgrad(dy2, x2, old2))

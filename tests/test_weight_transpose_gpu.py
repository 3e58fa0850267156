"""weight_transpose_kernel through ops.transpose_2d_: random 16-bit patterns
(NaN payloads, -0 and subnormals among them) compared as int16 against
src.t().contiguous(), writes confined to `out`, the contract's ValueErrors,
and graph capture."""
import pytest
import torch

from torch_on_k8s_amd import ops

# one element-vector; one exact tile; a non-square multiple of a tile;
# partial tiles in both directions; both rectangular orientations
SHAPES = ((8, 8), (64, 64), (64, 128), (72, 136), (200, 64), (320, 1000),
          (1000, 320))
SENTINEL = 0x5A5A
GUARD = 512      # elements on either side of `out`


def bits(R, C, seed=0, device="cuda"):
    """[R, C] bf16 whose bit patterns are uniform over all 65536."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-32768, 32768, (R, C), generator=g, dtype=torch.int16)
    return t.to(device).view(torch.bfloat16)


def i16(t):
    return t.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("RC", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bits_come_out_transposed_and_guards_stay(RC):
    R, C = RC
    src = bits(R, C, seed=R + 3 * C)
    src[0, 0] = -0.0
    i16(src)[-1, -1] = 0x7FA5                  # a NaN with a payload
    i16(src)[0, -1] = 0x0001                   # the smallest subnormal
    flat = torch.full((GUARD + R * C + GUARD,), SENTINEL, dtype=torch.int16,
                      device="cuda")
    out = flat[GUARD:GUARD + R * C].view(torch.bfloat16).view(C, R)
    keep = src.clone()
    assert ops.transpose_2d_(src, out) is out
    assert torch.equal(i16(out), i16(src).t().contiguous())
    assert torch.equal(i16(src), i16(keep))
    assert bool((flat[:GUARD] == SENTINEL).all())
    assert bool((flat[-GUARD:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("offset", (64, 8))
def test_views_into_one_flat_buffer(offset):
    """Source and destination are views of one allocation, `offset` elements
    in: 128-byte and bare 16-byte alignment."""
    R, C = 72, 136
    n = R * C
    flat = torch.full((offset + n + offset + n + offset,), SENTINEL,
                      dtype=torch.int16, device="cuda")
    a, b = offset, offset + n + offset
    src = flat[a:a + n].view(torch.bfloat16).view(R, C)
    out = flat[b:b + n].view(torch.bfloat16).view(C, R)
    src.copy_(bits(R, C, seed=offset))
    want = i16(src).t().contiguous()
    ops.transpose_2d_(src, out)
    assert torch.equal(i16(out), want)
    for lo, hi in ((0, a), (a + n, b), (b + n, b + n + offset)):
        assert bool((flat[lo:hi] == SENTINEL).all())


@pytest.mark.gpu
def test_contract_breaks_raise_value_error():
    src = bits(64, 128)
    out = torch.zeros(128, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):                 # wrong dtype
        ops.transpose_2d_(src.half(), out.half())
    with pytest.raises(ValueError):                 # non-contiguous input
        ops.transpose_2d_(bits(128, 64).t(), out)
    with pytest.raises(ValueError):                 # wrong output shape
        ops.transpose_2d_(src, torch.zeros_like(src))
    for R, C in ((64, 100), (60, 128)):             # not a multiple of 8
        with pytest.raises(ValueError):
            ops.transpose_2d_(bits(R, C), torch.zeros(
                C, R, dtype=torch.bfloat16, device="cuda"))
    n = 64 * 128
    flat = torch.zeros(2 * n + 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):                 # source off by one element
        ops.transpose_2d_(flat[1:1 + n].view(64, 128), out)
    with pytest.raises(ValueError):                 # destination off by one
        ops.transpose_2d_(src, flat[1:1 + n].view(128, 64))
    with pytest.raises(ValueError):                 # overlapping in and out
        ops.transpose_2d_(flat[:n].view(64, 128),
                          flat[n - 8:2 * n - 8].view(128, 64))
    with pytest.raises(ValueError):                 # the same storage
        ops.transpose_2d_(flat[:64 * 64].view(64, 64),
                          flat[:64 * 64].view(64, 64))
    assert bool((flat == 0).all()) and bool((out == 0).all())


@pytest.mark.gpu
def test_captured_calls_follow_new_source():
    R, C = 72, 136
    s1, s2 = bits(R, C, seed=1), bits(200, 64, seed=2)
    o1 = torch.zeros(C, R, dtype=torch.bfloat16, device="cuda")
    o2 = torch.zeros(64, 200, dtype=torch.bfloat16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.transpose_2d_(s1, o1)                   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.transpose_2d_(s1, o1)
        ops.transpose_2d_(s2, o2)
    s1.copy_(bits(R, C, seed=3))
    s2.copy_(bits(200, 64, seed=4))
    o1.zero_()
    o2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(i16(o1), i16(s1).t().contiguous())
    assert torch.equal(i16(o2), i16(s2).t().contiguous())


def test_cpu_fallback_moves_bits():
    src = bits(200, 64, seed=9, device="cpu")
    out = torch.zeros(64, 200, dtype=torch.bfloat16)
    ops.transpose_2d_(src, out)
    assert torch.equal(i16(out), i16(src).t().contiguous())
    with pytest.raises(ValueError):
        ops.transpose_2d_(src, torch.zeros(200, 64, dtype=torch.bfloat16))

"""attention_decode_ragged vs fp64: per-sequence lengths (full, 1, 0),
every GQA ratio the kernel is built for, both head dims, split counts that
leave chunks full, partial and empty, lengths on the chunk boundaries, NaN
in every cache row a sequence must not read, repeatability, and a captured
call that follows new lengths. Rule: kernel_oracle.py; references and k:
kernel_oracle_ragged.py."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ragged as kr
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(name, B, Tmax, Hq, Hkv, D, lens, num_splits, seed=0):
    q, kc, vc = kr.ragged_inputs(B, Tmax, Hq, Hkv, D, lens, seed=seed)
    S = num_splits if num_splits is not None else \
        ops.decode_ragged_splits(B, Hkv, Tmax)
    specs = kr.attention_decode_ragged(q, kc, vc, lens, S)
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = ops.attention_decode_ragged(q.to(DEV), kc.to(DEV), vc.to(DEV), lt,
                                      num_splits=num_splits)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    for b, n in enumerate(lens):
        if n == 0:
            assert (out[b] == 0).all()
    ko.check_all(name, kr.split_rows(out), specs)
    return out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
@pytest.mark.parametrize("num_splits", [1, 3, 8])
def test_ragged_lengths_vs_fp64(Hq, Hkv, D, num_splits):
    lens = [103, 1, 37, 0]
    q, kc, vc = kr.ragged_inputs(4, 103, Hq, Hkv, D, lens)
    spec0 = kr.attention_decode_ragged(q, kc, vc, lens, num_splits)["seq0"]
    # the planted key takes (nearly) all the weight in its heads
    assert (spec0.ref[0, 0] - vc[0, 103 // 2, 0].double()).abs().max() < 0.05
    run(f"ragged[{Hq}/{Hkv},D={D},S={num_splits}]", 4, 103, Hq, Hkv, D,
        lens, num_splits)


@pytest.mark.parametrize("D", [64, 128])
def test_lengths_on_chunk_boundaries(D):
    Tmax = 103
    c = ops.decode_ragged_chunk(Tmax, 3)
    assert 2 * c <= Tmax
    run(f"ragged_boundary[D={D},c={c}]", 4, Tmax, 8, 2, D,
        [c - 1, c, c + 1, 2 * c], 3)


@pytest.mark.parametrize("D", [64, 128])
def test_splits_wholly_beyond_every_length(D):
    run(f"ragged_short[D={D}]", 4, 103, 8, 2, D, [5, 1, 3, 0], 8)


def test_default_split_count_at_its_cap():
    assert ops.decode_ragged_splits(1, 1, 8200) > 1
    run("ragged_default[T=8200]", 1, 8200, 4, 1, 128, [8200], None)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 9, 100])
def test_equal_lengths(T, D):
    run(f"ragged_equal[T={T},D={D}]", 2, T + 7, 8, 2, D, [T, T], None)


def test_repeatable_and_capturable():
    B, Tmax, Hq, Hkv, D = 4, 103, 8, 2, 128
    q, kc, vc = kr.ragged_inputs(B, Tmax, Hq, Hkv, D, [Tmax] * B,
                                 nan_fill=False)
    qg, kg, vg = q.to(DEV), kc.to(DEV), vc.to(DEV)
    lens = torch.tensor([103, 1, 37, 0], dtype=torch.int32, device=DEV)
    for S in (1, 3):
        a = ops.attention_decode_ragged(qg, kg, vg, lens, num_splits=S)
        b = ops.attention_decode_ragged(qg, kg, vg, lens, num_splits=S)
        assert torch.equal(a, b)

        # capture with one set of lengths, replay with another
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attention_decode_ragged(qg, kg, vg, lens, num_splits=S)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = ops.attention_decode_ragged(qg, kg, vg, lens, num_splits=S)
        new = torch.tensor([2, 99, 0, 64], dtype=torch.int32, device=DEV)
        saved = lens.clone()
        lens.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want = ops.attention_decode_ragged(qg, kg, vg, new, num_splits=S)
        assert torch.equal(cap, want)
        assert not torch.equal(cap, a)
        lens.copy_(saved)


def test_unsupported_gqa_ratio_raises():
    q = torch.zeros(1, 3, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(1, 8, 1, 64, dtype=torch.bfloat16, device=DEV)
    lens = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
        ops.attention_decode_ragged(q, kc, kc.clone(), lens)

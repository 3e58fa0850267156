"""The sampler's fp64 reference (sampler_oracle.py) and the CPU path of
ops.sample_tokens against it: Philox known answers, every case of the grid
and the planted ones, and wrong references that must reject the tokens."""
import pytest
import torch

import sampler_oracle as so
from torch_on_k8s_amd import ops

# Random123 known answers: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert so.philox4x32_10(ctr, key) == want
    assert ops.philox4x32_10(ctr, key) == want


def test_uniform_words():
    # key = (low, high) of the seed, counter = (low, high, 0, 0)
    seed, ctr = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88
    w = so.philox4x32_10((0x243f6a88, 0x85a308d3, 0, 0),
                         (0xa4093822, 0x299f31d0))
    assert so.uniform(seed, ctr) == (w[0] >> 8) * 2.0 ** -24
    assert ops.sample_uniform(seed, ctr) == so.uniform(seed, ctr)
    assert 0.0 <= so.uniform(-1, -1) < 1.0   # int64 two's complement


def test_counted_budget():
    for V in so.VOCABS:
        k = so.k_sample(V)
        print(f"SAMPLER k_sample({V}) = {k}, k_top_p = {so.k_top_p(V)}")
        assert so.k_top_p(V) <= so.GAP * k


def run_cpu(c):
    return ops.sample_tokens(c["logits"], c["temperature"], c["top_k"],
                             c["top_p"], c["seed"], c["counter"],
                             u=c.get("u"))


@pytest.mark.parametrize("V", so.VOCABS)
def test_cpu_path_on_the_grid(V):
    for i, c in enumerate(so.grid_cases(V)):
        so.check(f"cpu.V{V}.case{i}", run_cpu(c), c["specs"])


@pytest.mark.parametrize("name", ["tie_at_k", "neg_inf", "neg_inf_tail", "tiny_T",
                                  "explicit_u"])
def test_cpu_path_on_planted_cases(name):
    c = so.planted_cases()[name]
    so.check(f"cpu.{name}", run_cpu(c), c["specs"])


def test_cpu_path_bad_inputs_stay_in_range():
    c = so.bad_input_case()
    tok = run_cpu(c)
    assert bool(((tok >= 0) & (tok < c["logits"].shape[1])).all()), tok


@pytest.mark.parametrize("wrong", [
    {"counter_shift": 1}, {"k_shift": 1}, {"cdf_desc": True}])
def test_wrong_references_reject(wrong):
    """u from counter + 1, top-k with k + 1, or the CDF in descending-logit
    order: each must reject tokens the right reference accepts."""
    n_rej = 0
    for V in (512, 1001):
        for c in so.grid_cases(V):
            tok = run_cpu(c)
            assert not so.rejected(tok, c["specs"])
            bad = so.specs(c["logits"], c["temperature"], c["top_k"],
                           c["top_p"], c["seed"], c["counter"], **wrong)
            n_rej += len(so.rejected(tok, bad))
    print(f"SAMPLER mutant {wrong}: rejected {n_rej} rows")
    assert n_rej >= 1

"""CPU checks of the input-gradient reference: the exact result rounded to
bf16 passes the rule, deliberately wrong references fail it, each on a shape
where it applies; plus the CPU side of ops.transpose_2d_ and ops.dgrad."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_dgrad as kd
from torch_on_k8s_amd import ops

# the shapes of tests/test_dgrad_wt_gpu.py
MNKS = ((128, 256, 192), (64, 72, 136), (192, 512, 64), (128, 256, 256))


@pytest.mark.parametrize("MNK", MNKS, ids=lambda s: "x".join(map(str, s)))
def test_rounded_exact_result_passes_and_mutants_fail(MNK):
    M, N, K = MNK
    dy, w = kd.dgrad_inputs(M, N, K, seed=M + N + 3 * K)
    spec = kd.dgrad(dy, w)
    good = spec.ref.to(torch.bfloat16)
    ko.check(f"dgrad[{M},{N},{K}].good", good, spec)
    # the last 8 rows of the contraction dropped: every shape
    bad = kd.dgrad(dy, w, drop_last_rows=True)
    assert ko.compare("drop_last_rows", good, bad).violations > 0
    if N == K:      # W used untransposed: square, asymmetric W
        assert not torch.equal(w, w.t())
        bad = kd.dgrad(dy, w, untransposed=True)
        assert ko.compare("untransposed", good, bad).violations > 0
    if K >= 2 * kd.BLOCK:   # two 64-column blocks of dx exchanged
        bad = kd.dgrad(dy, w, swap_blocks=True)
        assert ko.compare("swap_blocks", good, bad).violations > 0


def test_every_mutant_ran_on_some_shape():
    assert any(N == K for _, N, K in MNKS)
    assert any(K >= 2 * kd.BLOCK for _, _, K in MNKS)


def test_cpu_mm_passes():
    dy, w = kd.dgrad_inputs(64, 72, 136, seed=1)
    ko.check("dgrad.cpu_mm", ops.dgrad(dy, w), kd.dgrad(dy, w))


def _bits(R, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (R, C), generator=g,
                         dtype=torch.int16).view(torch.bfloat16)


def test_transpose_cpu_moves_bits():
    src = _bits(72, 136)
    out = torch.zeros(136, 72, dtype=torch.bfloat16)
    assert ops.transpose_2d_(src, out) is out
    assert torch.equal(out.view(torch.int16),
                       src.view(torch.int16).t().contiguous())


def test_transpose_cpu_rejects_contract_breaks():
    src = _bits(64, 128)
    out = torch.zeros(128, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):                 # dtype
        ops.transpose_2d_(src.float(), out.float())
    with pytest.raises(ValueError):                 # non-contiguous input
        ops.transpose_2d_(_bits(128, 64).t(), out)
    with pytest.raises(ValueError):                 # output shape
        ops.transpose_2d_(src, torch.zeros(64, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError):                 # not a multiple of 8
        ops.transpose_2d_(_bits(64, 100),
                          torch.zeros(100, 64, dtype=torch.bfloat16))
    flat = torch.zeros(2 * 64 * 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError):                 # overlap
        ops.transpose_2d_(flat[:64 * 128].view(64, 128),
                          flat[64:64 + 64 * 128].view(128, 64))


def test_dgrad_env_and_table(monkeypatch):
    """Only measured winners take the transposed path; wt_all and blas
    override; TOK_WGRAD_IMPL does not bear on it."""
    monkeypatch.delenv("TOK_DGRAD_IMPL", raising=False)
    assert ops.dgrad_impl() == "wt"
    assert not ops.dgrad_transposed(256, 192)       # unlisted
    for shape, on in ops._DGRAD_DISPATCH.items():
        assert isinstance(on, bool)
        assert ops.dgrad_transposed(*shape) is on
    monkeypatch.setenv("TOK_WGRAD_IMPL", "hip_all")
    assert not ops.dgrad_transposed(256, 192)
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt_all")
    assert ops.dgrad_transposed(256, 192)
    monkeypatch.setenv("TOK_DGRAD_IMPL", "blas")
    assert not any(ops.dgrad_transposed(*s) for s in ops._DGRAD_DISPATCH)
    monkeypatch.setenv("TOK_DGRAD_IMPL", "nope")
    with pytest.raises(ValueError):
        ops.dgrad_impl()


def test_cpu_linear_stays_on_mm(monkeypatch):
    """CPU tensors never take the transposed path, whatever the variable."""
    monkeypatch.setenv("TOK_DGRAD_IMPL", "wt_all")
    monkeypatch.delenv("TOK_WGRAD_IMPL", raising=False)
    seen = []
    monkeypatch.setattr(ops, "transpose_2d_",
                        lambda *a: seen.append(1))
    dy, w = kd.dgrad_inputs(16, 24, 40, seed=2)
    x = ko.bf(16, 40, seed=5).requires_grad_()
    ops.linear(x, w.requires_grad_()).backward(dy)
    assert not seen and torch.equal(x.grad, dy.mm(w.detach()))

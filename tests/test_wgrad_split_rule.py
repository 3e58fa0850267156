"""ops.wgrad_split: which trailing tiles of a weight-gradient output run as
half blocks. Pure arithmetic, no GPU."""
import pytest

from torch_on_k8s_amd import ops

FLAGSHIP = {                      # output [N, K] -> split at 256 units
    "gate_up": ((28672, 4096), 0),      # 1792 tiles, 7 rounds
    "down": ((4096, 14336), 128),       # 896 tiles, 3.5 rounds
    "qkv": ((6144, 4096), 128),         # 384 tiles, 1.5 rounds
    "o": ((4096, 4096), 0),             # 256 tiles, 1 round
    "lm_head": ((128256, 4096), 80),    # 8016 tiles, 31 rounds + 80
}


@pytest.mark.parametrize("name", FLAGSHIP)
def test_flagship_shapes_at_256_units(name):
    (N, K), want = FLAGSHIP[name]
    assert ops.wgrad_split(N, K, 256) == want


@pytest.mark.parametrize("cus", (1, 2, 7, 64, 104, 256, 304))
def test_rule_over_small_grids(cus):
    for tn in range(1, 40):
        for tk in (1, 2, 3, 16, 56):
            tiles = tn * tk
            split = ops.wgrad_split(256 * tn, 256 * tk, cus)
            r = tiles % cus
            assert 0 <= split <= tiles
            assert 2 * split <= cus
            if r == 0 or 2 * r > cus:
                assert split == 0
            else:
                assert split == r


def test_degenerate_arguments_give_no_split():
    assert ops.wgrad_split(0, 4096, 256) == 0
    assert ops.wgrad_split(4096, 4096, 0) == 0


def test_variant_env(monkeypatch):
    monkeypatch.delenv("TOK_WGRAD_VARIANT", raising=False)
    assert ops.wgrad_variant() == -1
    monkeypatch.setenv("TOK_WGRAD_VARIANT", "0")
    assert ops.wgrad_variant() == 0
    monkeypatch.setenv("TOK_WGRAD_VARIANT", "1")
    assert ops.wgrad_variant() == 1
    for bad in ("2", "fast"):
        monkeypatch.setenv("TOK_WGRAD_VARIANT", bad)
        with pytest.raises(ValueError):
            ops.wgrad_variant()

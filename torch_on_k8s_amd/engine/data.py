"""Token streams for training.

SyntheticTokens: there is no dataset/network access in the benchmark
environment; the headline metric (BASELINE.json) is defined on synthetic
data with random-init weights. Tokens are generated directly on the target
device (deterministic per rank+step), so the input pipeline costs ~0 and
never hides or inflates step time.

PackedTokenFile: a pre-tokenized corpus, documents packed end to end in one
flat file. With TrainerConfig.doc_eos_id the trainer derives the document
bounds of every batch from the EOS tokens (ops.doc_bounds).
"""
from __future__ import annotations

import numpy as np
import torch


class SyntheticTokens:
    def __init__(self, vocab_size: int, micro_batch: int, seq_len: int,
                 device: torch.device, rank: int = 0, seed: int = 1234):
        self.vocab_size = vocab_size
        self.micro_batch = micro_batch
        self.seq_len = seq_len
        self.device = device
        self.rank = rank
        self.seed = seed
        self._gen = torch.Generator(device=device)

    def batch(self, step: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Returns (input_ids, labels), each [B, S]."""
        self._gen.manual_seed(self.seed + 1000003 * self.rank + step)
        toks = torch.randint(
            0, self.vocab_size, (self.micro_batch, self.seq_len + 1),
            device=self.device, generator=self._gen)
        return toks[:, :-1].contiguous(), toks[:, 1:].contiguous()


class PackedTokenFile:
    """Flat little-endian token file (uint16 or uint32) read through a
    numpy memmap, cut into windows of seq_len + 1 tokens.

    batch(step) is a pure function of (step, rank, world), like
    SyntheticTokens.batch: global window (step * world + rank) * micro_batch
    + i goes to row i, visited in an order fixed by the seed (an affine map
    modulo the window count, so every window is visited once per epoch and
    no permutation array is held). Resume and elastic world changes need
    nothing beyond the step counter."""

    _DTYPES = {"uint16": "<u2", "uint32": "<u4"}

    def __init__(self, path: str, dtype: str, micro_batch: int, seq_len: int,
                 device: torch.device, rank: int = 0, world: int = 1,
                 seed: int = 1234):
        if dtype not in self._DTYPES:
            raise ValueError(
                f"data_dtype must be one of {sorted(self._DTYPES)}, "
                f"got {dtype!r}")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world {world}")
        self.tokens = np.memmap(path, dtype=self._DTYPES[dtype], mode="r")
        self.micro_batch = micro_batch
        self.seq_len = seq_len
        self.device = device
        self.rank = rank
        self.world = world
        self.window = seq_len + 1
        self.num_windows = len(self.tokens) // self.window
        if self.num_windows < 1:
            raise ValueError(
                f"{path}: {len(self.tokens)} tokens, one window needs "
                f"{self.window}")
        # window order: i -> (a * i + c) mod n with gcd(a, n) = 1
        rng = np.random.default_rng(seed)
        n = self.num_windows
        a = int(rng.integers(1, max(2, n)))
        while np.gcd(a, n) != 1:
            a += 1
        self._a, self._c = a % n if n > 1 else 0, int(rng.integers(0, n))

    def window_index(self, step: int, row: int) -> int:
        g = (step * self.world + self.rank) * self.micro_batch + row
        return (self._a * g + self._c) % self.num_windows

    def batch(self, step: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Returns (input_ids, labels), each [B, S] int64 on the device."""
        rows = np.empty((self.micro_batch, self.window), dtype=np.int64)
        for i in range(self.micro_batch):
            w = self.window_index(step, i) * self.window
            rows[i] = self.tokens[w:w + self.window]
        toks = torch.from_numpy(rows).to(self.device)
        return toks[:, :-1].contiguous(), toks[:, 1:].contiguous()

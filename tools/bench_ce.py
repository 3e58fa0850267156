#!/usr/bin/env python
"""Cross-entropy forward + backward at the flagship logits shape: the plain
pair (ce_fwd + ce_bwd, what the defaults of ops.cross_entropy run) against
the masked pair (ce_fwd_masked + ce_bwd_masked).

    plain     ce_fwd, ce_bwd                           every row counts
    valid     masked pair, every label valid           the same work, row-split
    half      masked pair, every second row ignored    half the reads
    inplace   masked pair, every label valid, the gradient over the logits

One process, interleaved rounds, device events; every arm is timed as a pair
and its forward and backward alone. The extension is called
directly, so no Python-side work is in the timing beyond the launches. The
in-place arm owns a second logits buffer (its logits are gradients after the
first call, which costs the same to process). Bytes: fwd reads the counted
rows once; bwd reads them again and writes every row.

    python tools/bench_ce.py [--rounds 3] [--iters 5] [--rows 32768]
                             [--vocab 128256]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_on_k8s_amd import ops  # noqa: E402


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--vocab", type=int, default=128256)
    args = ap.parse_args()
    N, V = args.rows, args.vocab
    dev = torch.device("cuda", 0)
    C = ops._require_ext("bench_ce")
    print(f"# {torch.cuda.get_device_name(0)} rows={N} vocab={V} "
          f"rounds={args.rounds} iters={args.iters}")
    gen = torch.Generator(device=dev).manual_seed(0)
    logits = torch.empty(N, V, device=dev, dtype=torch.bfloat16)
    for r0 in range(0, N, 2048):              # fill by slices: fp32 staging
        n = min(2048, N - r0)
        logits[r0:r0 + n] = (torch.randn(n, V, device=dev, generator=gen)
                             * 2.0).bfloat16()
    logits2 = logits.clone()
    labels = torch.randint(0, V, (N,), device=dev, generator=gen,
                           dtype=torch.int32)
    half = labels.clone()
    half[1::2] = -100
    gout = torch.ones((), device=dev)
    gscale = gout / N
    rowbytes = V * 2

    # arm -> (forward, backward given the forward's result, rows read)
    def fwd_plain():
        return C.ce_fwd(logits, labels)[1], gscale

    def bwd_plain(st):
        C.ce_bwd(logits, labels, st[0], st[1])

    def masked(lg, lab, out=None):
        def fwd():
            _, lse, inv, _ = C.ce_fwd_masked(lg, lab, 1e-4)
            return lse, inv

        def bwd(st):
            C.ce_bwd_masked(lg, lab, st[0], gout, st[1], 1e-4, out)
        return fwd, bwd

    arms = {"plain": (fwd_plain, bwd_plain, N),
            "valid": (*masked(logits, labels), N),
            "half": (*masked(logits, half), N - N // 2),
            "inplace": (*masked(logits2, labels, logits2), N)}
    peak, state = {}, {}
    for a, (fwd, bwd, _) in arms.items():     # warm-up, and peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        bwd(fwd())
        torch.cuda.synchronize()
        peak[a] = torch.cuda.max_memory_allocated() - base
        # for the backward timed alone; the in-place arm's logits are
        # gradients by now, so its forward result is taken again
        state[a] = fwd()
    ms = {(a, part): [] for a in arms for part in ("pair", "fwd", "bwd")}
    for _ in range(args.rounds):
        for a, (fwd, bwd, _) in arms.items():
            ms[a, "pair"].append(timed(lambda: bwd(fwd()), args.iters))
            ms[a, "fwd"].append(timed(fwd, args.iters))
            ms[a, "bwd"].append(timed(lambda: bwd(state[a]), args.iters))
    for (a, part), v in ms.items():
        counted = arms[a][2]
        nbytes = {"pair": 2 * counted + N, "fwd": counted,
                  "bwd": counted + N}[part] * rowbytes
        mem = (f"  peak above inputs {peak[a] / 2**30:6.2f} GiB"
               if part == "pair" else "")
        print(f"{a:8s} {part:4s} ms min={min(v):7.3f} max={max(v):7.3f}  "
              f"TB/s {nbytes / max(v) / 1e9:5.2f}-{nbytes / min(v) / 1e9:5.2f}"
              f"{mem}", flush=True)


if __name__ == "__main__":
    main()

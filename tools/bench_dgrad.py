#!/usr/bin/env python
"""Input-gradient GEMM dx = dy @ W on the flagship shapes: the library's NN
call against the TN call on a transposed weight copy, with and without the
transposition that makes the copy.

    (a) nn        dy.mm(W)                        what ops.dgrad does by default
    (b) tn        F.linear(dy, Wt), Wt pre-made   the GEMM alone
    (c) transpose ops._C.transpose_2d_(W, Wt)     the copy alone, W from HBM
    (d) wt+tn     (c) then (b), back to back      what the transposed path runs

One process, interleaved rounds, device events (a ranking needs all three).
Operands are randn scaled like gradients and weights: zero-filled operands
read 15-20 % high on an MFMA-dense kernel. (c) rotates over enough distinct
weights (more than twice the last-level cache in total) that every source
comes from HBM, as it does in a training step, where a whole forward and
backward lie between two uses of a weight. In (d) the GEMM reads the copy
that the transposition has just written, as in the step.

Dispatch rule for ops._DGRAD_DISPATCH: a shape goes to the transposed path
only where the slowest round of (d) beats the fastest round of (a).

    python tools/bench_dgrad.py [--rounds 3] [--iters 5] [--tokens 32768]
                                [--shapes gate_up,down,...]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_on_k8s_amd import ops  # noqa: E402

SHAPES = {                     # weight [N, K] of the flagship linears
    "gate_up": (28672, 4096),
    "down": (4096, 14336),
    "qkv": (6144, 4096),
    "o": (4096, 4096),
    "lm_head": (128256, 4096),
}
LLC_BYTES = 256 << 20
COPY_CEILING_TBS = 6.29        # measured device-to-device copy rate


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    M = args.tokens
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)} tokens={M} rounds={args.rounds} "
          f"iters={args.iters}")
    for name in args.shapes.split(","):
        N, K = SHAPES[name]
        gen = torch.Generator(device=dev).manual_seed(0)

        def rnd(*shape, scale):
            return (torch.randn(*shape, device=dev, generator=gen,
                                dtype=torch.float32) * scale).bfloat16()

        dy = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        for r0 in range(0, M, 4096):          # fill by slices: fp32 staging
            dy[r0:r0 + 4096] = rnd(min(4096, M - r0), N, scale=1e-3)
        wbytes = N * K * 2
        # more than two caches' worth of distinct sources, at least iters
        nw = max(args.iters, 2 * LLC_BYTES // wbytes + 1)
        nw = min(nw, max(2, (8 << 30) // wbytes))
        ws = [rnd(N, K, scale=0.02) for _ in range(nw)]
        wt = torch.empty(K, N, device=dev, dtype=torch.bfloat16)
        wt0 = ws[0].t().contiguous()
        flops = 2.0 * M * N * K

        def nn(i):
            dy.mm(ws[i % nw])

        def tn(i):
            F.linear(dy, wt0)

        def transpose(i):
            # the extension directly: no Python-side checks in the timing
            ops._C.transpose_2d_(ws[i % nw], wt)

        def wt_tn(i):
            ops._C.transpose_2d_(ws[i % nw], wt)
            F.linear(dy, wt)

        arms = {"nn": nn, "tn": tn, "transpose": transpose, "wt+tn": wt_tn}
        for fn in arms.values():              # warm-up: kernel selection
            fn(0)
        torch.cuda.synchronize()
        assert torch.equal(wt, wt0)
        ms = {a: [] for a in arms}
        for _ in range(args.rounds):
            for a, fn in arms.items():
                ms[a].append(timed(fn, args.iters))
        for a, v in ms.items():
            if a == "transpose":
                rate = (f"TB/s {2 * wbytes / max(v) / 1e9:6.2f}-"
                        f"{2 * wbytes / min(v) / 1e9:6.2f} of "
                        f"{COPY_CEILING_TBS} ({nw} sources, "
                        f"{nw * wbytes / 2**20:.0f} MB)")
            else:
                rate = (f"TF/s {flops / max(v) / 1e9:7.1f}-"
                        f"{flops / min(v) / 1e9:7.1f}")
            print(f"{name:8s} [{N}x{K}] {a:10s} ms min={min(v):7.3f} "
                  f"max={max(v):7.3f}  {rate}", flush=True)
        wins = max(ms["wt+tn"]) < min(ms["nn"])
        print(f"{name:8s} [{N}x{K}] verdict    "
              f"{'wt' if wins else 'nn'}: slowest wt+tn {max(ms['wt+tn']):.3f}"
              f" against fastest nn {min(ms['nn']):.3f} ms", flush=True)
        del dy, ws, wt, wt0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Weight-gradient GEMM: the library's NT call (+ the add_ autograd runs
after it) against wgrad_gemm_kernel, on the flagship shapes.

One process, interleaved rounds, device events (a ranking needs all three).
Operands are randn scaled like activations and gradients: zero-filled
operands read 15-20 % high on an MFMA-dense kernel. For reference the TN
(forward) and NN (dgrad) library calls of the same FLOPs are timed too.

Arms: hip_g<G> is the incumbent schedule (variant 0, no half blocks) at band
height G; v1_g<G> variant 1; v0s_g<G> and v1s_g<G> the same two with the
trailing tiles as half blocks by the rule of ops.wgrad_split (equal to the
arm without "s" where the rule gives 0).

    python tools/bench_wgrad.py [--rounds 3] [--iters 5] [--tokens 32768]
                                [--shapes gate_up,down,...] [--groups 1,4,8]
                                [--vgroups 4,8] [--no-blas]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_on_k8s_amd import ops  # noqa: E402

SHAPES = {                     # output [N, K] of the flagship wgrads
    "gate_up": (28672, 4096),
    "down": (4096, 14336),
    "qkv": (6144, 4096),
    "o": (4096, 4096),
    "lm_head": (128256, 4096),
}
LLC_BYTES = 256 << 20


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
    ap.add_argument("--groups", default="1,4,8")
    ap.add_argument("--vgroups", default="4,8",
                    help="band heights of the variant x split arms")
    ap.add_argument("--no-blas", action="store_true",
                    help="kernel arms only (counter runs)")
    args = ap.parse_args()
    M = args.tokens
    groups = [int(g) for g in args.groups.split(",")]
    vgroups = [int(g) for g in args.vgroups.split(",") if g]
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)} tokens={M} rounds={args.rounds} "
          f"iters={args.iters}")
    for name in args.shapes.split(","):
        N, K = SHAPES[name]
        # one operand set: the smallest working set here (o at 32768 tokens,
        # 570 MB) is over twice the last-level cache; rotate two sets only
        # for a run small enough to sit in it
        nset = 2 if (M * (N + K) + N * K) * 2 <= LLC_BYTES else 1
        gen = torch.Generator(device=dev).manual_seed(0)

        def rnd(*shape, scale):
            return (torch.randn(*shape, device=dev, generator=gen,
                                dtype=torch.float32) * scale).bfloat16()

        dys, xs, ws, gs = [], [], [], []
        for _ in range(nset):
            dys.append(torch.empty(M, N, device=dev, dtype=torch.bfloat16))
            for r0 in range(0, M, 4096):      # fill by slices: fp32 staging
                dys[-1][r0:r0 + 4096] = rnd(min(4096, M - r0), N, scale=1e-3)
            xs.append(rnd(M, K, scale=1.0))
            ws.append(rnd(N, K, scale=0.02))
            gs.append(torch.zeros(N, K, device=dev, dtype=torch.bfloat16))
        flops = 2.0 * M * N * K

        def lib_nt(i):
            s = i % nset
            gs[s].add_(torch.mm(dys[s].t(), xs[s]))

        def lib_nt_mm_only(i):
            s = i % nset
            torch.mm(dys[s].t(), xs[s])

        def lib_tn(i):
            s = i % nset
            torch.mm(xs[s], ws[s].t())

        def lib_nn(i):
            s = i % nset
            torch.mm(dys[s], ws[s])

        arms = {} if args.no_blas else {
            "blas_nt+add": lib_nt, "blas_nt": lib_nt_mm_only,
            "blas_tn": lib_tn, "blas_nn": lib_nn}

        def hip(g, variant, split):
            # the extension directly: ops.wgrad_gemm_ would apply the
            # dispatch table this tool exists to fill
            return lambda i: ops._C.wgrad_gemm_(
                dys[i % nset], xs[i % nset], gs[i % nset], True, g, variant,
                split)

        for g in groups:
            arms[f"hip_g{g}"] = hip(g, 0, 0)
        for g in vgroups:
            arms[f"v1_g{g}"] = hip(g, 1, 0)
            arms[f"v0s_g{g}"] = hip(g, 0, -1)
            arms[f"v1s_g{g}"] = hip(g, 1, -1)
        for fn in arms.values():              # warm-up: kernel selection
            fn(0)
        torch.cuda.synchronize()
        ms = {a: [] for a in arms}
        for _ in range(args.rounds):
            for a, fn in arms.items():
                ms[a].append(timed(fn, args.iters))
        for a, v in ms.items():
            print(f"{name:8s} [{N}x{K}] {a:12s} ms min={min(v):7.3f} "
                  f"max={max(v):7.3f}  TF/s {flops / max(v) / 1e9:7.1f}-"
                  f"{flops / min(v) / 1e9:7.1f}", flush=True)
        del dys, xs, ws, gs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

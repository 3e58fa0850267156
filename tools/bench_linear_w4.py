#!/usr/bin/env python3
"""MXFP4 weight-only linear microbenchmark (dev tool, not the driver contract).

Kernel level: for each projection of llama-1b and of the 8B shape, at
M = 1, 8, 32, 64, three arms: ``F.linear`` on the bf16 weight,
``ops.linear_w8`` on e4m3 weights and ``ops.linear_w4`` on MXFP4 weights, each
at its default split count. One process; every arm warmed, captured as a graph
of calls that rotate over enough separate weights that a launch cannot find
its weight in the 256 MB last-level cache (the count is sized for the smallest
arm, the fp4 one), and replayed alternately over the rounds; device events.
TB/s is the weight bytes an arm reads (2, 1 or 17/32 bytes per weight) over its
median time. "faster" / "slower" is printed only where the slowest round of
one arm beats the fastest of the other, against both other arms.
``--sweep`` runs every split count 1..16 of the fp4 arm instead, on the
llama-1b shapes at M = 8.

Model level: llama-1b ``generate_ragged`` (B=8, 128+128, graph on) with bf16,
fp8 and mxfp4 weights, interleaved rounds, tok/s.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_decode import COPY_CEILING_TBS, time_interleaved
from bench_linear_w8 import ROTATE_BYTES, SHAPES, projections

W4_BYTES = 0.5 + 1 / 32    # per weight: a nibble and 1/32 of a scale byte


def verdict(ts, other):
    return ("faster" if max(ts) < min(other) else
            "slower" if min(ts) > max(other) else "no claim")


def line(name, ts, nbytes, tail=""):
    med = statistics.median(ts)
    print(f"  {name:14s} {med * 1e6:8.1f} [{min(ts) * 1e6:8.1f}.."
          f"{max(ts) * 1e6:8.1f}] us {nbytes / med / 1e12:6.3f} TB/s{tail}",
          flush=True)


def kernel_level(args, ops, dev):
    print(f"# kernel level: us per call as median [min..max] over "
          f"{args.rounds} interleaved rounds; TB/s = weight bytes read / "
          f"median; copy ceiling {COPY_CEILING_TBS} TB/s")
    F = torch.nn.functional
    for model in (["llama-1b"] if args.sweep else args.models):
        for proj, N, K in projections(model):
            nbuf = max(2, min(128, int(-(-ROTATE_BYTES // (W4_BYTES * N * K)))))
            g = torch.Generator(device=dev).manual_seed(0)
            wb, w8, w4 = [], [], []
            for _ in range(nbuf):   # one bf16 weight at a time next to the rest
                w = torch.randn(N, K, device=dev, generator=g).bfloat16() * 0.02
                w8.append(ops.quantize_weight_fp8(w))
                w4.append(ops.quantize_weight_mxfp4(w))
                if len(wb) < 2 or len(wb) * 2 * N * K < ROTATE_BYTES:
                    wb.append(w)
            nb16, nb8 = len(wb), max(2, min(nbuf, -(-ROTATE_BYTES // (N * K))))
            for M in ([8] if args.sweep else args.M):
                x = torch.randn(M, K, device=dev, generator=g).bfloat16()
                S4, S8 = ops.linear_w4_splits(M, N, K), ops.linear_w8_splits(M, N, K)
                iters = int(max(20, min(400, 20e-3 / max(10e-6,
                                                         N * K / 3e12))))
                print(f"\n{model} {proj} N={N} K={K} M={M} weights={nbuf} "
                      f"iters={iters} default_splits fp4={S4} fp8={S8}")
                if args.sweep:
                    splits = [S for S in range(1, 17) if K // 128 >= S]
                    fns = [lambda i, S=S: ops.linear_w4(x, *w4[i % nbuf],
                                                        num_splits=S)
                           for S in splits]
                    times = time_interleaved(fns, nbuf, iters, args.rounds)
                    for S, ts in zip(splits, times):
                        line(f"fp4 S={S}", ts, W4_BYTES * N * K,
                             " <- default" if S == S4 else "")
                    continue
                fns = [lambda i: F.linear(x, wb[i % nb16]),
                       lambda i: ops.linear_w8(x, *w8[i % nb8]),
                       lambda i: ops.linear_w4(x, *w4[i % nbuf])]
                t16, t8, t4 = time_interleaved(fns, nbuf, iters, args.rounds)
                line("bf16 F.linear", t16, 2 * N * K)
                line(f"fp8 S={S8}", t8, N * K,
                     f"  vs bf16 {statistics.median(t8) / statistics.median(t16):.3f}: "
                     f"{verdict(t8, t16)}")
                line(f"fp4 S={S4}", t4, W4_BYTES * N * K,
                     f"  vs bf16 {statistics.median(t4) / statistics.median(t16):.3f}: "
                     f"{verdict(t4, t16)}; vs fp8 "
                     f"{statistics.median(t4) / statistics.median(t8):.3f}: "
                     f"{verdict(t4, t8)}")
            del wb, w8, w4
            torch.cuda.empty_cache()


def model_level(args, dev):
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-1b")
    model = LlamaModel(cfg).bfloat16().to(dev).eval()
    B, S0, N = 8, 128, 128
    ids = torch.randint(0, cfg.vocab_size, (B, S0),
                        generator=torch.Generator().manual_seed(1)).to(dev)
    prompts = [ids[b] for b in range(B)]
    runs = [("bf16 weights", {}), ("fp8 weights", {"weight_dtype": "fp8"}),
            ("mxfp4 weights", {"weight_dtype": "mxfp4"})]
    for _, kw in runs:
        model.generate_ragged(prompts, max_new_tokens=N, use_graph=True, **kw)
    times = [[] for _ in runs]
    for _ in range(args.rounds):
        for j, (_, kw) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate_ragged(prompts, max_new_tokens=N, use_graph=True,
                                  **kw)
            torch.cuda.synchronize()
            times[j].append(time.perf_counter() - t0)
    print(f"\n# model level: llama-1b B={B} prompt={S0} new={N} graph on; "
          f"whole call, {args.rounds} interleaved rounds, tok/s = B*new / wall")
    for j, ((name, _), ts) in enumerate(zip(runs, times)):
        rate = [B * N / t for t in ts]
        tail = "".join(f"  vs {runs[i][0]}: {verdict(ts, times[i])}"
                       for i in range(j))
        print(f"  {name:14s} {statistics.median(rate):8.0f} tok/s "
              f"[{min(rate):8.0f}..{max(rate):8.0f}]{tail}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(SHAPES))
    ap.add_argument("--M", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be >= 3: a figure needs its spread")
    if not torch.cuda.is_available():
        sys.exit("bench_linear_w4 needs a GPU: a CPU timing says nothing here")
    from torch_on_k8s_amd import ops
    dev = torch.device("cuda", 0)
    if not args.skip_kernel:
        kernel_level(args, ops, dev)
    if not args.skip_model and not args.sweep:
        model_level(args, dev)


if __name__ == "__main__":
    main()

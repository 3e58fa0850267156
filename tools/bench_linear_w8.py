#!/usr/bin/env python3
"""FP8 weight-only linear microbenchmark (dev tool, not the driver contract).

Kernel level: for each projection of llama-1b and of the 8B shape, at
M = 1, 8, 32, ``ops.linear_w8`` on e4m3 weights against ``F.linear`` on the
bf16 weight. One process; both arms warmed, captured as graphs of calls that
rotate over enough separate weights that a launch cannot find its weight in
the 256 MB last-level cache, and replayed alternately over the rounds; device
events. GB/s is the weight bytes an arm reads (N*K, or 2*N*K) over its median
time; the copy ceiling measured in this repository is 6.29 TB/s. "faster" is
printed only where the slowest round of one arm beats the fastest of the
other. ``--sweep`` adds every split count 1..16 for the fp8 arm.

Model level: llama-1b ``generate_ragged`` (B=8, 128+128, graph on) with and
without ``weight_dtype="fp8"``, interleaved rounds, tok/s and the share of
greedy tokens the two agree on.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_decode import COPY_CEILING_TBS, time_interleaved

ROTATE_BYTES = 1 << 30
SHAPES = {   # name -> (hidden, intermediate, vocab, (Hq + 2 Hkv) * D, Hq * D)
    "llama-1b": (2048, 5504, 32000, 4096, 2048),
    "llama3-8b": (4096, 14336, 128256, 6144, 4096),
}


def projections(name):
    h, i, v, qkv, o = SHAPES[name]
    return [("qkv_proj", qkv, h), ("o_proj", h, o), ("gate_up_proj", 2 * i, h),
            ("down_proj", h, i), ("lm_head", v, h)]


def kernel_level(args, ops, dev):
    print(f"# kernel level: us per call as median [min..max] over "
          f"{args.rounds} interleaved rounds; GB/s = weight bytes read / "
          f"median; copy ceiling {COPY_CEILING_TBS * 1e3:.0f} GB/s")
    for model in args.models:
        for proj, N, K in projections(model):
            nbuf = max(2, min(64, -(-ROTATE_BYTES // (2 * N * K))))
            g = torch.Generator(device=dev).manual_seed(0)
            wb = [torch.randn(N, K, device=dev, generator=g).bfloat16() * 0.02
                  for _ in range(nbuf)]
            wq = [ops.quantize_weight_fp8(w) for w in wb]
            for M in args.M:
                x = torch.randn(M, K, device=dev, generator=g).bfloat16()
                S0 = ops.linear_w8_splits(M, N, K)
                splits = sorted({S0} | (set(range(1, 17)) if args.sweep
                                        else set()))
                splits = [S for S in splits if S == 1 or K // 128 // S >= 1]
                names = ["bf16 F.linear"] + [f"fp8 S={S}" for S in splits]
                fns = [lambda i: torch.nn.functional.linear(x, wb[i % nbuf])]
                fns += [lambda i, S=S: ops.linear_w8(x, *wq[i % nbuf],
                                                     num_splits=S)
                        for S in splits]
                iters = int(max(20, min(400, 20e-3 / max(10e-6,
                                                         2 * N * K / 3e12))))
                times = time_interleaved(fns, nbuf, iters, args.rounds)
                diff = float((fns[1](0).float() - fns[0](0).float()).abs().max())
                print(f"\n{model} {proj} N={N} K={K} M={M} weights={nbuf} "
                      f"iters={iters} default_splits={S0} "
                      f"max|fp8-bf16|={diff:.3e}")
                t16 = times[0]
                for name, ts in zip(names, times):
                    nbytes = N * K * (2 if name.startswith("bf16") else 1)
                    gbs = nbytes / statistics.median(ts) / 1e9
                    tail = ""
                    if name.startswith("fp8"):
                        r = statistics.median(ts) / statistics.median(t16)
                        verdict = ("faster" if max(ts) < min(t16) else
                                   "slower" if min(ts) > max(t16) else
                                   "no claim")
                        tail = f"  ratio {r:.3f}: {verdict}"
                        if name == f"fp8 S={S0}":
                            tail += " <- default"
                    print(f"  {name:14s} {statistics.median(ts) * 1e6:8.1f} "
                          f"[{min(ts) * 1e6:8.1f}..{max(ts) * 1e6:8.1f}] us "
                          f"{gbs:7.0f} GB/s{tail}", flush=True)
            del wb, wq
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
            ("fp8 weights + fp8 KV", {"weight_dtype": "fp8",
                                      "kv_dtype": "fp8"})]
    outs = [model.generate_ragged(prompts, max_new_tokens=N, use_graph=True,
                                  **kw) for _, kw in runs]
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
    for (name, _), ts, out in zip(runs, times, outs):
        rate = [B * N / t for t in ts]
        same = sum(int((a[S0:] == b[S0:]).sum()) for a, b in zip(out, outs[0]))
        print(f"  {name:22s} {statistics.median(rate):8.0f} tok/s "
              f"[{min(rate):8.0f}..{max(rate):8.0f}]  greedy tokens equal to "
              f"bf16: {same}/{B * N}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(SHAPES))
    ap.add_argument("--M", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be >= 3: a figure needs its spread")
    if not torch.cuda.is_available():
        sys.exit("bench_linear_w8 needs a GPU: a CPU timing says nothing here")
    from torch_on_k8s_amd import ops
    dev = torch.device("cuda", 0)
    if not args.skip_kernel:
        kernel_level(args, ops, dev)
    if not args.skip_model:
        model_level(args, dev)


if __name__ == "__main__":
    main()

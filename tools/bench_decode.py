#!/usr/bin/env python3
"""Decode microbenchmark (dev tool, not the driver contract).

Kernel level (Hq=32, Hkv=8, D=128 by default): the older one-length
``attention_decode`` against ``attention_decode_ragged`` at every split
count, at equal lengths T and at lengths drawn uniformly from [T/8, T]
(new kernel only). Device-event timing of captured loops of calls; every
shape is warmed; the configurations alternate inside a round and the
rounds repeat, so each figure comes with its own round-to-round spread
(median [min..max]). The
calls rotate over enough separate caches that a launch cannot find its K/V
in the 256 MB last-level cache, as a decode step over many layers cannot.
TB/s is the bytes of the VALID K and V rows, each counted once, over time;
the copy ceiling measured in this repository is 6.29 TB/s.

Sampler level: ``sample_tokens`` against the torch composition it replaces
(scaled softmax, and with a filter sort, cumsum, mask; then multinomial) and
against ``argmax``, on bf16 logits [B, V], same captured-loop timing. The
calls rotate over 4 logits buffers, which stay in the last-level cache as
the rows the ``lm_head`` GEMM has just written do.

Model level (llama-1b, B=8, 128-token prompts, 128 new tokens, graph on):
``generate`` against ``generate_ragged`` at equal lengths,
``generate_ragged`` at prompt lengths 16..128, and sampling: captured
``generate_ragged`` sampled (T=0.8, top-k 50, top-p 0.95) against the eager
``generate(temperature=0.8)``.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

COPY_CEILING_TBS = 6.29
SPLITS = (1, 2, 4, 8, 16, 32)
ROTATE_BYTES = 1 << 30     # rotate over >= this much K+V, if it takes <= 256
MAX_BUFS = 256


def fmt(ts):
    """median [min..max] of per-call seconds, in microseconds."""
    return (f"{statistics.median(ts) * 1e6:9.1f} "
            f"[{min(ts) * 1e6:8.1f}..{max(ts) * 1e6:8.1f}]")


def capture_calls(fn, nbuf, iters):
    """A graph of `iters` calls that rotate over nbuf caches: decode runs
    from a captured step, and a replay keeps the host's launch cost out of
    a kernel that takes a few microseconds."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            fn(i % nbuf)
    return graph


def time_graph(graph, iters):
    """Seconds per call of one replay, by device events."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def kernel_level(args, ops, dev):
    Hq, Hkv, D = args.Hq, args.Hkv, args.D
    print(f"# kernel level: Hq={Hq} Hkv={Hkv} D={D}, us per call as "
          f"median [min..max] over {args.rounds} rounds; TB/s from the "
          f"median; copy ceiling {COPY_CEILING_TBS} TB/s")
    for B in args.B:
        for T in args.T:
            row_bytes = Hkv * D * 2 * 2                     # K + V, bf16
            one = B * T * row_bytes
            nbuf = max(1, min(MAX_BUFS, -(-ROTATE_BYTES // one)))
            g = torch.Generator(device=dev).manual_seed(0)
            q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev,
                            generator=g)
            kc = torch.randn(nbuf, B, T, Hkv, D, dtype=torch.bfloat16,
                             device=dev, generator=g)
            vc = torch.randn(nbuf, B, T, Hkv, D, dtype=torch.bfloat16,
                             device=dev, generator=g)
            eq = torch.full((B,), T, dtype=torch.int32, device=dev)
            rg = torch.randint(T // 8, T + 1, (B,),
                               generator=torch.Generator().manual_seed(B + T)
                               ).to(dev, torch.int32)
            default = ops.decode_ragged_splits(B, Hkv, T)
            # per-call cost sets the iteration count: ~25 ms per timing
            est = max(20e-6, one * 4 / 3e12)
            iters = int(max(10, min(400, 25e-3 / est)))

            cfgs = [("old", None, eq)]
            cfgs += [(f"new S={S}", S, eq) for S in SPLITS]
            cfgs += [(f"ragged S={S}", S, rg) for S in SPLITS]

            def call(S, lens):
                if S is None:
                    return lambda i: ops.attention_decode(q, kc[i], vc[i], T)
                return lambda i: ops.attention_decode_ragged(
                    q, kc[i], vc[i], lens, num_splits=S)

            fns = [call(S, lens) for _, S, lens in cfgs]
            for fn in fns:                                   # warm each
                for i in range(min(nbuf, 3)):
                    fn(i)
            torch.cuda.synchronize()
            graphs = [capture_calls(fn, nbuf, iters) for fn in fns]
            for gr in graphs:                                # warm replays
                gr.replay()
            torch.cuda.synchronize()
            times = [[] for _ in cfgs]
            for _ in range(args.rounds):
                for j, gr in enumerate(graphs):              # alternate
                    times[j].append(time_graph(gr, iters))
            del graphs

            ref = ops.attention_decode(q, kc[0], vc[0], T).float()
            diff = max(float((ops.attention_decode_ragged(
                q, kc[0], vc[0], eq, num_splits=S).float() - ref).abs().max())
                for S in SPLITS)
            print(f"\nB={B} T={T} caches={nbuf} iters={iters} "
                  f"default_splits={default} "
                  f"max|new-old|={diff:.2e} ragged_lens="
                  f"{int(rg.min())}..{int(rg.max())} (sum {int(rg.sum())})")
            for (name, S, lens), ts in zip(cfgs, times):
                valid = int(lens.sum()) * row_bytes
                tbs = valid / statistics.median(ts) / 1e12
                mark = " <- default" if S == default else ""
                print(f"  {name:13s} {fmt(ts)} us  {tbs:6.3f} TB/s{mark}",
                      flush=True)
            del kc, vc
            torch.cuda.empty_cache()


SAMPLER_VOCABS = (32000, 128256)
SAMPLER_MIXES = (("temperature", 0, 1.0), ("top-k 50", 50, 1.0),
                 ("top-p 0.9", 0, 0.9), ("top-k 50 + top-p 0.9", 50, 0.9))
SAMPLER_T = 0.8


def torch_sample(logits, T, k, p):
    """What one would write without the kernel. Plain temperature is what
    LlamaModel.generate does; a filter sorts once and cuts both ways."""
    probs = torch.softmax(logits.float() / T, dim=-1)
    if not k and p >= 1.0:
        return torch.multinomial(probs, 1)
    sp, si = torch.sort(probs, dim=-1, descending=True)
    if k:
        sp[:, k:] = 0.0
    if p < 1.0:
        cum = torch.cumsum(sp, dim=-1)
        sp = sp.masked_fill(cum - sp >= p * cum[:, -1:], 0.0)
    return si.gather(1, torch.multinomial(sp, 1))


def sampler_level(args, ops, dev):
    print(f"\n# sampler level: bf16 logits [B, V], T={SAMPLER_T}, us per "
          f"call as median [min..max] over {args.rounds} rounds; x = torch "
          f"composition / sample_tokens")
    nbuf, iters = 4, 100
    for V in SAMPLER_VOCABS:
        for B in args.B:
            g = torch.Generator(device=dev).manual_seed(0)
            logits = (4 * torch.randn(nbuf, B, V, device=dev, generator=g)
                      ).bfloat16()
            temp = torch.full((B,), SAMPLER_T, device=dev)
            seed = torch.arange(B, device=dev)
            ctr = torch.arange(B, device=dev, dtype=torch.int32)
            cfgs, fns = [("argmax", None)], [lambda i: logits[i].argmax(-1)]
            for name, k, p in SAMPLER_MIXES:
                kt = torch.full((B,), k, dtype=torch.int32, device=dev)
                pt = torch.full((B,), p, device=dev)
                cfgs.append((f"sample_tokens {name}", name))
                fns.append(lambda i, kt=kt, pt=pt: ops.sample_tokens(
                    logits[i], temp, kt, pt, seed, ctr))
                cfgs.append((f"torch {name}", name))
                fns.append(lambda i, k=k, p=p: torch_sample(
                    logits[i], SAMPLER_T, k, p))
            for fn in fns:
                for i in range(nbuf):
                    fn(i)
            torch.cuda.synchronize()
            graphs = [capture_calls(fn, nbuf, iters) for fn in fns]
            for gr in graphs:
                gr.replay()
            torch.cuda.synchronize()
            times = [[] for _ in cfgs]
            for _ in range(args.rounds):
                for j, gr in enumerate(graphs):
                    times[j].append(time_graph(gr, iters))
            del graphs
            print(f"\nB={B} V={V} buffers={nbuf} iters={iters}")
            med = {n: statistics.median(t) for (n, _), t in zip(cfgs, times)}
            for (name, mix), ts in zip(cfgs, times):
                tail = ""
                if name.startswith("torch"):
                    tail = f"  {med[name] / med['sample_tokens ' + mix]:5.1f}x"
                print(f"  {name:36s} {fmt(ts)} us{tail}", flush=True)


def model_level(args, dev):
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config(args.model)
    model = LlamaModel(cfg).bfloat16().to(dev).eval()
    B, S0, N = args.model_B, args.prompt_len, args.new_tokens
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, S0), generator=g).to(dev)
    lens = torch.randint(S0 // 8, S0 + 1, (B,), generator=g).tolist()
    equal = [ids[b] for b in range(B)]
    ragged = [ids[b, :lens[b]] for b in range(B)]

    runs = [
        ("generate (equal)", lambda: model.generate(
            ids, max_new_tokens=N, use_graph=True)),
        ("generate_ragged (equal)", lambda: model.generate_ragged(
            equal, max_new_tokens=N, use_graph=True)),
        (f"generate_ragged (lens {min(lens)}..{max(lens)})",
         lambda: model.generate_ragged(ragged, max_new_tokens=N,
                                       use_graph=True)),
        ("generate_ragged sampled (equal)", lambda: model.generate_ragged(
            equal, max_new_tokens=N, use_graph=True, temperature=0.8,
            top_k=50, top_p=0.95, seed=1)),
        ("generate_ragged T=0.8 only (equal)", lambda: model.generate_ragged(
            equal, max_new_tokens=N, use_graph=True, temperature=0.8,
            seed=1)),
        ("generate temperature=0.8 (eager)", lambda: model.generate(
            ids, max_new_tokens=N, temperature=0.8)),
    ]
    for _, fn in runs:        # warm: code objects, GEMM algorithm choice
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(args.rounds):
        for j, (_, fn) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[j].append(time.perf_counter() - t0)
    print(f"\n# model level: {args.model} B={B} prompt={S0} new={N} graph on;"
          f" whole call (prefill + capture + decode), {args.rounds} rounds,"
          f" tok/s = B*new / wall")
    for (name, _), ts in zip(runs, times):
        rate = [B * N / t for t in ts]
        print(f"  {name:36s} {statistics.median(rate):8.0f} tok/s "
              f"[{min(rate):8.0f}..{max(rate):8.0f}]  "
              f"{statistics.median(ts) * 1e3:7.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--T", type=int, nargs="+", default=[512, 4096, 32768])
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="llama-1b")
    ap.add_argument("--model-B", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-sampler", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be >= 3: a figure needs its spread")
    if not torch.cuda.is_available():
        sys.exit("bench_decode needs a GPU: a CPU timing says nothing here")
    from torch_on_k8s_amd import ops
    dev = torch.device("cuda", 0)
    if not args.skip_kernel:
        kernel_level(args, ops, dev)
    if not args.skip_sampler:
        sampler_level(args, ops, dev)
    if not args.skip_model:
        model_level(args, dev)


if __name__ == "__main__":
    main()

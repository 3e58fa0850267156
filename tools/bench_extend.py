#!/usr/bin/env python3
"""Chunked-prefill microbenchmark (dev tool, not the driver contract).

One process, device-event timing, the arms of a comparison alternate inside
a round and the rounds repeat: every figure is median [min..max] over the
rounds.

(a) ``attention_extend`` (B=4, Hq=32, Hkv=8, D=128) at Tq in {1, 8, 64, 256}
    new tokens over T in {512, 4096, 32768} cached keys, all sequences full.
    Next to it: Tq calls of ``attention_decode_ragged`` over the same cache
    (what Tq tokens cost one by one: the same K/V bytes Tq times), and
    ``ops.attention`` causal on a [B, Tq] rectangle with no prefix (equal
    query length, not equal keys: it cannot read a cache), where Tq >= 64.
(b) the split-count sweep of ``attention_extend`` at the same shapes.
(c) llama-1b, B=8, prompt lengths spread over 33..S0 for S0 in {256, 1024}:
    ``generate_ragged(max_new_tokens=1)`` wall time, padded prefill
    (prefill_chunk=None) against prefill_chunk in {128, 256, 512}.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torch_on_k8s_amd import ops

DEV = "cuda:0"
SPLITS = (1, 2, 4, 8, 16, 32)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def rounds(arms, iters, n_rounds):
    """arms: {name: fn}. Interleaved; returns {name: (median, min, max)} us."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(n_rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(x):
    return f"{x[0]:9.1f} [{x[1]:.1f}..{x[2]:.1f}]"


def kernel_level(args):
    B, Hq, Hkv, D = 4, 32, 8, 128
    for T in (512, 4096, 32768):
        kc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
        vc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
        lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
        for Tq in (1, 8, 64, 256):
            q = torch.randn(B, Tq, Hq, D, device=DEV).bfloat16()
            ql = torch.full((B,), Tq, dtype=torch.int32, device=DEV)
            dflt = ops.extend_splits(B, Hkv, Tq, Hq // Hkv, T)
            arms = {"extend": lambda: ops.attention_extend(q, kc, vc, lens, ql),
                    "decode_x1": lambda: ops.attention_decode_ragged(
                        q[:, 0], kc, vc, lens)}
            if Tq >= 64:
                kr, vr = kc[:, :Tq].contiguous(), vc[:, :Tq].contiguous()
                arms["attention_rect"] = (lambda kr=kr, vr=vr: ops.attention(
                    q, kr, vr, causal=True))
            for S in SPLITS:
                if S <= T // 64:
                    arms[f"extend_S{S}"] = (lambda S=S: ops.attention_extend(
                        q, kc, vc, lens, ql, num_splits=S))
            r = rounds(arms, args.iters, args.rounds)
            kv_gb = 2 * B * T * Hkv * D * 2 / 1e9
            print(f"EXTEND T={T} Tq={Tq} default_S={dflt}: "
                  f"extend {fmt(r['extend'])} us "
                  f"({kv_gb / r['extend'][0] * 1e3:.2f} TB/s of K+V once); "
                  f"decode x{Tq} {r['decode_x1'][0] * Tq:.1f} us"
                  + (f"; attention[B,{Tq}] {fmt(r['attention_rect'])} us"
                     if "attention_rect" in r else ""))
            print("  SWEEP " + "  ".join(
                f"S={S}:{r[f'extend_S{S}'][0]:.1f}" for S in SPLITS
                if f"extend_S{S}" in r))


def model_level(args):
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-1b")
    model = LlamaModel(cfg).bfloat16().to(DEV).eval()
    B = 8
    for S0 in (256, 1024):
        lens = [33 + (S0 - 33) * b // (B - 1) for b in range(B)]
        g = torch.Generator().manual_seed(1)
        prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g)
                   for n in lens]
        arms = {"padded": lambda: model.generate_ragged(
            prompts, max_new_tokens=1, use_graph=False)}
        for N in (128, 256, 512):
            arms[f"chunk{N}"] = (lambda N=N: model.generate_ragged(
                prompts, max_new_tokens=1, use_graph=False, prefill_chunk=N))
        r = rounds(arms, 1, args.rounds)
        print(f"PREFILL llama-1b B={B} lens={lens[0]}..{lens[-1]}: " +
              "  ".join(f"{k} {fmt(v)} us" for k, v in r.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    kernel_level(args)
    if not args.skip_model:
        model_level(args)


if __name__ == "__main__":
    main()

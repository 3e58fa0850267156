#!/usr/bin/env python3
"""Paged-KV microbenchmark (dev tool, not the driver contract).

One process, device-event timing, 3 interleaved rounds of 5 calls; every
figure is min..max ms over the rounds and TB/s of K+V read once (at the
slowest round). Hq=32, Hkv=8, D=128; B in {1, 8, 32}, T in {512, 4096, 32768},
equal lengths and ragged ones (T * (b + 1) / B).

(a) ``attention_paged`` at Tq = 1 against ``attention_decode_ragged``, and at
    Tq in {8, 64, 256} against ``attention_extend``; both comparison kernels
    run on a contiguous cache of the same content, the paged one on a
    shuffled page table.
(b) llama-1b, B=8, 128 + 128 tokens: ``generate_ragged`` tok/s, paged against
    unpaged, alternating.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torch_on_k8s_amd import ops

DEV = "cuda:0"
PG = ops.KV_PAGE


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                # ms per call


def rounds(arms, iters, n_rounds):
    """arms: {name: fn}. Interleaved; returns {name: (min, max)} ms."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(n_rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    return {k: (min(v), max(v)) for k, v in t.items()}


def kernel_level(args):
    Hq, Hkv, D = 32, 8, 128
    for B in (1, 8, 32):
        for T in (512, 4096, 32768):
            if B * T * Hkv * D * 2 * 2 > args.max_gib * 2 ** 30:
                continue
            NP = T // PG
            kc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
            vc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
            perm = torch.randperm(B * NP, device=DEV)
            tab = perm.view(B, NP).to(torch.int32)

            def pool(c):
                pages = c.view(B * NP, PG, Hkv, D).permute(0, 2, 1, 3)
                out = torch.empty_like(pages.contiguous())
                out[perm] = pages
                return out

            kp, vp = pool(kc), pool(vc)
            for name, ln in (("equal", [T] * B),
                             ("ragged", [T * (b + 1) // B for b in range(B)])):
                lens = torch.tensor(ln, dtype=torch.int32, device=DEV)
                gb = 2 * sum(ln) * Hkv * D * 2 / 1e9
                for Tq in (1, 8, 64, 256):
                    q = torch.randn(B, Tq, Hq, D, device=DEV).bfloat16()
                    ql = torch.full((B,), Tq, dtype=torch.int32, device=DEV)
                    arms = {"paged": lambda: ops.attention_paged(
                        q, kp, vp, tab, lens, ql)}
                    if Tq == 1:
                        arms["decode_ragged"] = \
                            lambda: ops.attention_decode_ragged(
                                q[:, 0], kc, vc, lens)
                    else:
                        arms["extend"] = lambda: ops.attention_extend(
                            q, kc, vc, lens, ql)
                    r = rounds(arms, args.iters, args.rounds)
                    print(f"PAGED B={B} T={T} {name} Tq={Tq}: " + "  ".join(
                        f"{k} {v[0]:.4f}..{v[1]:.4f} ms "
                        f"({gb / v[1]:.2f} TB/s)" for k, v in r.items()),
                        flush=True)
            del kc, vc, kp, vp


def model_level(args):
    import time
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-1b")
    model = LlamaModel(cfg).bfloat16().to(DEV).eval()
    B, S0, N = 8, 128, 128
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (S0,), generator=g)
               for _ in range(B)]
    rates = {"unpaged": [], "paged": []}
    for i in range(args.rounds + 1):
        for k, extra in (("unpaged", {}), ("paged", {"kv_page_size": PG})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate_ragged(prompts, max_new_tokens=N, **extra)
            torch.cuda.synchronize()
            if i:                                   # round 0 warms up
                rates[k].append(B * N / (time.perf_counter() - t0))
    print("GENERATE llama-1b B=8 128+128: " + "  ".join(
        f"{k} {min(v):.0f}..{max(v):.0f} tok/s" for k, v in rates.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-gib", type=float, default=40.0)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    kernel_level(args)
    if not args.skip_model:
        model_level(args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""FP8 paged-KV microbenchmark (dev tool, not the driver contract).

One process, device-event timing, 3 interleaved rounds of 5 calls; every
figure is min..max ms over the rounds and TB/s of the K+V bytes that arm reads
once (at the slowest round): (D + 4) bytes per row for the e4m3 arms, 2 D for
bf16. Hq=32, Hkv=8, D=128; B in {1, 8, 32}, T in {512, 4096, 32768}, equal
lengths and ragged ones (T * (b + 1) / B), Tq in {1, 8, 64, 256}.

(a) ``attention_paged`` over e4m3 pools against ``attention_paged`` over bf16
    pools of the same content and page table, and at Tq = 1 against
    ``attention_decode_ragged`` over the e4m3 rectangle of the same codes.
(b) llama-1b, B=8, 128 + 128 tokens: ``generate_ragged`` tok/s,
    kv_dtype="fp8_paged" against kv_dtype="fp8" and kv_page_size=64,
    alternating.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from bench_paged import DEV, PG, rounds
from torch_on_k8s_amd import ops

F8 = torch.float8_e4m3fn


def kernel_level(args):
    Hq, Hkv, D = 32, 8, 128
    for B in (1, 8, 32):
        for T in (512, 4096, 32768):
            if B * T * Hkv * D * 2 * 2 > args.max_gib * 2 ** 30:
                continue
            NP = T // PG
            kc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
            vc = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
            k8, v8 = (torch.empty(B, T, Hkv, D, dtype=torch.uint8,
                                  device=DEV).view(F8) for _ in range(2))
            ks, vs = (torch.empty(B, T, Hkv, device=DEV) for _ in range(2))
            i32 = dict(dtype=torch.int32, device=DEV)
            ops.kv_quantize_append_(kc, vc, torch.zeros(B, **i32),
                                    torch.full((B,), T, **i32), k8, v8, ks, vs)
            perm = torch.randperm(B * NP, device=DEV)
            tab = perm.view(B, NP).to(torch.int32)

            def pool(c):
                """[B, T, Hkv, ...] -> [P, Hkv, 64, ...] under the table"""
                pages = c.reshape(B * NP, PG, Hkv, -1).permute(0, 2, 1, 3)
                out = torch.empty_like(pages.contiguous())
                out[perm] = pages
                return out

            kp, vp = pool(kc), pool(vc)
            kp8, vp8 = (pool(c.view(torch.uint8)).view(F8) for c in (k8, v8))
            ksp, vsp = pool(ks).squeeze(-1), pool(vs).squeeze(-1)
            for name, ln in (("equal", [T] * B),
                             ("ragged", [T * (b + 1) // B for b in range(B)])):
                lens = torch.tensor(ln, **i32)
                rows = 2 * sum(ln) * Hkv / 1e9
                gb = {"paged_fp8": rows * (D + 4), "paged_bf16": rows * 2 * D,
                      "decode_fp8": rows * (D + 4)}
                for Tq in (1, 8, 64, 256):
                    q = torch.randn(B, Tq, Hq, D, device=DEV).bfloat16()
                    ql = torch.full((B,), Tq, **i32)
                    arms = {"paged_fp8": lambda: ops.attention_paged(
                                q, kp8, vp8, tab, lens, ql, kscale=ksp,
                                vscale=vsp),
                            "paged_bf16": lambda: ops.attention_paged(
                                q, kp, vp, tab, lens, ql)}
                    if Tq == 1:
                        arms["decode_fp8"] = \
                            lambda: ops.attention_decode_ragged(
                                q[:, 0], k8, v8, lens, kscale=ks, vscale=vs)
                    r = rounds(arms, args.iters, args.rounds)
                    print(f"PAGED_FP8 B={B} T={T} {name} Tq={Tq}: " + "  ".join(
                        f"{k} {v[0]:.4f}..{v[1]:.4f} ms "
                        f"({gb[k] / v[1]:.2f} TB/s)" for k, v in r.items()),
                        flush=True)
            del kc, vc, kp, vp, k8, v8, kp8, vp8, ks, vs, ksp, vsp


def model_level(args):
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-1b")
    model = LlamaModel(cfg).bfloat16().to(DEV).eval()
    B, S0, N = 8, 128, 128
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (S0,), generator=g)
               for _ in range(B)]
    arms = (("fp8_paged", {"kv_dtype": "fp8_paged"}),
            ("fp8", {"kv_dtype": "fp8"}), ("paged", {"kv_page_size": PG}))
    rates = {k: [] for k, _ in arms}
    for i in range(args.rounds + 1):
        for k, extra in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate_ragged(prompts, max_new_tokens=N, **extra)
            torch.cuda.synchronize()
            if i:                                   # round 0 warms up
                rates[k].append(B * N / (time.perf_counter() - t0))
    print("GENERATE llama-1b B=8 128+128: " + "  ".join(
        f"{k} {min(v):.0f}..{max(v):.0f} tok/s" for k, v in rates.items()))
    for k in (None, "fp8_paged"):
        print(f"KV bytes/token {k}: "
              f"{ops.kv_cache_bytes_per_token(cfg.num_kv_heads, cfg.head_dim, cfg.num_layers, k)}")


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

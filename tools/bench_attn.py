#!/usr/bin/env python3
"""Attention kernel microbenchmark (dev tool, not the driver contract).

Measures fwd / bwd wall time and effective TFLOP/s of the gfx950 flash
attention at the flagship shape, A/B against torch SDPA. The forward is
timed both ways, v4 (default) and the older v3, and so is the backward,
fused dK+dV (default) and split dV / dK, side by side; the fused backward
is also timed with each dQ kernel (dq_variant 1 = 8-wave kernel in
XCD-aware block order, the default; 0 = 4-wave kernel; 2 = 8-wave kernel in
plain block order): the calls differ only in the dQ kernel, so the
difference of their times is the difference of the dQ kernels.
Within-process interleaved rounds (guide §5.4 rule 24). The flagship
per-layer shape is --B 8; record runs at both --B 2 and --B 8.

--doc-len L[,L...] times packed-document attention instead: documents of L
tokens packed into every row, the last one short. One process, interleaved
rounds of (a) the plain causal call, (b) bounds that describe one document
per row, and one column per L; forward, and forward plus backward. The
yardstick printed next to the times is the live-tile ratio counted from the
layout: the share of the causal row's 32x32 (query, key) blocks that still
hold a visible pair.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def flops(B, S, Hq, D, causal, bwd=False):
    f = 4 * B * Hq * S * S * D
    if causal:
        f //= 2
    return f * (2.5 if bwd else 1.0)


def time_fn(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def doc_layout(S, L):
    """doc_start, doc_end (int32 [S]) of documents of L tokens, last short."""
    idx = torch.arange(S, dtype=torch.int32)
    ds = idx // L * L
    return ds, torch.clamp(ds + L, max=S)


def live_ratio(S, ds):
    """Share of the causal 32x32 blocks that hold a pair with
    doc_start[i] <= j <= i."""
    n = (S + 31) // 32
    blk = torch.arange(n)
    first_row = blk * 32
    last_row = torch.clamp(first_row + 31, max=S - 1)
    # doc_start is non-decreasing: a block row's smallest bound is its first
    # row's, and key block c is live iff it ends past that bound
    lo = ds[first_row].long().view(n, 1)
    live = (blk.view(1, n) * 32 <= last_row.view(n, 1)) & \
        (blk.view(1, n) * 32 + 31 >= lo)
    return float(live.sum()) / (n * (n + 1) // 2)


def bench_docs(args, ops, q, k, v, do):
    B, S = q.shape[:2]
    dev = q.device
    cols = [("plain", None)]
    for L in [S] + [int(x) for x in args.doc_len.split(",")]:
        ds, de = doc_layout(S, L)
        name = "one-doc" if L == S else f"doc-len {L}"
        cols.append((name, (ds, de)))
    fns, ratios = [], []
    for name, bd in cols:
        if bd is None:
            ratios.append(1.0)
            fwd = lambda: ops._C.attn_fwd(q, k, v, True)
            o, lse = fwd()
            bwd = lambda o=o, lse=lse: ops._C.attn_bwd(q, k, v, o, lse, do,
                                                       True)
        else:
            ratios.append(live_ratio(S, bd[0]))
            ds = bd[0].to(dev).unsqueeze(0).expand(B, S).contiguous()
            de = bd[1].to(dev).unsqueeze(0).expand(B, S).contiguous()
            fwd = lambda ds=ds: ops._C.attn_fwd(q, k, v, True, 0, ds)
            o, lse = fwd()
            bwd = lambda o=o, lse=lse, ds=ds, de=de: ops._C.attn_bwd(
                q, k, v, o, lse, do, True, False, 1, ds, de)
        fns.append((fwd, bwd, o, lse))
    o0, lse0 = fns[0][2], fns[0][3]
    print(f"one-doc bounds vs plain: O bitwise {torch.equal(o0, fns[1][2])}, "
          f"LSE bitwise {torch.equal(lse0, fns[1][3])}, dQ/dK/dV bitwise "
          f"{all(torch.equal(a, b) for a, b in zip(fns[0][1](), fns[1][1]()))}")
    for r in range(args.rounds):
        tf = [time_fn(f[0], args.iters) for f in fns]
        tb = [time_fn(f[1], args.iters) for f in fns]
        for (name, _), ratio, a, b in zip(cols, ratios, tf, tb):
            print(f"[round {r}] {name:>12}: fwd {a*1e3:7.3f} ms "
                  f"(x{a/tf[0]:.3f}) | fwd+bwd {(a+b)*1e3:7.3f} ms "
                  f"(x{(a+b)/(tf[0]+tb[0]):.3f}) | live tiles x{ratio:.3f}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--Hq", type=int, default=32)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dq-variants", default="1,0,2",
                    help="dQ kernels to time in the fused backward")
    ap.add_argument("--no-sdpa", action="store_true",
                    help="skip the torch SDPA columns (saves time at B=8)")
    ap.add_argument("--doc-len", default=None,
                    help="packed documents of this many tokens (comma list):"
                    " time plain / one document / each length and stop")
    args = ap.parse_args()
    from torch_on_k8s_amd import ops

    B, S, Hq, Hkv, D = args.B, args.S, args.Hq, args.Hkv, args.D
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    q = torch.randn(B, S, Hq, D, dtype=torch.bfloat16, device=dev)
    k = torch.randn(B, S, Hkv, D, dtype=torch.bfloat16, device=dev)
    v = torch.randn(B, S, Hkv, D, dtype=torch.bfloat16, device=dev)
    do = torch.randn(B, S, Hq, D, dtype=torch.bfloat16, device=dev)
    if args.doc_len:
        bench_docs(args, ops, q, k, v, do)
        return
    rep = Hq // Hkv
    qt = q.transpose(1, 2).contiguous()
    kt = k.transpose(1, 2).repeat_interleave(rep, dim=1).contiguous()
    vt = v.transpose(1, 2).repeat_interleave(rep, dim=1).contiguous()
    dot = do.transpose(1, 2).contiguous()

    ffw = flops(B, S, Hq, D, True)
    fbw = flops(B, S, Hq, D, True, bwd=True)

    def hip_fwd():
        o, lse = ops._C.attn_fwd(q, k, v, True)
        return o, lse

    def hip_fwd_v3():   # older forward kernel (variant 1)
        return ops._C.attn_fwd(q, k, v, True, 1)

    o_, lse_ = hip_fwd()

    def hip_bwd():      # fused dK+dV kernel (the default path)
        return ops._C.attn_bwd(q, k, v, o_, lse_, do, True, False)

    def hip_bwd_split():   # older split dV / dK kernels
        return ops._C.attn_bwd(q, k, v, o_, lse_, do, True, True)

    dq_variants = [int(x) for x in args.dq_variants.split(",")]

    def hip_bwd_dq(variant):   # fused dK+dV with the given dQ kernel
        return lambda: ops._C.attn_bwd(q, k, v, o_, lse_, do, True, False,
                                       variant)

    qs = qt.detach().requires_grad_(True)
    ks = kt.detach().requires_grad_(True)
    vs = vt.detach().requires_grad_(True)

    def sdpa_fwd():
        return torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, is_causal=True)

    def sdpa_fwdbwd():
        o = torch.nn.functional.scaled_dot_product_attention(
            qs, ks, vs, is_causal=True)
        o.backward(dot)
        qs.grad = ks.grad = vs.grad = None

    for r in range(args.rounds):
        th_f = time_fn(hip_fwd, args.iters)
        th_f3 = time_fn(hip_fwd_v3, args.iters)
        th_b = time_fn(hip_bwd, args.iters)
        th_bs = time_fn(hip_bwd_split, args.iters)
        th_dq = [time_fn(hip_bwd_dq(x), args.iters) for x in dq_variants]
        print(f"[round {r}] hip bwd fused by dq_variant: " + " | ".join(
            f"{x}: {t*1e3:7.3f} ms {fbw/t/1e12:6.1f} TF"
            for x, t in zip(dq_variants, th_dq))
            + f" | {dq_variants[-1]} - {dq_variants[0]}: "
            f"{(th_dq[-1] - th_dq[0])*1e3:+.3f} ms", flush=True)
        if args.no_sdpa:
            print(f"[round {r}] hip fwd {th_f*1e3:7.2f} ms "
                  f"{ffw/th_f/1e12:7.1f} TF"
                  f" | hip fwd v3 {th_f3*1e3:7.2f} ms "
                  f"{ffw/th_f3/1e12:7.1f} TF"
                  f" | hip bwd fused {th_b*1e3:7.2f} ms "
                  f"{fbw/th_b/1e12:7.1f} TF"
                  f" | hip bwd split {th_bs*1e3:7.2f} ms "
                  f"{fbw/th_bs/1e12:7.1f} TF", flush=True)
            continue
        ts_f = time_fn(sdpa_fwd, args.iters)
        ts_fb = time_fn(sdpa_fwdbwd, args.iters)
        print(f"[round {r}] hip fwd {th_f*1e3:7.2f} ms {ffw/th_f/1e12:7.1f} TF"
              f" | hip fwd v3 {th_f3*1e3:7.2f} ms {ffw/th_f3/1e12:7.1f} TF"
              f" | hip bwd fused {th_b*1e3:7.2f} ms {fbw/th_b/1e12:7.1f} TF"
              f" | hip bwd split {th_bs*1e3:7.2f} ms {fbw/th_bs/1e12:7.1f} TF"
              f" | sdpa fwd {ts_f*1e3:7.2f} ms {ffw/ts_f/1e12:7.1f} TF"
              f" | sdpa f+b {ts_fb*1e3:7.2f} ms "
              f"{(ffw+fbw)/ts_fb/1e12:7.1f} TF", flush=True)

    # the two forwards against each other
    o3, lse3 = hip_fwd_v3()
    print(f"max |O v4 - O v3| = "
          f"{(o_.float() - o3.float()).abs().max().item():.5f}, "
          f"max |LSE v4 - LSE v3| = {(lse_ - lse3).abs().max().item():.3e}")

    # the dQ kernels against each other
    dq0 = hip_bwd_dq(dq_variants[0])()[0]
    for x in dq_variants[1:]:
        dqx = hip_bwd_dq(x)()[0]
        print(f"max |dQ variant {dq_variants[0]} - dQ variant {x}| = "
              f"{(dq0.float() - dqx.float()).abs().max().item():.3e}")

    # correctness spot-check vs sdpa
    o_ref = sdpa_fwd().transpose(1, 2)
    err = (o_.float() - o_ref.float()).abs().max().item()
    print(f"max |hip - sdpa| = {err:.4f}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What grad clip + an LR schedule cost on the flagship step (dev tool,
not the driver contract; bench.py stays the headline measurement).

Variants, all at the bench.py flagship config (Llama-3-8B, one GPU):

  graph_plain      hip_graph, no clip, constant LR   (the headline config)
  graph_knobs      hip_graph + clip 1.0 + warmup/cosine: norm, clip
                   coefficient and LR all read from device memory
  eager_knobs      eager step + the same knobs, host clip path
                   (fp32 upcast of every bucket + coef.item() per step)
  eager_knobs_dev  eager step + the same knobs with clip_on_device=True
                   (not in the default set)
  graph_clip, graph_sched, graph_sched_flat
                   one knob at a time (not in the default set). Step time
                   depends on the values the GEMMs see, so a variant with
                   a different LR is not only a different code path:
                   graph_sched_flat runs the device-LR path at the plain LR

One variant per child process (an 8B trainer holds ~100 GB, two do not
fit comfortably), rounds alternate over the variants so drift hits all of
them alike. In the child the host clock goes around K steps issued with
sync=False and closed by a torch.cuda.synchronize().

  python tools/bench_step_knobs.py --rounds 3 --steps 8 --warmup 3

Prints one JSON line per run and one summary line per variant
(median / min / max ms per step).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = dict(grad_clip=1.0, lr_warmup_steps=100, lr_decay_steps=10000)
VARIANTS = {
    "graph_plain": dict(hip_graph=True),
    "graph_knobs": dict(hip_graph=True, **KNOBS),
    "eager_knobs": dict(hip_graph=False, **KNOBS),
    "eager_knobs_dev": dict(hip_graph=False, clip_on_device=True, **KNOBS),
    # one knob at a time, to tell the kernels' cost from the schedule's
    "graph_clip": dict(hip_graph=True, grad_clip=1.0),
    "graph_sched": dict(hip_graph=True, lr_warmup_steps=100,
                        lr_decay_steps=10000),
    # the device-LR path at (practically) the plain LR: step time depends
    # on the values the GEMMs see, and a warm-up LR leaves the weights
    # near their init
    "graph_sched_flat": dict(hip_graph=True, lr_decay_steps=10 ** 9),
}
DEFAULT = ["graph_plain", "graph_knobs", "eager_knobs"]


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", default=DEFAULT,
                    choices=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", type=str, default="llama3-8b")
    ap.add_argument("--micro-batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--child", type=str, default=None,
                    help=argparse.SUPPRESS)
    return ap.parse_args()


def child(args):
    from torch_on_k8s_amd.tunable import setup_tunableop
    setup_tunableop()
    import torch
    from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
    from torch_on_k8s_amd.parallel.env import DistContext

    torch.cuda.set_device(0)
    cfg = TrainerConfig(model=args.model,
                        model_overrides={"attn_impl": "hip"},
                        micro_batch=args.micro_batch, seq_len=args.seq_len,
                        **VARIANTS[args.child])
    tr = Trainer(cfg, DistContext(device=torch.device("cuda", 0)))
    for _ in range(args.warmup):
        tr.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = tr.train_step(sync=False)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    norm = tr.last_grad_norm()
    print(json.dumps({
        "variant": args.child,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "tokens_per_s": tr.tokens_per_step() * args.steps / elapsed,
        "steps": args.steps,
        "step_count": tr.step_count,
        "loss": float(loss.float().item()),
        "grad_norm": float(norm) if norm is not None else None,
    }), flush=True)


def main():
    args = parse_args()
    if args.child:
        child(args)
        return
    results = {v: [] for v in args.variants}
    for rnd in range(args.rounds):
        for v in args.variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v,
                   "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--model", args.model,
                   "--micro-batch", str(args.micro_batch),
                   "--seq-len", str(args.seq_len)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                # a failed variant ends the whole comparison: nothing more
                # is started on the GPU after a fault
                print(f"variant {v} round {rnd} failed "
                      f"(exit {p.returncode})", file=sys.stderr)
                sys.exit(1)
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            print(json.dumps(rec), flush=True)
            results[v].append(rec["ms_per_step"])
    for v, ms in results.items():
        print(json.dumps({
            "summary": v, "runs": len(ms),
            "ms_per_step_median": statistics.median(ms),
            "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
        }), flush=True)


if __name__ == "__main__":
    main()

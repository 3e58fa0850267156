"""Every kernel of a training step judged at the operands the MODEL gave it.

The kernel tests build synthetic operands and call one kernel alone. Inside
the model the operands are of another kind: the first block's norm has
res = None and the final norm's backward dxr = None, dO is a view of a dgrad
output, q, k and v come out of qkv_rope, the logits reach CE straight from a
GEMM, and the bounds tensors travel through every layer and through the
activation-checkpoint recompute. So this file spies on every binding of the
path (ops._C.* and ops.wgrad_gemm_ / ops.dgrad), lets the real function run,
records CPU copies of inputs and outputs, and then

 * judges every recorded call by the EXISTING per-element rule of its kernel
   from its own operands (kernel_oracle*.py; no new k or scale), and
 * asserts the ledger's shape: call counts, which optional operands were
   None, that every qkv_rope / attention call, recomputed ones included, got
   the test's bounds, and that attn_bwd got the o and lse of its own forward.

Runs: the `docs` case of test_model_oracle_gpu.py, the same with activation
checkpointing, and gpt2-tiny. Eager, default stream; never under hip_graph.
"""
import dataclasses

import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_attention as ka
import kernel_oracle_attention_docs as kd
import kernel_oracle_dgrad as kdg
import kernel_oracle_gemm as kg
import model_oracle as mo
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.gpt2 import GPT2_PRESETS, GPT2Model
from torch_on_k8s_amd.models.llama import LlamaModel, get_config

pytestmark = pytest.mark.gpu

B, S = 2, 192
DOCS = [[33, 31, 64, 64], [192]]
EXT = ["rmsnorm_res_fwd", "rmsnorm_res_bwd", "qkv_rope_fwd", "qkv_rope_bwd",
       "attn_fwd", "attn_bwd", "swiglu_fwd", "swiglu_bwd", "ce_fwd", "ce_bwd",
       "layernorm_fwd", "layernorm_bwd"]
PY = ["wgrad_gemm_", "dgrad"]
RUNS = {"docs": ("llama", False), "docs_ckpt": ("llama", True),
        "gpt2": ("gpt2", False)}


@dataclasses.dataclass
class Call:
    name: str
    args: list          # CPU copies of tensors; everything else as passed
    strides: list       # per argument: the tensor's strides, else None
    contiguous: list    # per argument: is_contiguous(), else None
    out: tuple          # CPU copies of the outputs
    extra: dict         # wgrad: `before`, `fast`

    def none(self, i):
        return len(self.args) <= i or self.args[i] is None


def _cpu(a):
    return a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a


def _spy(ledger, owner, name, mp):
    real = getattr(owner, name)

    def spy(*args, **kw):
        is_t = [isinstance(a, torch.Tensor) for a in args]
        rec = Call(name, [_cpu(a) for a in args],
                   [a.stride() if t else None for a, t in zip(args, is_t)],
                   [a.is_contiguous() if t else None
                    for a, t in zip(args, is_t)], (), {})
        if name == "wgrad_gemm_":
            rec.extra["fast"] = ops.wgrad_fast_path(*args[:3])
        out = real(*args, **kw)
        rec.out = tuple(_cpu(o) for o in
                        (out if isinstance(out, (tuple, list)) else (out,)))
        ledger.append(rec)
        return out

    mp.setattr(owner, name, spy)


@pytest.fixture(scope="module", params=list(RUNS))
def ledger(request):
    """One forward + backward of the run's model with every binding spied
    on. Returns (run name, model config, calls, bounds)."""
    family, ckpt = RUNS[request.param]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if family == "llama":
        model = LlamaModel(get_config("llama-tiny"),
                           activation_checkpointing=ckpt)
        ds, de = kd.bounds(DOCS, S)
        kw = {"doc_start": ds.to(dev), "doc_end": de.to(dev)}
    else:
        model = GPT2Model(GPT2_PRESETS["gpt2-tiny"])
        ds = de = None
        kw = {}
    model = mo.perturb_(model).to(dev).bfloat16().train()
    ids, labels = mo.tokens(B, S)
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        if family == "llama":
            mp.setenv("TOK_WGRAD_IMPL", "hip_all")
            mp.setenv("TOK_DGRAD_IMPL", "wt_all")
        else:
            mp.delenv("TOK_WGRAD_IMPL", raising=False)
            mp.delenv("TOK_DGRAD_IMPL", raising=False)
        for name in EXT:
            _spy(calls, ops._C, name, mp)
        for name in PY:
            _spy(calls, ops, name, mp)
        model(ids.to(dev), labels.to(dev), **kw).backward()
        torch.cuda.synchronize()
    n_linear = sum(1 for n, p in model.named_parameters()
                   if p.dim() == 2 and "embed" not in n)
    return request.param, model.cfg, calls, (ds, de), n_linear


def by_name(calls, name):
    return [c for c in calls if c.name == name]


def rows(t):
    return t.reshape(-1, t.shape[-1])


# --------------------------------------------------------------------------
# The ledger's shape
# --------------------------------------------------------------------------
def test_ledger_shape(ledger):
    run, cfg, calls, (ds, de), n_linear = ledger
    n = {name: len(by_name(calls, name)) for name in EXT + PY}
    print(f"LEDGER {run}: {n}")
    # every tensor a binding received is contiguous (the kernels index so)
    for c in calls:
        if c.name in EXT:
            assert all(f is not False for f in c.contiguous), (c.name,
                                                               c.strides)
    L = cfg.num_layers
    assert L == 2
    if run == "gpt2":
        assert n["layernorm_fwd"] == n["layernorm_bwd"] == 2 * L + 1 == 5
        assert n["attn_fwd"] == n["attn_bwd"] == L
        assert n["ce_fwd"] == n["ce_bwd"] == 1
        # GPT-2's projections are nn.Linear with biases, not ops.linear
        for name in ("rmsnorm_res_fwd", "rmsnorm_res_bwd", "qkv_rope_fwd",
                     "qkv_rope_bwd", "swiglu_fwd", "swiglu_bwd",
                     "wgrad_gemm_", "dgrad"):
            assert n[name] == 0, name
        for c in by_name(calls, "attn_fwd"):
            assert len(c.args) == 4
        return
    twice = 2 if run == "docs_ckpt" else 1      # block forwards, recomputed
    assert n["rmsnorm_res_fwd"] == 2 * L * twice + 1
    assert n["qkv_rope_fwd"] == n["attn_fwd"] == n["swiglu_fwd"] == L * twice
    assert n["rmsnorm_res_bwd"] == 2 * L + 1 == 5
    assert n["qkv_rope_bwd"] == n["attn_bwd"] == n["swiglu_bwd"] == L
    assert n["ce_fwd"] == n["ce_bwd"] == 1
    assert n["layernorm_fwd"] == n["layernorm_bwd"] == 0
    # one wgrad and one dgrad per linear weight: four per block and the
    # lm_head; the embedding's gradient is not a GEMM
    assert n_linear == 4 * L + 1 == 9
    assert n["wgrad_gemm_"] == n["dgrad"] == n_linear
    for c in by_name(calls, "wgrad_gemm_"):
        assert c.extra["fast"], [tuple(a.shape) for a in c.args[:3]]
        assert c.args[3] is False       # no flat buckets here: fresh tensors

    # res is None for the first block's input norm alone (and its recompute)
    fwd = by_name(calls, "rmsnorm_res_fwd")
    assert fwd[0].none(1)
    assert sum(c.none(1) for c in fwd) == twice
    # dxr is None for the final norm's backward alone: the first to run
    bwd = by_name(calls, "rmsnorm_res_bwd")
    assert bwd[0].none(3)
    assert sum(c.none(3) for c in bwd) == 1

    # the test's bounds reached every layer, forward, recompute and backward
    for c in by_name(calls, "qkv_rope_fwd"):
        assert len(c.args) == 7 and torch.equal(c.args[6], ds)
    for c in by_name(calls, "qkv_rope_bwd"):
        assert len(c.args) == 6 and torch.equal(c.args[5], ds)
    for c in by_name(calls, "attn_fwd"):
        assert len(c.args) == 6 and torch.equal(c.args[5], ds)
    for c in by_name(calls, "attn_bwd"):
        assert len(c.args) == 11
        assert torch.equal(c.args[9], ds) and torch.equal(c.args[10], de)


def test_attn_bwd_received_its_own_forward(ledger):
    run, cfg, calls, _, _ = ledger
    fwds = by_name(calls, "attn_fwd")
    for c in by_name(calls, "attn_bwd"):
        q, k, v, o, lse = c.args[:5]
        mine = [f for f in fwds if torch.equal(f.args[0], q)
                and torch.equal(f.args[1], k) and torch.equal(f.args[2], v)]
        # the layer's forward, and under checkpointing its recompute
        assert len(mine) == (2 if run == "docs_ckpt" else 1)
        for f in mine:
            assert torch.equal(f.out[0], o) and torch.equal(f.out[1], lse)


# --------------------------------------------------------------------------
# Every call by its kernel's rule
# --------------------------------------------------------------------------
def _doc_tables(cos, sin, ds_row):
    """Tables whose row s is position s - doc_start[s]: what ko.rope (row s
    = position s) needs to judge one packed row."""
    pos = torch.arange(ds_row.numel()) - ds_row.long()
    return cos[pos], sin[pos]


def _judge_rope(tag, x, got, cos, sin, ds, sign):
    """x, got: [B,S,H,D]; each batch row against ko.rope at its
    document-relative positions."""
    for b in range(x.shape[0]):
        cs, sn = (cos, sin) if ds is None else _doc_tables(cos, sin, ds[b])
        ko.check(f"{tag}[b{b}]", got[b:b + 1],
                 ko.rope(x[b:b + 1], cs, sn, sign))


def test_every_call_by_its_rule(ledger):
    run, cfg, calls, (ds, de), _ = ledger
    eps = cfg.ln_eps if run == "gpt2" else cfg.rms_eps
    layouts = None if run == "gpt2" else DOCS
    for i, c in enumerate(calls):
        tag, a, out = f"{run}.{i}.{c.name}", c.args, c.out
        if c.name == "rmsnorm_res_fwd":
            x, res, w = a[0], a[1], a[2]
            y, xr, invr = out
            if res is None:
                assert torch.equal(xr, x), tag
            else:
                ko.check(tag + ".xr", xr, ko.residual_sum(x, res))
            assert a[3] == eps
            # everything downstream is judged from the xr the kernel formed
            ko.check_all(tag, {"y": rows(y), "invr": invr},
                         ko.rmsnorm(rows(xr), w, eps))
        elif c.name == "rmsnorm_res_bwd":
            xr, w, dy, dxr = a[0], a[1], a[2], a[3]
            dx, dw = out
            assert dw.dtype == torch.float32
            ko.check_all(tag, {"dx": rows(dx), "dw": dw},
                         ko.rmsnorm(rows(xr), w, eps, rows(dy),
                                    rows(dxr) if dxr is not None else None))
        elif c.name == "qkv_rope_fwd":
            qkv, cos, sin, Hq, Hkv, D = a[:6]
            q, k, v = ko.qkv_split(qkv, Hq, Hkv, D)
            _judge_rope(tag + ".q", q, out[0], cos, sin, ds, 1.0)
            _judge_rope(tag + ".k", k, out[1], cos, sin, ds, 1.0)
            assert torch.equal(out[2], v), tag
        elif c.name == "qkv_rope_bwd":
            dq, dk, dv, cos, sin = a[:5]
            gq, gk, gv = ko.qkv_split(out[0], dq.shape[2], dk.shape[2],
                                      dq.shape[3])
            _judge_rope(tag + ".dq", dq, gq, cos, sin, ds, -1.0)
            _judge_rope(tag + ".dk", dk, gk, cos, sin, ds, -1.0)
            assert torch.equal(gv, dv), tag
        elif c.name == "attn_bwd":
            # with its forward: o and lse are that forward's outputs, bit
            # for bit (test_attn_bwd_received_its_own_forward)
            q, k, v, o, lse, do = a[:6]
            assert a[6] is True
            specs = ka.attention(q, k, v, do, True) if layouts is None \
                else kd.attention(q, k, v, do, layouts)
            ka.check_all(tag, {"o": o, "lse": lse, "dq": out[0],
                               "dk": out[1], "dv": out[2]}, specs)
        elif c.name == "attn_fwd":
            assert a[3] is True         # judged with its backward
        elif c.name == "swiglu_fwd":
            ko.check(tag, rows(out[0]), ko.swiglu(rows(a[0]))["out"])
        elif c.name == "swiglu_bwd":
            ko.check(tag, rows(out[0]),
                     ko.swiglu(rows(a[1]), rows(a[0]))["dgu"])
        elif c.name == "ce_fwd":
            sp = ko.cross_entropy(a[0], a[1])
            ko.check_all(tag, {"loss_rows": out[0], "lse": out[1]},
                         {n: sp[n] for n in ("loss_rows", "lse")})
        elif c.name == "ce_bwd":
            # gscale is grad_out / rows, formed on the device
            N = a[0].shape[0]
            assert N == B * S
            sp = ko.cross_entropy(a[0], a[1], grad_out=float(a[3]) * N)
            ko.check(tag, out[0], sp["dlogits"])
        elif c.name == "layernorm_fwd":
            assert a[3] == eps
            sp = ko.layernorm(rows(a[0]), a[1], a[2], eps)
            ko.check_all(tag, {"y": rows(out[0]), "mu": out[1],
                               "rstd": out[2]}, sp)
        elif c.name == "layernorm_bwd":
            x, w, dy = a[0], a[1], a[2]
            assert out[1].dtype == out[2].dtype == torch.float32
            # the bias moves y alone, which this call does not produce
            sp = ko.layernorm(rows(x), w, torch.zeros_like(w), eps, rows(dy))
            ko.check_all(tag, {"dx": rows(out[0]), "dw": out[1],
                               "db": out[2]},
                         {n: sp[n] for n in ("dx", "dw", "db")})
        elif c.name == "wgrad_gemm_":
            dy, x, before, acc = a[:4]
            ko.check(f"{tag}[{tuple(before.shape)}]", out[0],
                     kg.wgrad(dy, x, before if acc else None))
        elif c.name == "dgrad":
            ko.check(f"{tag}[{tuple(a[1].shape)}]", out[0],
                     kdg.dgrad(a[0], a[1]))
        else:
            raise AssertionError(c.name)

"""The HIP training path as a whole against the independent fp64 model of
model_oracle.py: logits, loss and every parameter gradient, by the
calibrated criterion (r2 <= M and rmax <= M against the bf16-storage
emulation run on the same bf16 weights and tokens; see model_oracle.py and
docs/TESTING.md).

Models are built directly, LlamaModel(cfg).to(dev).bfloat16(), and called as
model(ids, labels, doc_start, doc_end) followed by backward(). All cases are
hidden 256, 2 layers, vocab 512; B S = 384 is a multiple of 64, so the HIP
wgrad takes its fast path under TOK_WGRAD_IMPL=hip_all.

Without tolerance, on `base` and `docs`: activation checkpointing gives the
bits of the run without it (the recompute launches the same kernels on the
same bits), and bounds that describe one document per row give the bits of
the call without bounds: the loss, the logits and every gradient except the
norm weights', whose fp32 atomics have no fixed order (_assert_same_bits);
those are held to the oracle in both runs.

The trainer case holds ops.doc_bounds (derived on the device from the
batch), the flat-bucket in-place wgrad and two accumulated micro-batches to
the oracle together.
"""
import functools

import numpy as np
import pytest
import torch

import model_oracle as mo
from kernel_oracle_attention_docs import bounds
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.models.gpt2 import GPT2_PRESETS, GPT2Model
from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.parallel.env import DistContext

pytestmark = pytest.mark.gpu

HIP = {"TOK_WGRAD_IMPL": "hip_all", "TOK_DGRAD_IMPL": "wt_all"}
DOCS = ((33, 31, 64, 64), (192,))
# case: (config overrides, S, layouts, env; None = the defaults)
CASES = {
    "base": ({}, 192, None, HIP),
    "docs": ({}, 192, DOCS, HIP),
    "ragged": ({}, 200, ((33, 31, 72, 64), (200,)), None),
    "d128": (dict(head_dim=128, num_heads=2, num_kv_heads=1), 192, DOCS, HIP),
    "gqa4": (dict(num_heads=4, num_kv_heads=1), 192, DOCS, HIP),
    "tied": (dict(tie_embeddings=True), 192, None, HIP),
    "gpt2": (None, 192, None, None),
}
B = 2


def dev():
    return torch.device("cuda", 0)


def set_env(monkeypatch, env):
    for name in HIP:
        if env is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, env[name])


def build(case, **kw):
    """The case's model with bf16-valued, perturbed weights, on the GPU."""
    over = CASES[case][0]
    torch.manual_seed(0)
    if over is None:
        model = GPT2Model(GPT2_PRESETS["gpt2-tiny"], **kw)
    else:
        model = LlamaModel(get_config("llama-tiny", **over), **kw)
    return mo.perturb_(model).to(dev()).bfloat16()


def device_bounds(layouts, S):
    if layouts is None:
        return {}
    ds, de = bounds([list(l) for l in layouts], S)
    return {"doc_start": ds.to(dev()), "doc_end": de.to(dev())}


def run_hip(model, ids, labels, **kw):
    """logits (a forward of their own), then loss and gradients."""
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        logits = model(ids.to(dev()), **kw)
    loss = model(ids.to(dev()), labels.to(dev()), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return {"logits": logits, "loss": loss.detach(),
            "grads": {n: p.grad for n, p in model.named_parameters()}}


def cpu_state(module):
    return {n: v.detach().cpu() for n, v in module.state_dict().items()}


@functools.lru_cache(maxsize=None)
def references(case):
    """(ref64, emu) tensors of a case: once, shared, unchanged."""
    over, S, layouts, _ = CASES[case]
    model = build(case)
    ids, labels = mo.tokens(B, S)
    state, cfg = cpu_state(model), model.cfg.to_dict()
    if over is None:
        f = lambda storage: mo.gpt2(state, cfg, ids, labels, storage=storage)
    else:
        lay = [list(l) for l in layouts] if layouts is not None else None
        f = lambda storage: mo.llama(state, cfg, ids, labels, lay,
                                     storage=storage)
    return mo.tensors(f("fp64")), mo.tensors(f("bf16"))


@pytest.mark.parametrize("case", list(CASES))
def test_hip_model_against_fp64_oracle(case, monkeypatch):
    _, S, layouts, env = CASES[case]
    set_env(monkeypatch, env)
    ref, emu = references(case)
    ids, labels = mo.tokens(B, S)
    got = run_hip(build(case), ids, labels, **device_bounds(layouts, S))
    mo.check(case, mo.tensors(got), ref, emu)


def _assert_same_bits(a, b, what):
    """Loss and every gradient but the norm weights'. Those cannot be held
    to bit equality, between any two runs: rmsnorm.hip's colsum_kernel folds
    the per-row-split partials of dw with one fp32 atomicAdd per column per
    block (384 blocks at these shapes), in whatever order the blocks retire.
    Nothing downstream reads dw, so nothing else inherits the order. The
    callers hold both runs' norm-weight gradients to the oracle instead."""
    assert torch.equal(a["loss"], b["loss"]), what
    assert set(a["grads"]) == set(b["grads"])
    compared = 0
    for n, g in a["grads"].items():
        if g.dim() == 1:
            assert "norm" in n, n
            continue
        assert torch.equal(g, b["grads"][n]), (what, n)
        compared += 1
    assert compared >= 10       # embedding, 4 per block, lm_head


@pytest.mark.parametrize("case", ["base", "docs"])
def test_activation_checkpointing_gives_the_same_bits(case, monkeypatch):
    _, S, layouts, env = CASES[case]
    set_env(monkeypatch, env)
    ids, labels = mo.tokens(B, S)
    kw = device_bounds(layouts, S)
    plain = build(case).train()
    ckpt = build(case, activation_checkpointing=True).train()
    a = run_hip(plain, ids, labels, **kw)
    b = run_hip(ckpt, ids, labels, **kw)
    _assert_same_bits(a, b, "checkpointing")
    ref, emu = references(case)
    mo.check(case + ".plain", mo.tensors(a), ref, emu)
    mo.check(case + ".ckpt", mo.tensors(b), ref, emu)


@pytest.mark.parametrize("case", ["base", "docs"])
def test_one_document_per_row_is_the_plain_call_bitwise(case, monkeypatch):
    _, S, _, env = CASES[case]
    set_env(monkeypatch, env)
    ids, labels = mo.tokens(B, S)
    model = build(case)
    a = run_hip(model, ids, labels)
    a = {"logits": a["logits"], "loss": a["loss"],
         "grads": {n: g.clone() for n, g in a["grads"].items()}}
    b = run_hip(model, ids, labels, **device_bounds(((S,), (S,)), S))
    assert torch.equal(a["logits"], b["logits"])
    _assert_same_bits(a, b, "one document per row")
    # one document per row IS the plain model: the `base` references
    ref, emu = references("base")
    mo.check(case + ".plain", mo.tensors(a), ref, emu)
    mo.check(case + ".one_doc", mo.tensors(b), ref, emu)


# --------------------------------------------------------------------------
# Trainer: bounds derived on the device, flat-bucket wgrad, accumulation
# --------------------------------------------------------------------------
EOS = 0
S_TR = 192


@pytest.fixture(scope="module")
def token_file(tmp_path_factory):
    """Documents of 5..90 tokens, EOS-terminated, packed end to end."""
    rng = np.random.default_rng(0)
    toks = rng.integers(1, 512, 24 * (S_TR + 1))
    ends = np.cumsum(rng.integers(5, 91, 400))
    toks[ends[ends < len(toks)]] = EOS
    path = tmp_path_factory.mktemp("data") / "tokens.bin"
    toks.astype("<u2").tofile(path)
    return str(path)


def test_trainer_backward_against_fp64_oracle(token_file, monkeypatch):
    set_env(monkeypatch, HIP)
    torch.cuda.set_device(0)
    tr = Trainer(TrainerConfig(model="llama-tiny", micro_batch=B,
                               seq_len=S_TR, data_path=token_file,
                               doc_eos_id=EOS),
                 DistContext(device=dev()))
    mo.perturb_(tr.module)
    state, cfg = cpu_state(tr.module), tr.model_cfg.to_dict()
    params = dict(tr.module.named_parameters())
    assert all(getattr(p, "_tok_flat_grad", False) for p in params.values())

    def oracle(inp, lab, storage):
        lay = mo.layouts_from_ids(inp.cpu(), EOS)
        t = mo.tensors(mo.llama(state, cfg, inp.cpu(), lab.cpu(), lay,
                                storage=storage))
        del t["logits"]             # the trainer hands out the loss only
        return lay, t

    def got(loss):
        torch.cuda.synchronize()
        return mo.tensors({"logits": torch.zeros(()), "loss": loss.detach(),
                           "grads": {n: p.grad for n, p in params.items()}})

    tr.fb.zero_grads()
    tr.fb.set_accumulate(True)
    inp, lab = tr.data.batch(0)
    loss0 = tr._loss(inp, lab)
    loss0.backward()
    lay0, ref0 = oracle(inp, lab, "fp64")
    _, emu0 = oracle(inp, lab, "bf16")
    assert max(len(l) for l in lay0) >= 2       # the batch holds boundaries
    mo.check("trainer.batch0", got(loss0), ref0, emu0)

    # a second micro-batch accumulated into the same flat grads
    tr.fb.set_accumulate(False)
    inp, lab = tr.data.batch(1)
    loss1 = tr._loss(inp, lab)
    loss1.backward()
    _, ref1 = oracle(inp, lab, "fp64")
    _, emu1 = oracle(inp, lab, "bf16")
    ref = {n: (ref1[n] if n == "loss" else ref0[n] + ref1[n]) for n in ref1}
    emu = {n: (emu1[n] if n == "loss" else emu0[n] + emu1[n]) for n in emu1}
    mo.check("trainer.batch0+1", got(loss1), ref, emu)

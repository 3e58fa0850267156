"""The whole-model fp64 oracle (model_oracle.py) held against the package on
the CPU, and its criterion given teeth.

 * fp64 mode IS the package's model: LlamaModel / GPT2Model in .double() on
   the CPU path, same weights, agree in logits, loss and every gradient to
   1e-10 relative L2 (conventions, head order, label convention, structure;
   the norm weights and biases are perturbed off their init values so that
   none of them is interchangeable with another).
 * A packed row is each document on its own: the oracle on the packed row
   against the oracle on every document as a row of its own.
 * The package's CPU path with a .bfloat16() model stays inside the
   criterion (r2 <= M and rmax <= M against the bf16-storage emulation).
 * Every mutant reaches r2 >= 2 M on every tensor SPOILS lists for it.
"""
import functools

import pytest
import torch

import model_oracle as mo
from kernel_oracle import f64
from kernel_oracle_attention_docs import bounds
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.gpt2 import GPT2_PRESETS, GPT2Model
from torch_on_k8s_amd.models.llama import LlamaModel, get_config

B, S = 2, 192
DOCS = ((33, 31, 64, 64), (192,))
CASES = {
    "base": ({}, None),
    "docs": ({}, DOCS),
    "tied": ({"tie_embeddings": True}, None),
    "tied_docs": ({"tie_embeddings": True}, DOCS),
}


def rel(a, b):
    a, b = f64(a), f64(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def tokens():
    return mo.tokens(B, S)


@functools.lru_cache(maxsize=None)
def llama_model(tied):
    torch.manual_seed(0)
    return mo.perturb_(LlamaModel(get_config("llama-tiny",
                                             tie_embeddings=tied)))


@functools.lru_cache(maxsize=None)
def gpt2_model():
    torch.manual_seed(0)
    return mo.perturb_(GPT2Model(GPT2_PRESETS["gpt2-tiny"]))


def run_package(model, dtype, ids, labels, layouts):
    """logits, loss and gradients of a copy of `model` in `dtype` on the
    package's CPU path."""
    m = type(model)(model.cfg)
    m.load_state_dict(model.state_dict())
    m = m.to(dtype)
    kw = {}
    if layouts is not None:
        kw["doc_start"], kw["doc_end"] = bounds([list(l) for l in layouts], S)
    with torch.no_grad():
        logits = m(ids, **kw)
    loss = m(ids, labels, **kw)
    loss.backward()
    return {"logits": logits, "loss": loss.detach(),
            "grads": {n: p.grad for n, p in m.named_parameters()}}


@functools.lru_cache(maxsize=None)
def oracle(case, storage="fp64", wrong=None):
    """One oracle run per (case, storage, mutant), shared and unchanged."""
    ids, labels = tokens()
    if case == "gpt2":
        model = gpt2_model()
        return mo.gpt2(model.state_dict(), model.cfg.to_dict(), ids, labels,
                       storage=storage, wrong=wrong)
    over, layouts = CASES[case]
    model = llama_model(bool(over))
    lay = [list(l) for l in layouts] if layouts is not None else None
    return mo.llama(model.state_dict(), model.cfg.to_dict(), ids, labels,
                    lay, storage=storage, wrong=wrong)


def package(case, dtype):
    ids, labels = tokens()
    if case == "gpt2":
        return run_package(gpt2_model(), dtype, ids, labels, None)
    over, layouts = CASES[case]
    return run_package(llama_model(bool(over)), dtype, ids, labels, layouts)


ALL = list(CASES) + ["gpt2"]


@pytest.mark.parametrize("case", ALL)
def test_fp64_mode_is_the_package_model(case):
    want = mo.tensors(oracle(case))
    got = mo.tensors(package(case, torch.float64))
    assert set(got) == set(want)
    worst = max((rel(got[n], want[n]), n) for n in want)
    print(f"fp64 {case}: worst relative L2 {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 1e-10, worst


@pytest.mark.parametrize("case", ["docs", "tied_docs"])
def test_packed_row_is_each_document_alone(case):
    over, layouts = CASES[case]
    model = llama_model(bool(over))
    state, cfg = model.state_dict(), model.cfg.to_dict()
    ids, labels = tokens()
    packed = oracle(case)
    total = {n: torch.zeros_like(g) for n, g in packed["grads"].items()}
    loss = 0.0
    for b, lengths in enumerate(layouts):
        a = 0
        for L in lengths:
            alone = mo.llama(state, cfg, ids[b:b + 1, a:a + L],
                             labels[b:b + 1, a:a + L])
            assert rel(alone["logits"], packed["logits"][b:b + 1, a:a + L]) \
                <= 1e-10, (b, a)
            share = L / (B * S)     # of the mean over the packed batch
            loss = loss + share * alone["loss"]
            for n, g in alone["grads"].items():
                total[n] += share * g
            a += L
    assert rel(loss, packed["loss"]) <= 1e-10
    for n, g in packed["grads"].items():
        assert rel(total[n], g) <= 1e-10, n
    # and the bounds are not idle: the plain row is another function
    plain = oracle("tied" if over else "base")
    assert rel(plain["logits"], packed["logits"]) > 1e-3


def test_layouts_from_ids_follow_doc_bounds():
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 6, (5, 40), generator=g)    # EOS = 0, often
    ids[0, 0] = 0           # a one-token document at the row start
    ids[1, -1] = 0          # an EOS that ends the row
    ids[2] = 3              # no EOS at all
    ids[3, 10:13] = 0       # one-token documents in a run
    layouts = mo.layouts_from_ids(ids, 0)
    ds, de = bounds(layouts, 40)
    ws, we = ops.doc_bounds(ids, 0)
    assert torch.equal(ds, ws) and torch.equal(de, we)
    assert layouts[2] == [40] and layouts[0][0] == 1
    assert torch.equal(mo.doc_starts(layouts, 40), ws.long())


@pytest.mark.parametrize("case", ALL)
def test_cpu_bf16_path_is_inside_the_criterion(case):
    ref, emu = mo.tensors(oracle(case)), mo.tensors(oracle(case, "bf16"))
    got = mo.tensors(package(case, torch.bfloat16))
    rat = mo.check(f"cpu_bf16.{case}", got, ref, emu)
    for n, (r2, rmax) in sorted(rat.items()):
        print(f"  {n}: r2={r2:.3f} rmax={rmax:.3f}")


def spoiled(mutant, names):
    """The tensors `mutant` must move by r2 >= 2 M, with the reason for
    every tensor left out."""
    grads = [n for n in names if n.startswith("grad:")]
    if mutant == "res_grad_dropped":
        # The forward does not change: not logits, not the loss. Block 1
        # forms xr = x + res; dropping d/dres leaves d/dx (block 0's MLP
        # output) as it was, so block 0's MLP and, through an unchanged dy,
        # its post_attn_norm weight keep their gradients. What is lost is
        # the dxr of block 0's post-attention norm: everything in front of
        # it.
        return ["grad:embed_tokens.weight", "grad:layers.0.input_norm.weight",
                "grad:layers.0.attn.qkv_proj.weight",
                "grad:layers.0.attn.o_proj.weight"]
    if mutant == "rope_not_restarted":
        # Nothing at the model's outputs. RoPE scores depend on i - j alone:
        # with the mask in place, phases counted from the row start give
        # every document the scores it has with phases counted from its own
        # first token, for ANY weights, so logits, loss and with them every
        # gradient are the same function (docs/TESTING.md). The restart is
        # visible in the roped q and k only; test_rope_restart_* below and
        # the per-call ledger of test_model_calls_gpu.py hold it there.
        return []
    if mutant == "label_shift":
        return ["loss"] + grads             # the logits do not see labels
    if mutant == "mean_divisor_off":
        # 1/(B S - 1) against 1/(B S) scales every gradient by 1 + 1/383 =
        # 0.26 %, all elements alike: below one bf16 rounding (2^-9 = 0.2 %
        # mean, 0.39 % worst) of the stored gradient, so no criterion built
        # on bf16 storage can see it there. The loss is fp32 and shows it.
        return ["loss"]
    if mutant == "tied_embed_grad_dropped":
        return ["grad:embed_tokens.weight"]
    # kv_head_rolled, mask_not_applied, mask_start_plus_one,
    # swiglu_halves_swapped, bounds_dropped_in_layer1: the forward changes
    # in or before the last block, so the logits and every gradient move.
    # Not the loss: with untrained weights it is ln V give or take a little
    # whatever the blocks compute (a scalar, and e(emu) of a scalar is one
    # draw of rounding noise), so only the mutants of the loss formula
    # itself are held to it.
    return ["logits"] + grads


def mutant_case(mutant):
    if mutant in mo.NEEDS_TIED:
        return "tied"
    return "docs"


@pytest.mark.parametrize("mutant", mo.MUTANTS)
def test_teeth(mutant):
    case = mutant_case(mutant)
    ref, emu = mo.tensors(oracle(case)), mo.tensors(oracle(case, "bf16"))
    rat = mo.ratios(mo.tensors(oracle(case, "fp64", mutant)), ref, emu)
    names = spoiled(mutant, list(ref))
    for n, (r2, rmax) in sorted(rat.items()):
        print(f"  {mutant} {n}: r2={r2:.2f}{' *' if n in names else ''}")
    if names:
        low = min((rat[n][0], n) for n in names)
        print(f"TEETH {mutant}: smallest listed r2={low[0]:.2f} ({low[1]})")
        assert low[0] >= 2 * mo.M, low


def test_rope_restart_shows_in_q_and_k_only():
    """The one mutant with nothing to show at the outputs: its roped q and k
    differ from the model's at every document but a row's first."""
    good, bad = oracle("docs"), oracle("docs", "fp64", "rope_not_restarted")
    a = DOCS[0][0]
    for (q, k), (qw, kw) in zip(good["qk"], bad["qk"]):
        assert torch.equal(q[0, :a], qw[0, :a])
        assert rel(qw[0, a:], q[0, a:]) > 0.1
        assert rel(kw[0, a:], k[0, a:]) > 0.1
        assert torch.equal(q[1], qw[1])         # row 1 is one document
    assert rel(bad["logits"], good["logits"]) < 1e-5


@pytest.mark.parametrize("used", ["y", "xr", "both"])
def test_fused_norm_backward_with_an_unused_output(used):
    """ops.rmsnorm_residual hands an unused output's gradient to its
    backward as None (the final norm's xr; test_model_calls_gpu.py pins that
    the kernel then gets dxr = None): every combination gives the gradients
    of the plain formula."""
    g = torch.Generator().manual_seed(7)
    x, res = (torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
              for _ in range(2))
    w = torch.randn(16, generator=g, dtype=torch.float64)
    dy, dxr = (torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
               for _ in range(2))

    def outputs(fused, x, res, w):
        if fused:
            y, xr = ops.rmsnorm_residual(x, res, w, 1e-5)
        else:
            xr = x + res
            y = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-5) * w
        outs, gs = [], []
        if used in ("y", "both"):
            outs.append(y), gs.append(dy)
        if used in ("xr", "both"):
            outs.append(xr), gs.append(dxr)
        return outs, gs

    grads = []
    for fused in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (x, res, w)]
        outs, gs = outputs(fused, *leaves)
        torch.autograd.backward(outs, gs)
        grads.append([t.grad for t in leaves])
    for a, b, n in zip(*grads, ("dx", "dres", "dw")):
        if used == "xr" and n == "dw":
            assert b is None and float(a.abs().max()) == 0.0
        else:
            assert rel(a, b) <= 1e-12, n


def test_mutants_refuse_what_they_cannot_spoil():
    ids, labels = tokens()
    model = llama_model(False)
    with pytest.raises(ValueError):
        mo.llama(model.state_dict(), model.cfg.to_dict(), ids, labels,
                 wrong="mask_not_applied")
    with pytest.raises(ValueError):
        mo.llama(model.state_dict(), model.cfg.to_dict(), ids, labels,
                 wrong="tied_embed_grad_dropped")
    with pytest.raises(ValueError):
        mo.llama(model.state_dict(), model.cfg.to_dict(), ids, labels,
                 wrong="no_such_mutant")

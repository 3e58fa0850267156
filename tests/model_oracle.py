"""An independent fp64 model: Llama and GPT-2 written out in plain torch ops
under ordinary autograd, for holding the COMPOSITION of the HIP kernels
(logits, loss, every parameter gradient) to something that shares no code
with the package.

Imports torch and ``kernel_oracle`` (``q16``, ``f64``) and nothing from
``torch_on_k8s_amd``. The per-call rules of ``kernel_oracle*.py`` are derived
from a kernel's arithmetic; a whole model has no such derivation (errors pass
through two blocks of normalisations and softmaxes), so it gets a CALIBRATED
criterion instead:

    storage="fp64"   the model in float64 on the values it is given
    storage="bf16"   the same computation with every tensor the HIP path
                     stores in bf16 rounded to bf16 where it is stored, in
                     the forward and (the matching gradient) in the backward:
                     norm outputs and xr, GEMM outputs, roped q/k/v,
                     attention O, the SwiGLU output, the logits, the parameter
                     gradients. Everything between two such points stays
                     fp64. It says how far an honest bf16-storage
                     implementation lands from fp64 on THIS input ("emu").

With e(x) = x - ref64, per tensor T (logits, loss, each parameter gradient):

    r2   = ||e(x)||_2 / ||e(emu)||_2
    rmax = max|e(x)| / max|e(emu)|

and the criterion is r2 <= M and rmax <= M for every tensor. M is ONE
constant, never fitted per tensor and never set from HIP outputs alone.

Where M started: 3. The emulation rounds once per stored tensor. The HIP
path also rounds P, dS^T and the O that delta reads inside attention (the
attention oracle's printed tol_shares put that `mid` term on the order of
the output rounding), accumulates in fp32, and the emulation is a single
sample of rounding noise. M may rise only after an honest GPU run exceeds it
while every per-call rule holds, and only as far as the teeth condition
2 M <= (smallest ratio of any mutant on any tensor it lists) still holds.

Why M = 12 now. That happened, on one tensor: the loss. It is a scalar, so
e(emu) is not a norm over thousands of roundings but ONE draw of a zero-mean
error, and the ratio of two such draws of equal spread exceeds m with
probability (2/pi) atan(1/m): 20 % at m = 3, whatever the implementation.
On the `ragged` case the emulation's draw came out at 6.3e-6 where the
other cases have 2.5e-5 .. 1.2e-4 (and the per-row loss errors put the
standard error of the mean at 8e-5); the HIP loss, 3.7e-5 off, like every
other case, is then at ratio 5.9 with every recorded call inside its
derived rule. M = 12 leaves an honest scalar a 5 % chance per case of
falling outside and keeps 2 M = 24 under the smallest listed mutant ratio
(33.6, swiglu_halves_swapped on the final norm's weight gradient). The
reasoning behind 3 is untouched for every tensor of more than one element,
where the norms concentrate (measured on the GPU: at most 1.4), so those are
ALSO held to M_TENSOR = 3: a second, stricter condition on top of the
criterion, not a replacement for it. Measured ratios: profiles/README.md.

``wrong=`` selects one deliberately wrong model (MUTANTS); SPOILS lists, per
mutant, the tensors on which it must reach r2 >= 2 M, with the reason for
every tensor that is NOT listed.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from kernel_oracle import f64, q16

M = 12.0            # every tensor (see above for why it is not 3)
M_TENSOR = 3.0      # on top, for every tensor of more than one element

MUTANTS = (
    "res_grad_dropped", "kv_head_rolled", "rope_not_restarted",
    "mask_not_applied", "mask_start_plus_one", "label_shift",
    "mean_divisor_off", "swiglu_halves_swapped", "tied_embed_grad_dropped",
    "bounds_dropped_in_layer1",
)
NEEDS_LAYOUTS = ("rope_not_restarted", "mask_not_applied",
                 "mask_start_plus_one", "bounds_dropped_in_layer1")
NEEDS_TIED = ("tied_embed_grad_dropped",)


# --------------------------------------------------------------------------
# bf16 storage points
# --------------------------------------------------------------------------
def _r16(t: torch.Tensor) -> torch.Tensor:
    return q16(t).to(torch.float64)


class _Stored(torch.autograd.Function):
    """A tensor the HIP path keeps in bf16: the value is rounded on the way
    forward and its gradient on the way back."""

    @staticmethod
    def forward(ctx, x):
        return _r16(x)

    @staticmethod
    def backward(ctx, g):
        return _r16(g)


def _storage(storage: str):
    if storage == "fp64":
        return lambda t: t
    if storage == "bf16":
        return _Stored.apply
    raise ValueError(f"storage must be fp64 or bf16, got {storage!r}")


def _params(state: dict, skip=()) -> dict:
    return {n: f64(v).clone().requires_grad_(True)
            for n, v in state.items() if n not in skip}


def _finish(logits, loss, params, storage) -> dict:
    loss.backward()
    grads = {}
    for n, p in params.items():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        grads[n] = _r16(g) if storage == "bf16" else g.clone()
    return {"logits": logits.detach(), "loss": loss.detach(), "grads": grads}


# --------------------------------------------------------------------------
# Inputs shared by the CPU and GPU tests
# --------------------------------------------------------------------------
def tokens(B: int, S: int, seed: int = 1, vocab: int = 512):
    """(ids, labels), int64 [B, S]: next-token pairs of one random row of
    S + 1 tokens per batch entry, none of them token 0."""
    t = torch.randint(1, vocab, (B, S + 1),
                      generator=torch.Generator().manual_seed(seed))
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


@torch.no_grad()
def perturb_(module, seed: int = 5):
    """Move every 1-D parameter (norm weights, biases) off its init value
    of one or zero, so that none is interchangeable with another, and round
    all parameters to bf16 values. In place; returns the module."""
    g = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        if p.dim() == 1:
            p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p))
        p.copy_(q16(p).to(p.dtype))
    return module


# --------------------------------------------------------------------------
# Packed documents
# --------------------------------------------------------------------------
def layouts_from_ids(ids, eos: int) -> list:
    """Document lengths per row from the token ids alone: the token after an
    EOS starts a new document, the EOS belongs to the document it ends, and
    a row's last document ends with the row."""
    a = np.asarray(torch.as_tensor(ids).cpu().numpy())
    out = []
    for row in a:
        cuts = [int(i) + 1 for i in np.nonzero(row == eos)[0]
                if i + 1 < len(row)]
        edges = [0] + cuts + [len(row)]
        out.append([e - s for s, e in zip(edges[:-1], edges[1:])])
    return out


def doc_starts(layouts, S: int) -> torch.Tensor:
    """int64 [B, S]: the row index of the first token of each token's
    document."""
    ds = torch.zeros(len(layouts), S, dtype=torch.long)
    for b, lengths in enumerate(layouts):
        assert sum(lengths) == S and min(lengths) >= 1, (lengths, S)
        a = 0
        for L in lengths:
            ds[b, a:a + L] = a
            a += L
    return ds


# --------------------------------------------------------------------------
# Pieces
# --------------------------------------------------------------------------
def rope_table(S: int, D: int, theta: float):
    """cos/sin [S, D/2]: built in fp64 and rounded to fp32, as the model's
    host-side table is."""
    half = D // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    ang = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return ang.cos().float().double(), ang.sin().float().double()


def _rope(x, cos, sin, pos):
    """x [B,S,H,D], rotate-half; pos int64 [B,S]."""
    D = x.shape[-1]
    cs, sn = cos[pos].unsqueeze(2), sin[pos].unsqueeze(2)
    a, b = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([a * cs - b * sn, b * cs + a * sn], -1)


def _attention(q, k, v, lo, kv_roll=0):
    """Causal GQA attention as an explicit masked softmax. q [B,S,Hq,D],
    k/v [B,S,Hkv,D]; lo int64 [B,S]: query i sees keys lo[b,i] .. i."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    hk = (torch.arange(Hq) // (Hq // Hkv) + kv_roll) % Hkv
    qh = q.permute(0, 2, 1, 3)
    kh = k.permute(0, 2, 1, 3)[:, hk]
    vh = v.permute(0, 2, 1, 3)[:, hk]
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    i = torch.arange(S).view(1, S, 1)
    j = torch.arange(S).view(1, 1, S)
    ok = (j <= i) & (j >= lo.view(B, S, 1))
    s = s.masked_fill(~ok.unsqueeze(1), float("-inf"))
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3)


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * w + b


def _mean_ce(logits, labels, divisor):
    x = logits.reshape(-1, logits.shape[-1])
    lab = torch.as_tensor(labels).cpu().long().reshape(-1, 1)
    rows = torch.logsumexp(x, -1) - x.gather(1, lab).squeeze(1)
    return rows.sum() / divisor


def _gelu_tanh(x):
    c = math.sqrt(2.0 / math.pi)
    return 0.5 * x * (1.0 + torch.tanh(c * (x + 0.044715 * x.pow(3))))


# --------------------------------------------------------------------------
# Llama
# --------------------------------------------------------------------------
def llama(state, cfg_dict, ids, labels, layouts=None, *, storage="fp64",
          wrong=None) -> dict:
    """state: name -> tensor as LlamaModel.state_dict() gives it (converted
    to fp64 after whatever rounding the caller applied). labels are the
    targets of the logits row for row, as LlamaModel.forward takes them.
    Returns {"logits" [B,S,V], "loss", "grads": {parameter name: tensor},
    "qk": [(roped q, roped k) per layer]}, all fp64."""
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    if wrong in NEEDS_LAYOUTS and layouts is None:
        raise ValueError(f"{wrong} needs layouts")
    c = cfg_dict
    tied = bool(c["tie_embeddings"])
    if wrong in NEEDS_TIED and not tied:
        raise ValueError(f"{wrong} needs tie_embeddings")
    R = _storage(storage)
    p = _params(state, skip=("lm_head.weight",) if tied else ())
    ids = torch.as_tensor(ids).cpu().long()
    labels = torch.as_tensor(labels).cpu().long()
    B, S = ids.shape
    Hq, Hkv, D = c["num_heads"], c["num_kv_heads"], c["head_dim"]
    I, eps = c["intermediate_size"], c["rms_eps"]
    cos, sin = rope_table(S, D, c["rope_theta"])
    row = torch.arange(S).unsqueeze(0).expand(B, S)
    zero = torch.zeros(B, S, dtype=torch.long)
    ds = doc_starts(layouts, S) if layouts is not None else zero

    emb = p["embed_tokens.weight"]
    if wrong == "tied_embed_grad_dropped":
        emb = emb.detach()
    x, res, qk = R(emb[ids]), None, []
    for i in range(c["num_layers"]):
        pre = f"layers.{i}."
        dsi = zero if (wrong == "bounds_dropped_in_layer1" and i == 1) else ds
        if res is None:
            xr = x
        elif wrong == "res_grad_dropped" and i == 1:
            xr = R(x + res.detach())
        else:
            xr = R(x + res)
        h = R(_rms(xr, p[pre + "input_norm.weight"], eps))
        qkv = R(h @ p[pre + "attn.qkv_proj.weight"].t())
        parts = qkv.view(B, S, Hq + 2 * Hkv, D)
        pos = row if wrong == "rope_not_restarted" else row - dsi
        q = R(_rope(parts[:, :, :Hq], cos, sin, pos))
        k = R(_rope(parts[:, :, Hq:Hq + Hkv], cos, sin, pos))
        v = R(parts[:, :, Hq + Hkv:])
        qk.append((q.detach(), k.detach()))
        if wrong == "mask_not_applied":
            lo = zero
        elif wrong == "mask_start_plus_one":
            lo = torch.minimum(dsi + 1, row)
        else:
            lo = dsi
        o = R(_attention(q, k, v, lo,
                         kv_roll=1 if wrong == "kv_head_rolled" else 0))
        a = R(o.reshape(B, S, Hq * D) @ p[pre + "attn.o_proj.weight"].t())
        xr2 = R(a + xr)
        h2 = R(_rms(xr2, p[pre + "post_attn_norm.weight"], eps))
        gu = R(h2 @ p[pre + "mlp.gate_up_proj.weight"].t())
        g, u = gu[..., :I], gu[..., I:]
        if wrong == "swiglu_halves_swapped":
            g, u = u, g
        act = R(torch.nn.functional.silu(g) * u)
        x, res = R(act @ p[pre + "mlp.down_proj.weight"].t()), xr2
    y = R(_rms(R(x + res), p["norm.weight"], eps))
    head = p["embed_tokens.weight"] if tied else p["lm_head.weight"]
    logits = R(y @ head.t())
    if wrong == "label_shift":
        labels = torch.roll(labels, -1, 1)
    loss = _mean_ce(logits, labels,
                    B * S - 1 if wrong == "mean_divisor_off" else B * S)
    out = _finish(logits, loss, p, storage)
    out["qk"] = qk
    return out


# --------------------------------------------------------------------------
# GPT-2
# --------------------------------------------------------------------------
def gpt2(state, cfg_dict, ids, labels, *, storage="fp64", wrong=None) -> dict:
    """state as GPT2Model.state_dict() gives it; learned positions, pre-LN
    blocks with biases, GELU-tanh, tied embeddings, causal MHA."""
    if wrong not in (None, "label_shift", "mean_divisor_off"):
        raise ValueError(f"gpt2 has no mutant {wrong!r}")
    c = cfg_dict
    tied = bool(c["tie_embeddings"])
    R = _storage(storage)
    p = _params(state, skip=("lm_head.weight",) if tied else ())
    ids = torch.as_tensor(ids).cpu().long()
    labels = torch.as_tensor(labels).cpu().long()
    B, S = ids.shape
    H, nh, hd, eps = c["hidden_size"], c["num_heads"], c["head_dim"], \
        c["ln_eps"]
    zero = torch.zeros(B, S, dtype=torch.long)

    def lin(t, name):
        return R(t @ p[name + ".weight"].t() + p[name + ".bias"])

    x = R(R(p["wte.weight"][ids]) + R(p["wpe.weight"][:S]))
    for i in range(c["num_layers"]):
        pre = f"blocks.{i}."
        h = R(_ln(x, p[pre + "ln_1.weight"], p[pre + "ln_1.bias"], eps))
        qkv = lin(h, pre + "qkv")
        q, k, v = (t.reshape(B, S, nh, hd) for t in qkv.split(H, -1))
        o = R(_attention(q, k, v, zero))
        x = R(x + lin(o.reshape(B, S, H), pre + "proj"))
        h2 = R(_ln(x, p[pre + "ln_2.weight"], p[pre + "ln_2.bias"], eps))
        x = R(x + lin(R(_gelu_tanh(lin(h2, pre + "fc"))), pre + "fc_out"))
    y = R(_ln(x, p["ln_f.weight"], p["ln_f.bias"], eps))
    head = p["wte.weight"] if tied else p["lm_head.weight"]
    logits = R(y @ head.t())
    if wrong == "label_shift":
        labels = torch.roll(labels, -1, 1)
    loss = _mean_ce(logits, labels,
                    B * S - 1 if wrong == "mean_divisor_off" else B * S)
    return _finish(logits, loss, p, storage)


# --------------------------------------------------------------------------
# The criterion
# --------------------------------------------------------------------------
def tensors(out: dict) -> dict:
    """logits, loss and every parameter gradient of a run, by name, fp64.
    `out` is an oracle result or {"logits", "loss", "grads"} of any run."""
    t = {"logits": f64(out["logits"]), "loss": f64(out["loss"]).reshape(1)}
    for n, g in out["grads"].items():
        t["grad:" + n] = f64(g)
    return t


def ratios(got: dict, ref: dict, emu: dict) -> dict:
    """name -> (r2, rmax) of `got` against the emulation's own error. All
    three are `tensors()` dicts; every tensor of `ref` must be present in
    `got`. A tensor the emulation reproduces exactly (e(emu) = 0) demands
    the same of `got`: its ratio is 0 or inf."""
    out = {}
    for n, r in ref.items():
        assert got[n].shape == r.shape == emu[n].shape, (n, got[n].shape,
                                                         r.shape)
        ex, ee = got[n] - r, emu[n] - r
        if not bool(torch.isfinite(ex).all()):
            out[n] = (float("inf"), float("inf"))
            continue

        def div(a, b):
            a, b = float(a), float(b)
            return a / b if b > 0 else (0.0 if a == 0 else float("inf"))
        out[n] = (div(ex.norm(), ee.norm()),
                  div(ex.abs().max(), ee.abs().max()))
    return out


def worst(rat: dict):
    """((r2, tensor), (rmax, tensor)) of a ratios() dict."""
    a = max(rat, key=lambda n: rat[n][0])
    b = max(rat, key=lambda n: rat[n][1])
    return (rat[a][0], a), (rat[b][1], b)


def report(case: str, rat: dict) -> str:
    (r2, n2), (rm, nm) = worst(rat)
    return (f"MODEL {case}: worst r2={r2:.3f} ({n2}) "
            f"worst rmax={rm:.3f} ({nm})")


def check(case: str, got: dict, ref: dict, emu: dict) -> dict:
    """Print the worst ratios (over all tensors, then over the
    multi-element ones), then fail on any tensor outside the criterion:
    r2 <= M and rmax <= M for every tensor, and M_TENSOR for every tensor of
    more than one element."""
    rat = ratios(got, ref, emu)
    print(report(case, rat))
    many = {n: r for n, r in rat.items() if ref[n].numel() > 1}
    print(report(case + "[numel>1]", many))
    bad = {n: r for n, r in rat.items() if not (r[0] <= M and r[1] <= M)}
    bad.update({n: r for n, r in many.items()
                if not (r[0] <= M_TENSOR and r[1] <= M_TENSOR)})
    assert not bad, f"{case}: outside M={M} / M_TENSOR={M_TENSOR}: {bad}"
    return rat

"""The oracle under test (CPU): kernel_oracle's fp64 references and its
comparison rule must accept the project's fp32 CPU paths (outputs rounded
to bf16 where the kernels round) with ZERO violations, and must reject
deliberately wrong references. The GPU files test_*_oracle_gpu.py hold the
HIP kernels to the same references and the same rule."""
import dataclasses

import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

EPS = 1e-5


def as_bf16(spec):
    """The CPU paths cast dw/db to the weight's dtype."""
    return dataclasses.replace(spec, bf16=True)


# ---- the project's CPU paths, as dicts of outputs ------------------------
def cpu_rmsnorm(x, w, dy, res=None, dxr=None, fused=False):
    xl = x.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    if fused:
        rl = res.clone().requires_grad_(True) if res is not None else None
        y, xr = ops.rmsnorm_residual(xl, rl, wl, EPS)
        invr = y.grad_fn.saved_tensors[2]
        if dxr is None:
            y.backward(dy)
        else:
            torch.autograd.backward([y, xr], [dy, dxr])
        out = {"y": y, "invr": invr, "dx": xl.grad, "dw": wl.grad, "xr": xr}
        if rl is not None:
            out["dres"] = rl.grad
        return out
    y = ops.rmsnorm(xl, wl, EPS)
    invr = y.grad_fn.saved_tensors[2]
    y.backward(dy)
    return {"y": y, "invr": invr, "dx": xl.grad, "dw": wl.grad}


def cpu_layernorm(x, w, b, dy):
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = ops.layernorm(xl, wl, bl, EPS)
    _, _, mu, rstd = y.grad_fn.saved_tensors
    y.backward(dy)
    return {"y": y, "mu": mu, "rstd": rstd, "dx": xl.grad, "dw": wl.grad,
            "db": bl.grad}


def cpu_ce(logits, labels, grad_out):
    ll = logits.clone().requires_grad_(True)
    loss = ops.cross_entropy(ll, labels)
    (loss * grad_out).backward()
    return {"loss": loss.reshape(1), "dlogits": ll.grad}


def cpu_swiglu(gu, dout):
    gl = gu.clone().requires_grad_(True)
    out = ops.swiglu(gl)
    out.backward(dout)
    return {"out": out, "dgu": gl.grad}


HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1,
          grad_scale=0.5)


# ---- the CPU paths pass ---------------------------------------------------
RMS_SHAPES = [(3, 64), (3, 768), (3, 2112), (3, 4160), (520, 64)]


@pytest.mark.parametrize("shape", RMS_SHAPES)
@pytest.mark.parametrize("mag", [1.0, 1e-3])
def test_rmsnorm_cpu_path_passes(shape, mag):
    x, dy = ko.bf(*shape, scale=mag, seed=1), ko.bf(*shape, seed=2)
    w = ko.bf(shape[1], seed=3)
    got = cpu_rmsnorm(x, w, dy)
    specs = ko.rmsnorm(x, w, EPS, dy)
    specs["dw"] = as_bf16(specs["dw"])
    ko.check_all(f"cpu.rmsnorm{shape}x{mag}", got, specs)


@pytest.mark.parametrize("shape", RMS_SHAPES)
@pytest.mark.parametrize("with_res", [True, False])
def test_rmsnorm_residual_cpu_path_passes(shape, with_res):
    x, dy, dxr = (ko.bf(*shape, seed=s) for s in (1, 2, 4))
    res = ko.bf(*shape, seed=5) if with_res else None
    w = ko.bf(shape[1], seed=3)
    got = cpu_rmsnorm(x, w, dy, res, dxr if with_res else None, fused=True)
    xr = got.pop("xr")
    if with_res:
        ko.check("cpu.rmsnorm_res.xr", xr, ko.residual_sum(x, res))
    else:
        assert torch.equal(xr, x)
    specs = ko.rmsnorm(xr, w, EPS, dy, dxr if with_res else None)
    specs["dw"] = as_bf16(specs["dw"])
    specs["dres"] = specs["dx"]
    ko.check_all(f"cpu.rmsnorm_res{shape}", got, specs)


LN_CASES = [(3, 768), (3, 1600), (3, 2056), (520, 64), (1, 768),
            ("offset", 100.0), ("offset", 200.0), "const"]


@pytest.mark.parametrize("case", LN_CASES, ids=str)
def test_layernorm_cpu_path_passes(case):
    x, w, b, dy = ko.ln_inputs(case)
    got = cpu_layernorm(x, w, b, dy)
    specs = ko.layernorm(x, w, b, EPS, dy)
    specs["dw"], specs["db"] = as_bf16(specs["dw"]), as_bf16(specs["db"])
    ko.check_all(f"cpu.layernorm[{case}]", got, specs)


def test_layernorm_one_pass_variance_is_rejected():
    """The defect this oracle was built to see: var = E[x^2] - mu^2 in fp32
    at offset 200, std 1 misses rstd by about a bf16 rounding."""
    x = ko.bf(3, 1024, offset=200.0, seed=1).float()
    mu = x.mean(-1)
    var = (x * x).mean(-1) - mu * mu
    rstd = torch.rsqrt(var.clamp_min(0) + EPS)
    specs = ko.layernorm(x, torch.ones(1024), torch.zeros(1024), EPS)
    assert ko.compare("rstd", rstd, specs["rstd"]).violations > 0
    two_pass = torch.rsqrt((x - mu[:, None]).pow(2).mean(-1) + EPS)
    assert ko.compare("rstd", two_pass, specs["rstd"]).violations == 0


@pytest.mark.parametrize("shape", [(70, 2056), (2, 16392)])
def test_cross_entropy_cpu_path_passes(shape):
    logits, labels = ko.ce_inputs(*shape)
    got = cpu_ce(logits, labels, 3.5)
    specs = ko.cross_entropy(logits, labels, 3.5)
    ko.check_all(f"cpu.ce{shape}", got, specs)


@pytest.mark.parametrize("B,S,H,D,rows", [(2, 37, 3, 64, 37), (2, 37, 3, 128, 37),
                                          (4, 1, 2, 128, 1), (2, 19, 2, 64, 38)])
def test_rope_cpu_path_passes(B, S, H, D, rows):
    cos, sin = ko.rope_table(rows, D)
    x, dy = ko.bf(B, S, H, D, seed=1), ko.bf(B, S, H, D, seed=2)
    xl = x.clone().requires_grad_(True)
    y = ops.apply_rope(xl, cos, sin)
    y.backward(dy)
    ko.check("cpu.rope.y", y, ko.rope(x, cos, sin, 1.0))
    ko.check("cpu.rope.dx", xl.grad, ko.rope(dy, cos, sin, -1.0))


@pytest.mark.parametrize("D", [64, 128])
def test_qkv_rope_cpu_path_passes(D):
    B, S, Hq, Hkv = 2, 21, 4, 2
    cos, sin = ko.rope_table(2 * S, D)      # longer table: first S rows count
    qkv = ko.bf(B, S, (Hq + 2 * Hkv) * D, seed=1)
    douts = [ko.bf(B, S, h, D, seed=s) for h, s in ((Hq, 2), (Hkv, 3), (Hkv, 4))]
    ql = qkv.clone().requires_grad_(True)
    q, k, v = ops.qkv_rope(ql, cos, sin, Hq, Hkv, D)
    torch.autograd.backward([q, k, v], douts)
    q_in, k_in, v_in = ko.qkv_split(qkv, Hq, Hkv, D)
    ko.check("cpu.qkv_rope.q", q, ko.rope(q_in, cos, sin))
    ko.check("cpu.qkv_rope.k", k, ko.rope(k_in, cos, sin))
    assert torch.equal(v, v_in)
    dq, dk, dv = ko.qkv_split(ql.grad, Hq, Hkv, D)
    ko.check("cpu.qkv_rope.dq", dq, ko.rope(douts[0], cos, sin, -1.0))
    ko.check("cpu.qkv_rope.dk", dk, ko.rope(douts[1], cos, sin, -1.0))
    assert torch.equal(dv, douts[2])


@pytest.mark.parametrize("rows,I", [(37, 128), (5, 2056)])
def test_swiglu_cpu_path_passes(rows, I):
    gu, dout = ko.swiglu_inputs(rows, I)
    ko.check_all(f"cpu.swiglu{rows}x{I}", cpu_swiglu(gu, dout),
                 ko.swiglu(gu, dout))


@pytest.mark.parametrize("n", [8, 4104])
@pytest.mark.parametrize("wd", [0.1, 8.0])
def test_adamw_cpu_path_passes(n, wd):
    hp = dict(HP, weight_decay=wd)
    p = ko.q16(0.02 * torch.randn(n, generator=torch.Generator().manual_seed(0)))
    g = ko.bf(n, seed=1)
    m, v = torch.zeros(n), torch.zeros(n)
    p0 = p.clone()
    for step in (1, 2, 3):
        specs = ko.adamw_step(p, g, m, v, step=step, **hp)
        ops.fused_adamw_(p, g, m, v, step=step, **hp)
        ko.check_all(f"cpu.adamw[n={n},wd={wd},t={step}]",
                     {"p": p, "m": m, "v": v}, specs)
    assert (p != p0).all()


@pytest.mark.parametrize("T", [1, 5, 8, 9, 100])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_cpu_path_passes(T, D):
    q, kc, vc = ko.decode_inputs(2, T, 8, 2, D)
    out = ops.attention_decode(q, kc, vc, T)
    assert torch.isfinite(out.float()).all()
    ko.check(f"cpu.decode[T={T},D={D}]", out,
             ko.attention_decode(q, kc, vc, T))


# ---- deliberately wrong references fail -----------------------------------
@pytest.mark.parametrize("H", [768, 2112, 4096])
@pytest.mark.parametrize("mutant", [dict(drop_last_vec=True),
                                    dict(divisor_off=8),
                                    dict(divisor_off=-8)], ids=str)
def test_norm_reduction_mutants_fail(H, mutant):
    x, dy, w, b = ko.bf(3, H, seed=1), ko.bf(3, H, seed=2), ko.bf(H, seed=3), ko.bf(H, seed=4)
    got = cpu_rmsnorm(x, w, dy)
    bad = ko.violates(got, ko.rmsnorm(x, w, EPS, dy, **mutant))
    assert "invr" in bad and "y" in bad, bad
    got = cpu_layernorm(x, w, b, dy)
    bad = ko.violates(got, ko.layernorm(x, w, b, EPS, dy, **mutant))
    assert "rstd" in bad and "y" in bad, bad


def test_eps_mutant_fails_on_small_rows():
    H = 768
    dy, w, b = ko.bf(3, H, seed=2), ko.bf(H, seed=3), ko.bf(H, seed=4)
    small = ko.bf(3, H, scale=1e-3, seed=1)
    got = cpu_rmsnorm(small, w, dy)
    bad = ko.violates(got, ko.rmsnorm(small, w, EPS, dy, no_eps=True))
    assert {"invr", "y", "dx"} <= set(bad), bad
    got = cpu_layernorm(small, w, b, dy)
    bad = ko.violates(got, ko.layernorm(small, w, b, EPS, dy, no_eps=True))
    assert {"rstd", "y", "dx"} <= set(bad), bad


def test_cross_entropy_mutants_fail():
    logits, labels = ko.ce_inputs(70, 2056)
    got = cpu_ce(logits, labels, 3.5)
    for mutant in (dict(label_shift=1), dict(label_shift=-1),
                   dict(drop_last_vec=True), dict(divisor_off=1)):
        bad = ko.violates(got, ko.cross_entropy(logits, labels, 3.5, **mutant))
        assert bad == ["loss", "dlogits"], (mutant, bad)


def test_rope_mutants_fail():
    B, S, H, D = 2, 37, 3, 64
    cos, sin = ko.rope_table(S, D)
    x = ko.bf(B, S, H, D, seed=1)
    y = ops.apply_rope(x, cos, sin)
    for mutant in (dict(pos_shift=1), dict(pos_shift=-1),
                   dict(swap_halves=True)):
        assert ko.compare("y", y, ko.rope(x, cos, sin, **mutant)).violations, \
            mutant
    # inverse rotation instead of forward
    assert ko.compare("y", y, ko.rope(x, cos, sin, -1.0)).violations


def test_adamw_without_weight_decay_fails():
    n = 4104
    hp = dict(HP, weight_decay=8.0)
    p = ko.q16(0.02 * torch.randn(n, generator=torch.Generator().manual_seed(0)))
    g, m, v = ko.bf(n, seed=1), torch.zeros(n), torch.zeros(n)
    wrong = ko.adamw_step(p, g, m, v, step=1, no_weight_decay=True, **hp)
    ops.fused_adamw_(p, g, m, v, step=1, **hp)
    assert ko.violates({"p": p, "m": m, "v": v}, wrong) == ["p"]


def test_decode_wrong_kv_head_fails():
    q, kc, vc = ko.decode_inputs(2, 9, 8, 2, 64)
    out = ops.attention_decode(q, kc, vc, 9)
    wrong = ko.attention_decode(q, kc, vc, 9, kv_head_shift=1)
    assert ko.compare("out", out, wrong).violations


def test_rule_rejects_nan_and_untouched_output():
    spec = ko.Spec(torch.ones(4, dtype=torch.float64),
                   torch.ones(4, dtype=torch.float64), 8, True)
    assert ko.compare("x", torch.ones(4), spec).violations == 0
    assert ko.compare("x", torch.tensor([1, 1, float("nan"), 1.0]),
                      spec).violations == 1
    assert ko.compare("x", torch.tensor([1, 1.0079, 1, 1.0]),
                      spec).violations == 1          # one bf16 ulp off
    assert ko.compare("x", torch.tensor([1, 1.0039, 1, 1.0]),
                      spec).violations == 0          # half an ulp

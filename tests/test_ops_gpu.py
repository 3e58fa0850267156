"""GPU numerics tests: gfx950 HIP kernels vs plain PyTorch fp32 references.

Every test here compares the handwritten kernel against the fp32 CPU/eager
reference of the same op (tolerances account for bf16 I/O).
"""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def test_hip_ext_loaded():
    # on a GPU box the native extension must be present - no silent fallback
    assert ops.hip_ext_available(), "gfx950 extension not built/loaded"


def test_mfma_16x16x32_layout():
    """Transpose-detecting probe: asymmetric A and B (guide §5.4 r16)."""
    torch.manual_seed(0)
    A = (torch.randn(16, 32) * 0.5).bfloat16().to(dev())
    B = (torch.randn(32, 16) * 0.5).bfloat16().to(dev())
    D = ops._C.mfma_probe(A, B)
    ref = A.float().cpu() @ B.float().cpu()
    err = (D.cpu() - ref).abs().max().item()
    assert err < 1e-2, f"MFMA layout mismatch, max err {err}\nD={D.cpu()}\nref={ref}"


def test_mfma_32x32x16_layout():
    torch.manual_seed(1)
    A = (torch.randn(32, 16) * 0.5).bfloat16().to(dev())
    B = (torch.randn(16, 32) * 0.5).bfloat16().to(dev())
    D = ops._C.mfma_probe(A, B)
    ref = A.float().cpu() @ B.float().cpu()
    err = (D.cpu() - ref).abs().max().item()
    assert err < 1e-2, f"32x32x16 layout mismatch, max err {err}"


@pytest.mark.parametrize("shape", [(32, 256), (1024, 4096), (33, 1024)])
def test_rmsnorm_fwd_bwd(shape):
    torch.manual_seed(0)
    # quantize inputs to bf16 FIRST so the fp32 reference sees the same
    # values as the kernel (isolates kernel math error from input rounding)
    x = torch.randn(shape).bfloat16().float()
    w = torch.randn(shape[-1]).bfloat16().float()
    dy = torch.randn(shape).bfloat16().float()

    # fp32 CPU reference with autograd
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    yr = ops.rmsnorm(xr, wr, 1e-5)
    yr.backward(dy)

    xg = x.bfloat16().to(dev()).requires_grad_(True)
    wg = w.bfloat16().to(dev()).requires_grad_(True)
    yg = ops.rmsnorm(xg, wg, 1e-5)
    yg.backward(dy.bfloat16().to(dev()))

    assert (yg.float().cpu() - yr.detach()).abs().max() < 0.05
    assert (xg.grad.float().cpu() - xr.grad).abs().max() < 0.05
    # dw accumulates over rows - compare relative
    dw_err = (wg.grad.float().cpu() - wr.grad).abs().max()
    assert dw_err < 0.05 * max(1.0, wr.grad.abs().max().item())


def test_rope_fwd_bwd():
    from torch_on_k8s_amd.models.llama import build_rope_table, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-tiny", head_dim=128)
    B, S, H, D = 2, 64, 4, 128
    cos, sin = build_rope_table(cfg, S, dev())
    x = torch.randn(B, S, H, D)
    dy = torch.randn(B, S, H, D)

    y_ref = ops.rope_ref(x, cos.cpu(), sin.cpu(), 1.0)
    dx_ref = ops.rope_ref(dy, cos.cpu(), sin.cpu(), -1.0)

    xg = x.bfloat16().to(dev()).requires_grad_(True)
    yg = ops.apply_rope(xg, cos, sin)
    yg.backward(dy.bfloat16().to(dev()))

    assert (yg.float().cpu() - y_ref.float()).abs().max() < 0.03
    assert (xg.grad.float().cpu() - dx_ref.float()).abs().max() < 0.03


def _adamw_steps_vs_fp64(n, weight_decay, steps=3, tail=0):
    """Every step is judged on its own, from the state the kernel left:
    p (bf16) by the bf16 rule, m and v (fp32) by the fp32 rule of
    kernel_oracle.py. A trajectory compared only at its end would have to
    forgive a whole bf16 ulp wherever one rounding fell the other way."""
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8,
              weight_decay=weight_decay, grad_scale=0.5)
    gen = torch.Generator().manual_seed(0)
    p0 = ko.q16(0.02 * torch.randn(n, generator=gen))
    g = ko.q16(torch.randn(n, generator=gen))
    pg, gg = p0.to(dev()), g.to(dev())
    mg = torch.zeros(n, device=dev())
    vg = torch.zeros(n, device=dev())
    for step in range(1, steps + 1):
        specs = ko.adamw_step(pg, g, mg, vg, step=step, **hp)
        before = pg.clone()
        ops.fused_adamw_(pg, gg, mg, vg, step=step, **hp)
        got = {"p": pg, "m": mg, "v": vg}
        tag = f"adamw[n={n},wd={weight_decay},t={step}]"
        ko.check_all(tag, got, specs)
        if tail:  # the elements only a later grid sweep reaches
            ko.check_all(tag + ".tail", {k: t[-tail:] for k, t in got.items()},
                         {k: ko.Spec(s.ref[-tail:], s.scale[-tail:], s.k,
                                     s.bf16) for k, s in specs.items()})
            assert (pg[-tail:] != before[-tail:]).all()
        # a kernel that never writes p must not pass
        assert (pg != before).all(), "some p elements did not move"
    assert (pg.cpu() != p0).all()
    assert (mg != 0).all() and (vg > 0).all()


def test_fused_adamw_vs_reference():
    # wd = 0.1 is the trainer's; at wd = 8, lr*wd exceeds a bf16 half ulp,
    # so a kernel without the decay term cannot pass either
    _adamw_steps_vs_fp64(4096 + 8, 0.1)
    _adamw_steps_vs_fp64(4096 + 8, 8.0)


def test_fused_adamw_single_vector():
    _adamw_steps_vs_fp64(8, 0.1)


def test_fused_adamw_second_grid_sweep():
    """2048 blocks x 256 threads x 8 elements = 4,194,304 per sweep; the
    8000 elements beyond exist only for the stride loop."""
    _adamw_steps_vs_fp64(4_194_304 + 8000, 0.1, tail=8000)


def test_fused_cross_entropy():
    torch.manual_seed(0)
    N, V = 64, 1024
    logits = (torch.randn(N, V) * 2).bfloat16().float()
    labels = torch.randint(0, V, (N,))

    lr = logits.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, labels)
    ref.backward()

    lg = logits.bfloat16().to(dev()).requires_grad_(True)
    loss = ops.cross_entropy(lg, labels.to(dev()))
    loss.backward()

    assert abs(loss.item() - ref.item()) < 2e-3
    gerr = (lg.grad.float().cpu() - lr.grad).abs().max().item()
    assert gerr < 1e-3, f"CE grad err {gerr}"


def test_trainer_single_gpu_step():
    """End-to-end: tiny Llama fwd+bwd+fused AdamW on GPU, loss finite and
    decreasing on a fixed batch."""
    from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
    from torch_on_k8s_amd.parallel.env import DistContext
    torch.manual_seed(0)
    ctx = DistContext(device=dev())
    cfg = TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=128,
                        lr=1e-3)  # default attn_impl="hip": the fused
    # flash-attention kernel is the path under test
    tr = Trainer(cfg, ctx)
    losses = []
    for _ in range(6):
        tr.step_count = 0
        losses.append(tr.train_step())
        tr.step_count = 1
    assert all(l == l for l in losses)
    assert losses[-1] < losses[0], losses


def test_layernorm_gpu():
    torch.manual_seed(0)
    x = torch.randn(256, 1024).bfloat16().float()
    w = torch.randn(1024).bfloat16().float()
    b = torch.randn(1024).bfloat16().float()
    dy = torch.randn(256, 1024).bfloat16().float()

    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (1024,), wr, br, 1e-5)
    yr.backward(dy)

    xg = x.bfloat16().to(dev()).requires_grad_(True)
    wg = w.bfloat16().to(dev()).requires_grad_(True)
    bg = b.bfloat16().to(dev()).requires_grad_(True)
    yg = ops.layernorm(xg, wg, bg, 1e-5)
    yg.backward(dy.bfloat16().to(dev()))

    assert (yg.float().cpu() - yr.detach()).abs().max() < 0.05
    assert (xg.grad.float().cpu() - xr.grad).abs().max() < 0.05
    assert (wg.grad.float().cpu() - wr.grad).abs().max() < \
        0.05 * max(1.0, wr.grad.abs().max().item())
    assert (bg.grad.float().cpu() - br.grad).abs().max() < \
        0.05 * max(1.0, br.grad.abs().max().item())


def test_gpt2_trainer_gpu_step():
    from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
    from torch_on_k8s_amd.parallel.env import DistContext
    torch.manual_seed(0)
    tr = Trainer(TrainerConfig(model="gpt2-tiny", micro_batch=2, seq_len=128,
                               lr=1e-3), DistContext(device=dev()))
    losses = []
    for _ in range(5):
        tr.step_count = 0
        losses.append(tr.train_step())
        tr.step_count = 1
    assert all(l == l for l in losses)
    assert losses[-1] < losses[0], losses


def test_native_extension_is_in_tree():
    """The gfx950 extension must be the in-tree build (not a site-packages
    or JIT-cache copy) so repo snapshots carry the exact code under test."""
    import os
    import torch_on_k8s_amd
    pkg_root = os.path.dirname(os.path.dirname(
        os.path.abspath(torch_on_k8s_amd.__file__)))
    assert ops._C.__file__.startswith(pkg_root), ops._C.__file__
    assert "site-packages" not in ops._C.__file__


def test_swiglu_fwd_bwd():
    """Fused SwiGLU over packed gate_up vs fp32 reference."""
    torch.manual_seed(0)
    rows, I = 1024, 1024
    gu = torch.randn(rows, 2 * I).bfloat16().float()
    dout = torch.randn(rows, I).bfloat16().float()

    ref_gu = gu.clone().requires_grad_(True)
    ref = ops.swiglu_ref(ref_gu.bfloat16()).float()
    # fp32 manual backward
    g, u = gu.split(I, dim=-1)
    sg = torch.sigmoid(g)
    dg_ref = dout * u * (sg * (1 + g * (1 - sg)))
    du_ref = dout * (g * sg)

    gug = gu.bfloat16().to(dev()).requires_grad_(True)
    out = ops.swiglu(gug)
    out.backward(dout.bfloat16().to(dev()))
    # bf16 output rounding scales with magnitude (|dg| can reach ~10 for
    # products of three ~N(0,1) terms): bound RELATIVE to the max ref
    def tol(ref_t):
        return max(3e-2, 2.5 / 256 * ref_t.abs().max().item())

    err_f = (out.float().cpu() - ref).abs().max().item()
    dgu = gug.grad.float().cpu()
    err_g = (dgu[:, :I] - dg_ref).abs().max().item()
    err_u = (dgu[:, I:] - du_ref).abs().max().item()
    assert err_f < tol(ref), f"swiglu fwd err {err_f}"
    assert err_g < tol(dg_ref), f"swiglu dgate err {err_g}"
    assert err_u < tol(du_ref), f"swiglu dup err {err_u}"


def test_qkv_rope_fwd_bwd():
    """Packed-QKV split+rope kernel vs the fp32 reference path."""
    torch.manual_seed(0)
    B, S, Hq, Hkv, D = 2, 128, 8, 4, 128
    from torch_on_k8s_amd.models.llama import build_rope_table, get_config
    cfg = get_config("llama-tiny", head_dim=D)
    cos, sin = build_rope_table(cfg, S, torch.device("cpu"))
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D).bfloat16().float()
    dq = torch.randn(B, S, Hq, D).bfloat16().float()
    dk = torch.randn(B, S, Hkv, D).bfloat16().float()
    dv = torch.randn(B, S, Hkv, D).bfloat16().float()

    q_ref, k_ref, v_ref = ops.qkv_rope_ref(qkv, cos, sin, Hq, Hkv, D)

    qkv_g = qkv.bfloat16().to(dev()).requires_grad_(True)
    q, k, v = ops.qkv_rope(qkv_g, cos.to(dev()), sin.to(dev()), Hq, Hkv, D)
    for got, ref, name in [(q, q_ref, "q"), (k, k_ref, "k"), (v, v_ref, "v")]:
        err = (got.float().cpu() - ref.float()).abs().max().item()
        assert err < 2e-2, f"qkv_rope {name} err {err}"
    torch.autograd.backward([q, k, v], [dq.bfloat16().to(dev()),
                                        dk.bfloat16().to(dev()),
                                        dv.bfloat16().to(dev())])
    # reference backward: inverse-rotate dq/dk, concat with dv
    dq_r = ops.rope_ref(dq, cos, sin, -1.0).reshape(B, S, Hq * D)
    dk_r = ops.rope_ref(dk, cos, sin, -1.0).reshape(B, S, Hkv * D)
    dqkv_ref = torch.cat([dq_r, dk_r, dv.reshape(B, S, Hkv * D)], dim=-1)
    err = (qkv_g.grad.float().cpu() - dqkv_ref.float()).abs().max().item()
    assert err < 2e-2, f"qkv_rope bwd err {err}"


def test_rmsnorm_dw_two_stage_large():
    """dw over many rows (the two-stage reduction path) matches fp32."""
    torch.manual_seed(3)
    rows, H = 16384, 4096
    x = torch.randn(rows, H).bfloat16().float()
    dy = torch.randn(rows, H).bfloat16().float()
    w = torch.ones(H).bfloat16().float()
    xg = x.bfloat16().to(dev()).requires_grad_(True)
    y = ops.rmsnorm(xg, w.bfloat16().to(dev()), 1e-5)
    y.backward(dy.bfloat16().to(dev()))
    # fp32 reference dw
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5)
    dw_ref = (dy * x * r).sum(0)
    # kernel dw is on the weight's grad — recompute through the module path
    wp = w.bfloat16().to(dev()).requires_grad_(True)
    xg2 = x.bfloat16().to(dev())
    y2 = ops.rmsnorm(xg2, wp, 1e-5)
    y2.backward(dy.bfloat16().to(dev()))
    rel = ((wp.grad.float().cpu() - dw_ref).abs() /
           (dw_ref.abs() + 1.0)).max().item()
    assert rel < 2e-2, f"rmsnorm dw two-stage rel err {rel}"


def test_rmsnorm_residual_fused():
    """Fused residual+RMSNorm (fwd: y, xr; bwd: dx includes dxr addend)
    vs the unfused fp32 reference."""
    torch.manual_seed(5)
    rows, H = 512, 1024
    x = torch.randn(rows, H).bfloat16().float()
    res = torch.randn(rows, H).bfloat16().float()
    w = torch.randn(H).bfloat16().float()
    dy = torch.randn(rows, H).bfloat16().float()
    dxr_in = torch.randn(rows, H).bfloat16().float()

    xg = x.bfloat16().to(dev()).requires_grad_(True)
    rg = res.bfloat16().to(dev()).requires_grad_(True)
    wg = w.bfloat16().to(dev()).requires_grad_(True)
    y, xr = ops.rmsnorm_residual(xg, rg, wg, 1e-5)
    torch.autograd.backward([y, xr], [dy.bfloat16().to(dev()),
                                      dxr_in.bfloat16().to(dev())])

    # fp32 reference (with the bf16 residual-sum rounding the kernel does)
    xr_ref = (x + res)
    xr_q = xr_ref.to(torch.bfloat16).float()
    r = torch.rsqrt(xr_q.pow(2).mean(-1, keepdim=True) + 1e-5)
    y_ref = xr_q * r * w
    c = (dy * w * xr_q).sum(-1, keepdim=True)
    dx_ref = r * (w * dy - xr_q * (r * r / H) * c) + dxr_in
    dw_ref = (dy * xr_q * r).sum(0)

    def tol(ref_t):  # bf16 output rounding scales with magnitude
        return max(3e-2, 2.5 / 256 * ref_t.abs().max().item())

    err_y = (y.float().cpu() - y_ref).abs().max().item()
    err_xr = (xr.float().cpu() - xr_q).abs().max().item()
    err_dx = (xg.grad.float().cpu() - dx_ref).abs().max().item()
    err_dr = (rg.grad.float().cpu() - dx_ref).abs().max().item()
    assert err_y < tol(y_ref), f"y err {err_y}"
    assert err_xr < 2e-2, f"xr err {err_xr}"
    assert err_dx < tol(dx_ref), f"dx err {err_dx}"
    assert err_dr < tol(dx_ref), f"dres err {err_dr}"
    rel = ((wg.grad.float().cpu() - dw_ref).abs() /
           (dw_ref.abs() + 1.0)).max().item()
    assert rel < 3e-2, f"dw rel err {rel}"


def test_llama_tiny_fused_block_matches_cpu():
    """End-to-end: the tiny model's LOSS on the GPU (all fused kernels)
    matches the CPU fp32 path within 0.05. The loss only: no gradient is
    looked at here. Logits, loss and every parameter gradient of the HIP
    path are held to an independent fp64 model in
    test_model_oracle_gpu.py."""
    from torch_on_k8s_amd.models.llama import LlamaModel, get_config
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    m_cpu = LlamaModel(cfg)
    m_gpu = LlamaModel(cfg).to(dev()).bfloat16()
    m_gpu.load_state_dict({k: v.bfloat16()
                           for k, v in m_cpu.state_dict().items()})
    ids = torch.randint(0, cfg.vocab_size, (2, 64))
    l_cpu = m_cpu(ids, ids)
    l_gpu = m_gpu(ids.to(dev()), ids.to(dev()))
    assert abs(l_cpu.item() - l_gpu.float().item()) < 0.05, \
        (l_cpu.item(), l_gpu.float().item())

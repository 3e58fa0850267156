"""MI355X-native fused ops.

Dispatch policy:
  * GPU tensors ALWAYS run the handwritten gfx950 HIP kernels from the
    in-tree extension ``torch_on_k8s_amd.ops._C``. If the extension is
    missing on a GPU machine, ops raise instead of silently falling back
    to eager PyTorch.
  * CPU tensors use plain fp32 PyTorch reference implementations (used by
    the CPU test suite and as the numerics oracle for the HIP kernels).

Capability parity: the reference (hliangzhao/torch-on-k8s) ships no
kernels at all -- it schedules opaque containers. These ops
are the data plane its env-var contract assumes exists inside the
container, built MI355X-first per SURVEY.md §7 step 2.
"""
from __future__ import annotations

import os

import torch

try:  # the in-tree gfx950 extension; built by `setup.py build_ext --inplace`
    from . import _C  # type: ignore
except ImportError:  # pragma: no cover - exercised only on unbuilt checkouts
    _C = None


def hip_ext_available() -> bool:
    return _C is not None


def _require_ext(op: str):
    if _C is None:
        raise RuntimeError(
            f"torch_on_k8s_amd HIP extension is required for {op} on GPU but "
            "is not built. Run: PYTORCH_ROCM_ARCH=gfx950 python setup.py "
            "build_ext --inplace"
        )
    return _C


def _wide(t: torch.Tensor) -> torch.Tensor:
    """The type the CPU reference paths compute in: fp32 for bf16, fp16 and
    fp32 inputs, and fp64 for fp64 inputs, which are never narrowed (a
    .double() model on the CPU path is then the model in fp64, which is what
    tests/model_oracle.py is held against)."""
    return t if t.dtype == torch.float64 else t.float()


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------
def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """fp32 reference: y = x * w / sqrt(mean(x^2) + eps)."""
    xf = _wide(x)
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * r * _wide(w)).to(x.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        if x.is_cuda:
            y, invr = _require_ext("rmsnorm").rmsnorm_fwd(x, w, eps)
        else:
            xf = _wide(x)
            invr = torch.rsqrt(xf.pow(2).mean(-1) + eps).reshape(-1)
            y = (xf * invr.view(*x.shape[:-1], 1) * _wide(w)).to(x.dtype)
        ctx.save_for_backward(x, w, invr)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, invr = ctx.saved_tensors
        dy = dy.contiguous()
        if x.is_cuda:
            dx, dw = _C.rmsnorm_bwd(x, w, dy, invr)
        else:
            xf, wf, dyf = _wide(x), _wide(w), _wide(dy)
            H = x.shape[-1]
            r = invr.view(*x.shape[:-1], 1)
            c = (dyf * wf * xf).sum(-1, keepdim=True)
            dx = (r * (wf * dyf - xf * (r * r / H) * c)).to(x.dtype)
            dw = (dyf * xf * r).reshape(-1, H).sum(0)
        return dx, dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNormFn.apply(x.contiguous(), w, eps)


class _RMSNormResFn(torch.autograd.Function):
    """Fused residual-add + RMSNorm: (x, res, w) -> (y, xr) with
    xr = x + res (bf16) and y = rmsnorm(xr) * w. Backward fuses the
    downstream residual grad (dxr) into the norm's dx pass, and dres
    equals dx (the add routes gradients unchanged)."""

    @staticmethod
    def forward(ctx, x, res, w, eps):
        if x.is_cuda:
            y, xr, invr = _require_ext("rmsnorm_res").rmsnorm_res_fwd(
                x, res, w, eps)
        else:
            xr = x + res if res is not None else x
            xf = _wide(xr)
            invr = torch.rsqrt(xf.pow(2).mean(-1) + eps).reshape(-1)
            y = (xf * invr.view(*xr.shape[:-1], 1) * _wide(w)).to(x.dtype)
        ctx.save_for_backward(xr, w, invr)
        ctx.has_res = res is not None
        # an output nobody used (the final norm's xr) arrives in backward
        # as None, not as a zero tensor to fill, read and add
        ctx.set_materialize_grads(False)
        return y, xr

    @staticmethod
    def backward(ctx, dy, dxr):
        xr, w, invr = ctx.saved_tensors
        if dy is None:      # only xr was used: the norm itself had no reader
            dy = torch.zeros_like(xr)
        dy = dy.contiguous()
        if dxr is not None:
            dxr = dxr.contiguous()
        if xr.is_cuda:
            dx, dw = _C.rmsnorm_res_bwd(xr, w, dy, dxr, invr)
        else:
            xf, wf, dyf = _wide(xr), _wide(w), _wide(dy)
            H = xr.shape[-1]
            r = invr.view(*xr.shape[:-1], 1)
            c = (dyf * wf * xf).sum(-1, keepdim=True)
            dx = r * (wf * dyf - xf * (r * r / H) * c)
            if dxr is not None:  # added in fp32, one rounding, as the kernel
                dx = dx + _wide(dxr)
            dx = dx.to(xr.dtype)
            dw = (dyf * xf * r).reshape(-1, H).sum(0)
        dres = dx if ctx.has_res else None
        return dx, dres, dw.to(w.dtype), None


def rmsnorm_residual(x: torch.Tensor, res: torch.Tensor | None,
                     w: torch.Tensor, eps: float = 1e-5):
    """Returns (normed, x+res). One pass instead of add + norm; the
    residual stream stays fused through backward too."""
    return _RMSNormResFn.apply(
        x.contiguous(), res.contiguous() if res is not None else None, w, eps)


# --------------------------------------------------------------------------
# RoPE (Llama rotate-half convention)
# --------------------------------------------------------------------------
def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             sign: float = 1.0,
             doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """x: [B, S, H, D]; cos/sin: [>= S, D/2] fp32, row s = position s, or
    position s - doc_start[b, s] with packed-document bounds."""
    B, S, H, D = x.shape
    if cos.shape[0] < S or sin.shape[0] < S:
        raise ValueError(
            f"rope table has {cos.shape[0]} rows, sequence needs {S}")
    xf = _wide(x)
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    if doc_start is None:
        cs = cos[:S].reshape(1, S, 1, D // 2)
        sn = sin[:S].reshape(1, S, 1, D // 2) * sign
    else:
        pos = (torch.arange(S, device=x.device).unsqueeze(0)
               - doc_start.long())
        cs = cos[pos].reshape(B, S, 1, D // 2)
        sn = sin[pos].reshape(B, S, 1, D // 2) * sign
    return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], dim=-1).to(x.dtype)


class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        ctx.heads = x.shape[2]
        if x.is_cuda:
            return _require_ext("rope").rope(x.contiguous(), cos, sin, x.shape[2], 1.0)
        return rope_ref(x, cos, sin, 1.0)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        if dy.is_cuda:
            dx = _C.rope(dy.contiguous(), cos, sin, ctx.heads, -1.0)
        else:
            dx = rope_ref(dy, cos, sin, -1.0)
        return dx, None, None


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Apply rotary embedding to [B, S, H, D] activations."""
    return _RopeFn.apply(x, cos, sin)


# --------------------------------------------------------------------------
# Packed-QKV split + RoPE (one pass over the fused qkv projection output)
# --------------------------------------------------------------------------
def qkv_rope_ref(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 Hq: int, Hkv: int, D: int, sign: float = 1.0,
                 doc_start: torch.Tensor | None = None):
    """fp32 reference. qkv: [B, S, (Hq+2Hkv)*D]; returns roped q, k and
    copied v with contiguous [B,S,H,D] layouts."""
    B, S, _ = qkv.shape
    if doc_start is not None:
        validate_doc_bounds(doc_start, None, B, S)
    parts = qkv.view(B, S, Hq + 2 * Hkv, D)
    q = parts[:, :, :Hq].contiguous()
    k = parts[:, :, Hq:Hq + Hkv].contiguous()
    v = parts[:, :, Hq + Hkv:].contiguous()
    return (rope_ref(q, cos, sin, sign, doc_start),
            rope_ref(k, cos, sin, sign, doc_start), v)


class _QKVRopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, Hq, Hkv, D, doc_start=None):
        ctx.dims = (Hq, Hkv, D)
        ctx.docs = doc_start is not None
        if ctx.docs:
            ctx.save_for_backward(cos, sin, doc_start)
        else:
            ctx.save_for_backward(cos, sin)
        if qkv.is_cuda:
            ext = _require_ext("qkv_rope")
            if ctx.docs:
                q, k, v = ext.qkv_rope_fwd(qkv.contiguous(), cos, sin, Hq,
                                           Hkv, D, doc_start)
            else:
                q, k, v = ext.qkv_rope_fwd(qkv.contiguous(), cos, sin, Hq,
                                           Hkv, D)
            return q, k, v
        return qkv_rope_ref(qkv, cos, sin, Hq, Hkv, D, 1.0, doc_start)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        saved = ctx.saved_tensors   # read once (activation checkpointing)
        cos, sin = saved[:2]
        ds = saved[2] if ctx.docs else None
        Hq, Hkv, D = ctx.dims
        if dq.is_cuda:
            if ctx.docs:
                dqkv = _C.qkv_rope_bwd(dq.contiguous(), dk.contiguous(),
                                       dv.contiguous(), cos, sin, ds)
            else:
                dqkv = _C.qkv_rope_bwd(dq.contiguous(), dk.contiguous(),
                                       dv.contiguous(), cos, sin)
        else:
            B, S = dq.shape[:2]
            dqf = rope_ref(dq, cos, sin, -1.0, ds).view(B, S, Hq * D)
            dkf = rope_ref(dk, cos, sin, -1.0, ds).view(B, S, Hkv * D)
            dqkv = torch.cat([dqf, dkf, dv.reshape(B, S, Hkv * D)], dim=-1)
        return dqkv, None, None, None, None, None, None


def qkv_rope(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             Hq: int, Hkv: int, D: int,
             doc_start: torch.Tensor | None = None):
    """Split the packed qkv projection [B,S,(Hq+2Hkv)*D] into contiguous
    q/k/v with RoPE applied to q and k — one kernel instead of three
    splits + two rope launches (GEMM-packing lever, ROADMAP §1a). With
    packed-document bounds (doc_bounds) a token's position is counted from
    the first token of its document."""
    if doc_start is None:
        return _QKVRopeFn.apply(qkv, cos, sin, Hq, Hkv, D)
    return _QKVRopeFn.apply(qkv, cos, sin, Hq, Hkv, D,
                            _doc_tensor(doc_start, qkv, "doc_start"))


# --------------------------------------------------------------------------
# Fused SwiGLU over the packed gate_up projection
# --------------------------------------------------------------------------
def swiglu_ref(gu: torch.Tensor) -> torch.Tensor:
    """fp32 reference: silu(gate) * up over packed [..., 2I]."""
    I = gu.shape[-1] // 2
    g, u = _wide(gu).split(I, dim=-1)
    return (torch.nn.functional.silu(g) * u).to(gu.dtype)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        if gu.is_cuda:
            return _require_ext("swiglu").swiglu_fwd(gu.contiguous())
        return swiglu_ref(gu)

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        if gu.is_cuda:
            return _C.swiglu_bwd(dout.contiguous(), gu)
        I = gu.shape[-1] // 2
        g, u = _wide(gu).split(I, dim=-1)
        sg = torch.sigmoid(g)
        silu = g * sg
        dsilu = sg * (1 + g * (1 - sg))
        df = _wide(dout)
        return torch.cat([df * u * dsilu, df * silu], dim=-1).to(gu.dtype)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    """silu(gate)*up over the PACKED gate_up output [..., 2I]; fwd+bwd
    each one fused pass (no materialized silu intermediate)."""
    return _SwiGLUFn.apply(gu)


# --------------------------------------------------------------------------
# Fused AdamW on a flat bucket
# --------------------------------------------------------------------------
def fused_adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                 v: torch.Tensor, *, lr: float, beta1: float, beta2: float,
                 eps: float, weight_decay: float, step: int,
                 grad_scale: float = 1.0,
                 step_dev: torch.Tensor | None = None,
                 lr_dev: torch.Tensor | None = None,
                 gscale_dev: torch.Tensor | None = None) -> None:
    """In-place AdamW over one flat bucket (p/g bf16, m/v fp32).

    step_dev: optional int32 device scalar overriding `step` — used under
    hipGraph replay, where host-side scalars are frozen into the graph.
    lr_dev / gscale_dev: optional fp32 device scalars overriding `lr` and
    `grad_scale` the same way (scheduled LR; clip coefficient computed by
    grad_norm_finalize_ without a host sync).
    """
    if p.is_cuda:
        _require_ext("fused_adamw").adamw_(p, g, m, v, lr, beta1, beta2, eps,
                                           weight_decay, step, grad_scale,
                                           step_dev, lr_dev=lr_dev,
                                           gscale_dev=gscale_dev)
        return
    if lr_dev is not None:
        lr = float(lr_dev.reshape(-1)[0])
    if gscale_dev is not None:
        grad_scale = float(gscale_dev.reshape(-1)[0])
    gf = g.float() * grad_scale
    pf = p.float()
    pf -= lr * weight_decay * pf
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1.0 / (1.0 - beta1 ** step)
    bc2 = 1.0 / (1.0 - beta2 ** step)
    pf -= lr * (m * bc1) / ((v * bc2).sqrt() + eps)
    p.copy_(pf.to(p.dtype))


# --------------------------------------------------------------------------
# Global grad norm + clip coefficient, on device (no host sync, capturable)
# --------------------------------------------------------------------------
_SUMSQ_BLOCK_ELEMS = 256 * 8   # one bf16x8 vector per thread per sweep
_SUMSQ_MAX_BLOCKS = 2048       # grid cap, as the AdamW kernel


def grad_sumsq_blocks(n: int) -> int:
    """Partial slots (= blocks) grad_sumsq_ uses for a bucket of n
    elements. Depends on n alone, so a bucket's launch geometry — and with
    it the order of every addition — is the same on every step."""
    return max(1, min(_SUMSQ_MAX_BLOCKS, -(-n // _SUMSQ_BLOCK_ELEMS)))


@torch.no_grad()
def grad_sumsq_(g: torch.Tensor, partials: torch.Tensor) -> None:
    """Sum of squares of a flat bucket, as per-block fp32 partials.

    Writes EVERY slot of `partials` (1-D fp32, grad_sumsq_blocks(n) slots,
    caller-owned); their sum is sum(g^2). How the sum is split over the
    slots is unspecified. g.numel() must be a multiple of 8. Allocates
    nothing on GPU and never syncs; no atomics, so repeatable bit for bit.
    """
    if g.is_cuda:
        _require_ext("grad_sumsq").grad_sumsq_(g, partials)
        return
    assert g.numel() % 8 == 0, "bucket size must be a multiple of 8"
    partials.zero_()
    partials[0] = g.float().pow(2).sum()


@torch.no_grad()
def grad_norm_finalize_(partials: torch.Tensor, out: torch.Tensor, *,
                        inv_count: float, clip: float) -> None:
    """Fold all buckets' partials into two fp32 scalars:

        out[0] = norm   = sqrt(sum(partials)) * inv_count
        out[1] = gscale = inv_count * min(1, clip / (norm + 1e-6))

    inv_count is 1/(world*accum); clip <= 0 means no clipping (gscale =
    inv_count). A non-finite norm propagates into gscale, as on the host
    path. `out` feeds fused_adamw_(gscale_dev=out[1:]).
    """
    if partials.is_cuda:
        _require_ext("grad_norm_finalize").grad_norm_finalize_(
            partials, out, float(inv_count), float(clip))
        return
    inv = torch.tensor(inv_count, dtype=torch.float32)
    norm = partials.float().sum().sqrt() * inv
    coef = torch.ones((), dtype=torch.float32)
    if clip > 0:
        coef = torch.clamp(
            torch.tensor(clip, dtype=torch.float32) / (norm + 1e-6), max=1.0)
    out[0] = norm
    out[1] = inv * coef


# --------------------------------------------------------------------------
# Flash attention (causal, GQA)
# --------------------------------------------------------------------------
def doc_bounds(input_ids: torch.Tensor, eos_token_id: int):
    """Packed-document bounds of a [B, S] token batch, as int32 [B, S]:
    doc_start[b, i] is the row index of the first token of the document
    token i belongs to and doc_end[b, i] one past its last. The token after
    an EOS starts a new document; the EOS belongs to the document it ends.
    Plain tensor ops with no host sync and no data-dependent shape, so it
    runs inside a captured step; once per micro-batch."""
    B, S = input_ids.shape
    idx = torch.arange(S, device=input_ids.device, dtype=torch.int32)
    idx = idx.unsqueeze(0).expand(B, S)
    eos = input_ids == eos_token_id
    first = torch.ones_like(eos)
    first[:, 1:] = eos[:, :-1]
    start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)),
                         dim=1).values
    last = eos.clone()
    last[:, -1] = True
    ends = torch.where(last, idx + 1, torch.full_like(idx, S))
    end = torch.cummin(ends.flip(1), dim=1).values.flip(1)
    return start.contiguous(), end.contiguous()


def doc_end_from_start(doc_start: torch.Tensor) -> torch.Tensor:
    """doc_end for a valid doc_start: a document ends where the next one
    starts, the last at S. No host sync."""
    B, S = doc_start.shape
    idx = torch.arange(S, device=doc_start.device, dtype=doc_start.dtype)
    idx = idx.unsqueeze(0).expand(B, S)
    first = doc_start == idx
    # a start at i ends the document of token i-1 at i
    ends = torch.full_like(doc_start, S)
    ends[:, :-1] = torch.where(first[:, 1:], idx[:, 1:],
                               torch.full_like(idx[:, 1:], S))
    return torch.cummin(ends.flip(1), dim=1).values.flip(1).contiguous()


def validate_doc_bounds(doc_start: torch.Tensor,
                        doc_end: torch.Tensor | None, B: int, S: int) -> None:
    """Host-side check of the bounds contract (CPU path only; the GPU
    kernels never read the tensors on the host and clamp instead)."""
    for name, t in (("doc_start", doc_start), ("doc_end", doc_end)):
        if t is None:
            continue
        if t.dtype != torch.int32 or tuple(t.shape) != (B, S):
            raise ValueError(
                f"{name} must be int32 [{B}, {S}], got {t.dtype} "
                f"{tuple(t.shape)}")
    idx = torch.arange(S, device=doc_start.device).unsqueeze(0)
    ds = doc_start.long()
    if bool((ds < 0).any()) or bool((ds > idx).any()):
        raise ValueError("doc_start must satisfy 0 <= doc_start[b, i] <= i")
    if bool((ds[:, 1:] < ds[:, :-1]).any()):
        raise ValueError("doc_start must be non-decreasing along a row")
    if bool((torch.gather(ds, 1, ds) != ds).any()):
        raise ValueError("doc_start must be constant inside a document")
    if doc_end is not None:
        want = doc_end_from_start(doc_start)
        if not torch.equal(doc_end, want):
            raise ValueError("doc_end does not match doc_start")


def _doc_tensor(t: torch.Tensor, like: torch.Tensor, name: str):
    B, S = like.shape[:2]
    if t.dtype != torch.int32 or tuple(t.shape) != (B, S):
        raise ValueError(
            f"{name} must be int32 [{B}, {S}], got {t.dtype} {tuple(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{name} must be on {like.device}, is on {t.device}")
    return t.contiguous()


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  causal: bool = True,
                  doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 reference attention. q: [B,S,Hq,D], k/v: [B,S,Hkv,D]. With
    doc_start (int32 [B,S]) query i sees keys doc_start[b, i] .. i."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = _wide(q).permute(0, 2, 1, 3)  # B,Hq,S,D
    kf = _wide(k).permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = _wide(v).permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) / (D ** 0.5)
    if causal:
        mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1)
        s = s.masked_fill(mask, float("-inf"))
    if doc_start is not None:
        keys = torch.arange(S, device=q.device).view(1, 1, 1, S)
        before = keys < doc_start.long().view(B, 1, S, 1)
        s = s.masked_fill(before, float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, vf)
    return o.permute(0, 2, 1, 3).to(q.dtype)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, doc_start=None, doc_end=None):
        if q.is_cuda:
            ext = _require_ext("flash_attention")
            if not hasattr(ext, "attn_fwd"):
                raise RuntimeError(
                    "HIP flash attention kernel missing from extension; "
                    "rebuild the extension")
            ctx.causal = causal
            ctx.docs = doc_start is not None
            if ctx.docs:
                o, lse = ext.attn_fwd(q, k, v, causal, 0, doc_start)
                ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
            else:
                o, lse = ext.attn_fwd(q, k, v, causal)
                ctx.save_for_backward(q, k, v, o, lse)
            return o
        # CPU path: differentiable reference (no custom backward needed).
        raise RuntimeError("use attention() entry point for CPU tensors")

    @staticmethod
    def backward(ctx, do):
        saved = ctx.saved_tensors   # read once (activation checkpointing)
        q, k, v, o, lse = saved[:5]
        if ctx.docs:
            ds, de = saved[5:]
            dq, dk, dv = _C.attn_bwd(q, k, v, o, lse, do.contiguous(),
                                     ctx.causal, False, 1, ds, de)
        else:
            dq, dk, dv = _C.attn_bwd(q, k, v, o, lse, do.contiguous(),
                                     ctx.causal)
        return dq, dk, dv, None, None, None


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              causal: bool = True, doc_start: torch.Tensor | None = None,
              doc_end: torch.Tensor | None = None) -> torch.Tensor:
    """Causal GQA attention: HIP flash kernel on GPU, reference on CPU.

    doc_start / doc_end (int32 [B,S], see doc_bounds) restrict query i to
    the keys of its own packed document, doc_start[b, i] .. i; doc_end is
    derived when omitted. The GPU kernels clamp what they read from the
    tensors, so malformed bounds give wrong numbers, never a bad access;
    the CPU path validates them and raises ValueError."""
    if doc_start is None:
        if doc_end is not None:
            raise ValueError("doc_end needs doc_start")
        if q.is_cuda:
            return _FlashAttnFn.apply(q.contiguous(), k.contiguous(),
                                      v.contiguous(), causal)
        return attention_ref(q, k, v, causal)
    if not causal:
        raise ValueError("document bounds need causal=True")
    doc_start = _doc_tensor(doc_start, q, "doc_start")
    if doc_end is not None:
        doc_end = _doc_tensor(doc_end, q, "doc_end")
    if q.is_cuda:
        if doc_end is None:
            doc_end = doc_end_from_start(doc_start)
        return _FlashAttnFn.apply(q.contiguous(), k.contiguous(),
                                  v.contiguous(), causal, doc_start, doc_end)
    validate_doc_bounds(doc_start, doc_end, q.shape[0], q.shape[1])
    return attention_ref(q, k, v, causal, doc_start)


# --------------------------------------------------------------------------
# KV-cache attention decode (serving path; no autograd)
# --------------------------------------------------------------------------
@torch.no_grad()
def attention_decode(q: torch.Tensor, kcache: torch.Tensor,
                     vcache: torch.Tensor, T: int,
                     T_dev: torch.Tensor | None = None) -> torch.Tensor:
    """q: [B, Hq, D] new-token queries (post-RoPE); kcache/vcache:
    [B, Tmax, Hkv, D] with the first T rows valid. Returns [B, Hq, D].
    T_dev (int32 device scalar) overrides T under hipGraph replay."""
    if q.is_cuda:
        return _require_ext("attention_decode").attn_decode(
            q.contiguous(), kcache, vcache, T, T_dev)
    B, Hq, D = q.shape
    Hkv = kcache.shape[2]
    rep = Hq // Hkv
    kf = kcache[:, :T].float().permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    vf = vcache[:, :T].float().permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    s = torch.einsum("bhd,bhtd->bht", q.float(), kf) / (D ** 0.5)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bht,bhtd->bhd", p, vf).to(q.dtype)


# --------------------------------------------------------------------------
# Ragged-batch decode: per-sequence KV lengths on the device (no autograd)
# --------------------------------------------------------------------------
_RAGGED_TARGET_BLOCKS = 512    # about two blocks per CU (256 CUs)
_RAGGED_MIN_CHUNK = 64         # keys: one block step (4 loads x 16 rows)
_RAGGED_MAX_CHUNK = 2048       # keys: a longer chunk is a long serial tail
_RAGGED_MAX_SPLITS = 32
_RAGGED_CHUNK_ALIGN = 16       # rows of one block step at D = 128


def decode_ragged_splits(B: int, Hkv: int, Tmax: int) -> int:
    """Default split count of attention_decode_ragged. Depends on shapes
    alone — never on the lengths — so a captured grid stays valid. From the
    sweep in profiles/decode_ragged.log: about two blocks per CU, but no
    chunk above 2048 keys however many blocks that makes (unequal lengths
    leave the long sequences' blocks running alone); no chunk below 64
    keys; at most 32 splits."""
    want = max(_RAGGED_TARGET_BLOCKS // max(1, B * Hkv),
               -(-Tmax // _RAGGED_MAX_CHUNK))
    return max(1, min(want, Tmax // _RAGGED_MIN_CHUNK, _RAGGED_MAX_SPLITS))


def decode_ragged_chunk(Tmax: int, num_splits: int) -> int:
    """Keys per split: split z owns rows [z*chunk, (z+1)*chunk)."""
    per = -(-Tmax // max(1, num_splits))
    return -(-per // _RAGGED_CHUNK_ALIGN) * _RAGGED_CHUNK_ALIGN


@torch.no_grad()
def attention_decode_ragged(q: torch.Tensor, kcache: torch.Tensor,
                            vcache: torch.Tensor, lens: torch.Tensor, *,
                            num_splits: int | None = None) -> torch.Tensor:
    """q: [B, Hq, D] new-token queries (post-RoPE); kcache/vcache:
    [B, Tmax, Hkv, D]; lens: [B] int32 on q's device. Sequence b attends to
    rows [0, clamp(lens[b], 0, Tmax)); lens[b] == 0 gives a zero row. The
    host never reads lens, so the call can be captured and a replay follows
    new contents. Returns [B, Hq, D]."""
    B, Hq, D = q.shape
    Tmax, Hkv = kcache.shape[1], kcache.shape[2]
    if num_splits is None:
        num_splits = decode_ragged_splits(B, Hkv, Tmax)
    if q.is_cuda:
        return _require_ext("attention_decode_ragged").attn_decode_ragged(
            q.contiguous(), kcache, vcache, lens, int(num_splits),
            decode_ragged_chunk(Tmax, num_splits))
    rep = Hq // Hkv
    n = lens.clamp(0, Tmax).view(B, 1, 1)
    dead = torch.arange(Tmax).view(1, 1, Tmax) >= n          # [B,1,Tmax]
    # rows a sequence must not read may hold anything, NaN included
    gone = dead.view(B, Tmax, 1, 1)
    kf = kcache.float().masked_fill(gone, 0.0)
    vf = vcache.float().masked_fill(gone, 0.0)
    kf = kf.permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    vf = vf.permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    s = torch.einsum("bhd,bhtd->bht", q.float(), kf) / (D ** 0.5)
    s = s.masked_fill(dead, float("-inf"))
    p = torch.softmax(s, dim=-1).masked_fill(n == 0, 0.0)
    return torch.einsum("bht,bhtd->bhd", p, vf).to(q.dtype)


@torch.no_grad()
def qkv_rope_append_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                     pos: torch.Tensor, kcache: torch.Tensor,
                     vcache: torch.Tensor, Hq: int, Hkv: int,
                     D: int) -> torch.Tensor:
    """qkv: [B, (Hq+2Hkv)*D], one new token per sequence; pos: [B] int32 on
    qkv's device; cos/sin: [>= Tmax, D/2]. Rotates q and k of sequence b at
    pos[b] and writes the roped k and the v copy into cache[b, pos[b]] in
    place. A row with pos[b] outside [0, Tmax) writes nothing and gets a
    zero q row (a finished sequence). Returns q [B, Hq, D]."""
    if qkv.is_cuda:
        return _require_ext("qkv_rope_append").qkv_rope_append_(
            qkv.contiguous(), cos, sin, pos, kcache, vcache, Hq, Hkv, D)
    B = qkv.shape[0]
    Tmax = kcache.shape[1]
    if cos.shape[0] < Tmax or sin.shape[0] < Tmax:
        raise ValueError(
            f"rope table has {cos.shape[0]} rows, cache needs {Tmax}")
    live = (pos >= 0) & (pos < Tmax)
    p = pos.long().clamp(0, Tmax - 1)
    parts = qkv.view(B, Hq + 2 * Hkv, D).float()
    cs = cos[p].view(B, 1, D // 2)
    sn = sin[p].view(B, 1, D // 2)

    def rot(x):
        x1, x2 = x[..., : D // 2], x[..., D // 2:]
        return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], dim=-1)

    q = rot(parts[:, :Hq]).to(qkv.dtype)
    q = q.masked_fill(~live.view(B, 1, 1), 0)
    k = rot(parts[:, Hq:Hq + Hkv]).to(kcache.dtype)
    v = parts[:, Hq + Hkv:].to(vcache.dtype)
    rows = torch.nonzero(live).flatten()
    kcache[rows, p[rows]] = k[rows]
    vcache[rows, p[rows]] = v[rows]
    return q


# --------------------------------------------------------------------------
# Token sampling: temperature / top-k / top-p, one draw per row (no autograd)
# --------------------------------------------------------------------------
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 on Python ints: counter 4 words, key 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _M32)
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def sample_uniform(seed: int, counter: int) -> float:
    """The draw of sample_tokens for one row: key = (low, high) words of
    seed, counter = (low, high words of counter, 0, 0), u = (word 0 >> 8) *
    2^-24, in [0, 1)."""
    s, c = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    w = philox4x32_10((c & _M32, c >> 32, 0, 0), (s & _M32, s >> 32))
    return (w[0] >> 8) * 2.0 ** -24


def _sample_row_cpu(l: torch.Tensor, T: float, k: int, p: float,
                    u: float) -> int:
    V = l.numel()
    if not T > 0:
        return int(torch.argmax(l))        # first index of the maximum
    top = l.max()
    if not torch.isfinite(top):            # NaN, +inf or nothing finite:
        return int(torch.argmax(l))        # unspecified, but in range
    e = torch.exp((l - top) / T)           # exp(-inf) = 0
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < k < V:
        keep &= l >= torch.topk(l, k).values[-1]
    if p < 1:
        vals, inv = torch.unique(l[keep], return_inverse=True)  # ascending
        mass = torch.zeros(vals.numel(), dtype=l.dtype).index_add_(
            0, inv, e[keep])
        cum = torch.cumsum(mass.flip(0), 0)                     # descending
        hit = torch.nonzero(cum >= p * cum[-1]).flatten()
        at = int(hit[0]) if hit.numel() and p > 0 else 0
        keep &= l >= vals.flip(0)[at]
    C = torch.cumsum(torch.where(keep, e, torch.zeros_like(e)), 0)
    hit = torch.nonzero(keep & (C > u * C[-1])).flatten()
    if hit.numel():
        return int(hit[0])
    return int(torch.nonzero(keep & (e > 0)).flatten()[-1])


@torch.no_grad()
def sample_tokens(logits: torch.Tensor, temperature: torch.Tensor,
                  top_k: torch.Tensor, top_p: torch.Tensor,
                  seed: torch.Tensor, counter: torch.Tensor, *,
                  u: torch.Tensor | None = None) -> torch.Tensor:
    """One token per row of logits [B, V] (unit stride in V, any row
    stride; bf16 on the GPU). temperature / top_p: [B] fp32, top_k: [B]
    int32, seed: [B] int64, counter: [B] int32 or int64, all on the logits'
    device and never read by the host, so the call can be captured and a
    replay follows new contents. Returns int64 [B].

    Row b: temperature <= 0 gives the lowest index of the maximum logit and
    ignores the rest. Otherwise e_i = exp((l_i - max l) / T); 0 < top_k < V
    keeps the logits >= the k-th largest (ties kept); top_p < 1 then keeps
    the logits >= the first distinct value, descending, at which the
    cumulative mass reaches top_p * (surviving mass), top_p <= 0 the top
    tie group only. With C the running sum of the kept e_i in index order
    and M its total, the result is the first kept index with C_i > u * M
    (the last kept index of nonzero mass if rounding leaves none), where u =
    sample_uniform(seed[b], counter[b]) unless `u` ([B] fp32 in [0, 1)) is
    given. The same row gives the same token in any slot of any batch."""
    if logits.dim() != 2:
        raise ValueError("sample_tokens: logits must be [B, V]")
    if logits.is_cuda:
        if logits.dtype != torch.bfloat16:
            raise TypeError(
                f"sample_tokens: GPU logits must be bfloat16, got "
                f"{logits.dtype}")
        return _require_ext("sample_tokens").sample_tokens(
            logits, temperature, top_k, top_p, seed, counter, u)
    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.long)
    lf = logits.double()
    for b in range(B):
        ub = (float(u[b]) if u is not None
              else sample_uniform(int(seed[b]), int(counter[b])))
        out[b] = _sample_row_cpu(lf[b], float(temperature[b]), int(top_k[b]),
                                 float(top_p[b]), ub)
    return out


# --------------------------------------------------------------------------
# LayerNorm (GPT-family normalization)
# --------------------------------------------------------------------------
class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        if x.is_cuda:
            y, mu, rstd = _require_ext("layernorm").layernorm_fwd(x, w, b, eps)
        else:
            xf = _wide(x)
            mu = xf.mean(-1)
            var = xf.var(-1, unbiased=False)
            rstd = torch.rsqrt(var + eps)
            y = (((xf - mu.unsqueeze(-1)) * rstd.unsqueeze(-1)) * _wide(w) +
                 _wide(b)).to(x.dtype)
            mu, rstd = mu.reshape(-1), rstd.reshape(-1)
        ctx.save_for_backward(x, w, mu, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mu, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        if x.is_cuda:
            dx, dw, db = _C.layernorm_bwd(x, w, dy, mu, rstd)
        else:
            H = x.shape[-1]
            xf, wf, dyf = _wide(x), _wide(w), _wide(dy)
            muv = mu.view(*x.shape[:-1], 1)
            rs = rstd.view(*x.shape[:-1], 1)
            xhat = (xf - muv) * rs
            dyw = dyf * wf
            a1 = dyw.mean(-1, keepdim=True)
            a2 = (dyw * xhat).mean(-1, keepdim=True)
            dx = (rs * (dyw - a1 - xhat * a2)).to(x.dtype)
            dw = (dyf * xhat).reshape(-1, H).sum(0)
            db = dyf.reshape(-1, H).sum(0)
        return dx, dw.to(w.dtype), db.to(w.dtype), None


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
              eps: float = 1e-5) -> torch.Tensor:
    return _LayerNormFn.apply(x.contiguous(), w, b, eps)


# --------------------------------------------------------------------------
# Fused cross-entropy (mean reduction over all tokens)
# --------------------------------------------------------------------------
class _FusedCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, lse = _require_ext("cross_entropy").ce_fwd(logits, labels)
        ctx.save_for_backward(logits, labels, lse)
        return loss.mean()

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, lse = ctx.saved_tensors
        # device-scalar grad scale: stays correct under hipGraph replay
        gscale = (grad_out.float() / logits.numel() * logits.size(-1)) \
            .reshape(())
        dlogits = _C.ce_bwd(logits, labels, lse, gscale.contiguous())
        return dlogits, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean next-token CE. GPU bf16: fused single-pass kernels (one logits
    read fwd, one read + bf16 grad write bwd). CPU: eager fp32."""
    if logits.is_cuda and logits.dtype == torch.bfloat16:
        return _FusedCEFn.apply(logits.contiguous().view(-1, logits.shape[-1]),
                                labels.reshape(-1).int())
    return torch.nn.functional.cross_entropy(
        _wide(logits).view(-1, logits.shape[-1]), labels.reshape(-1))


# --------------------------------------------------------------------------
# Weight-gradient GEMM and the linear layer that accumulates through it
# --------------------------------------------------------------------------
_WGRAD_TILE = 256      # output tile edge of wgrad_gemm_kernel
_WGRAD_TOKENS = 64     # tokens per step
_WGRAD_GROUP = 4       # raster band height, in dy column slabs

# Dispatch by output shape [N, K], from tools/bench_wgrad.py at 32768 tokens
# (profiles/wgrad_gemm.log for the first kernel, profiles/wgrad_v2.log for
# variant 1 and the half blocks, whose figures stand below). The kernel
# serves a shape only where it was measured and its slowest round beat the
# fastest round of the library's mm + add_; the value is the raster band
# height. "blas": the library won when the table was made. A shape that is
# not listed was not measured and stays on the library (a small output is a
# handful of blocks on 256 CUs).
_WGRAD_DISPATCH = {
    (28672, 4096): 4,        # gate_up  5.68-5.71 ms against 6.76-6.81
    (4096, 14336): 4,        # down     2.95-2.98 (128 tiles halved) / 3.91-3.92
    (4096, 4096): 8,         # o        0.79-0.81 against 1.00-1.01
    (128256, 4096): 4,       # lm_head  26.53-26.63 (80 halved) / 30.80-30.98
    (6144, 4096): "blas",    # qkv      kept: now 1.26-1.29 against 1.51-1.52
}


def wgrad_impl() -> str:
    """TOK_WGRAD_IMPL, read at every call so one process can run an A/B:
    'hip' (default): the kernel for the shapes the dispatch table gives it;
    'hip_all': the kernel wherever it can run (tests, measuring new shapes);
    'blas': the library everywhere, and ops.linear is plain F.linear."""
    impl = os.environ.get("TOK_WGRAD_IMPL", "hip").lower()
    if impl not in ("hip", "hip_all", "blas"):
        raise ValueError(
            f"TOK_WGRAD_IMPL must be hip, hip_all or blas, got {impl!r}")
    return impl


def wgrad_band(N: int, K: int) -> int | None:
    """Raster band height if the current TOK_WGRAD_IMPL sends an [N, K]
    output to the kernel, None if it goes to the library."""
    impl = wgrad_impl()
    band = _WGRAD_DISPATCH.get((N, K))
    if impl == "hip_all":
        return band if isinstance(band, int) else _WGRAD_GROUP
    if impl == "hip" and isinstance(band, int):
        return band
    return None


def wgrad_fast_path(dy: torch.Tensor, x: torch.Tensor,
                    out: torch.Tensor) -> bool:
    """True if wgrad_gemm_kernel can run on these operands (whether it is
    chosen is wgrad_band's business)."""
    if not (dy.is_cuda and x.is_cuda and out.is_cuda):
        return False
    if dy.dim() != 2 or x.dim() != 2 or out.dim() != 2:
        return False
    M, N = dy.shape
    K = x.shape[1]
    return (all(t.dtype == torch.bfloat16 and t.is_contiguous() and
                t.data_ptr() % 16 == 0 for t in (dy, x, out))
            and M >= _WGRAD_TOKENS and M % _WGRAD_TOKENS == 0
            and N >= _WGRAD_TILE and N % _WGRAD_TILE == 0
            and K >= _WGRAD_TILE and K % _WGRAD_TILE == 0)


def wgrad_variant() -> int:
    """TOK_WGRAD_VARIANT, read at every call so one process can ablate the
    kernel's schedule: 0 is the two-barrier schedule, 1 reads the LDS
    fragments under the MFMAs; unset (or negative) is the extension's
    default. Every variant gives the same bits."""
    raw = os.environ.get("TOK_WGRAD_VARIANT", "-1")
    try:
        v = int(raw)
    except ValueError:
        v = 2
    if v > 1:
        raise ValueError(f"TOK_WGRAD_VARIANT must be 0 or 1, got {raw!r}")
    return max(v, -1)


def wgrad_split(N: int, K: int, cus: int) -> int:
    """Trailing tiles of an [N, K] output that wgrad_gemm_ computes as two
    128 x 256 half blocks each on a device of `cus` compute units. One block
    runs per unit, so r = tiles % cus tiles are left for the last round;
    when their 2 r halves still fit one round (0 < 2 r <= cus) that round
    costs a half block's time instead of a full one's."""
    if N <= 0 or K <= 0 or cus <= 0:
        return 0
    r = ((N // _WGRAD_TILE) * (K // _WGRAD_TILE)) % cus
    return r if 0 < 2 * r <= cus else 0


@torch.no_grad()
def wgrad_gemm_(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor,
                accumulate: bool, *, group: int | None = None,
                variant: int | None = None,
                split: int | None = None) -> torch.Tensor:
    """out[N,K] = (out if accumulate else 0) + dy[M,N]^T @ x[M,K], in place.

    CUDA bf16, contiguous, 16-byte aligned operands with M % 64 == 0 and N, K
    multiples of 256 run wgrad_gemm_kernel: fp32 accumulation, the old `out`
    added in fp32, one rounding, no temporary, where wgrad_band() gives the
    shape to the kernel (or `group` is passed, which forces it). It launches
    on the current stream and neither allocates nor syncs, so it can be
    captured. `variant` picks the kernel's schedule (None: wgrad_variant());
    `split` the number of trailing tiles computed as half blocks (None: the
    rule of wgrad_split for the device, 0: none). Neither changes a bit of
    the result. Every other input computes torch.mm(dy.t(), x) and adds or
    copies it. A GPU call the kernel should serve raises if the extension
    is not built, as every op of this package does."""
    if x.shape[0] != dy.shape[0] or out.shape != (dy.shape[1], x.shape[1]):
        raise ValueError(
            f"wgrad_gemm_: dy {tuple(dy.shape)}, x {tuple(x.shape)}, "
            f"out {tuple(out.shape)} do not fit out[N,K] = dy[M,N]^T x[M,K]")
    if group is None:
        group = wgrad_band(*out.shape)
    if group is not None and wgrad_fast_path(dy, x, out):
        tiles = (out.shape[0] // _WGRAD_TILE) * (out.shape[1] // _WGRAD_TILE)
        if split is not None and not 0 <= split <= tiles:
            raise ValueError(
                f"wgrad_gemm_: split {split} outside 0..{tiles} tiles")
        if variant is not None and variant not in (0, 1):
            raise ValueError(f"wgrad_gemm_: variant {variant} is not 0 or 1")
        _require_ext("wgrad_gemm_").wgrad_gemm_(
            dy, x, out, bool(accumulate), int(group),
            wgrad_variant() if variant is None else int(variant),
            -1 if split is None else int(split))
        return out
    g = torch.mm(dy.t(), x)
    if accumulate:
        out.add_(g)
    else:
        out.copy_(g)
    return out


def _grad_in_place(weight: torch.Tensor) -> bool:
    """The weight's .grad is a flat-bucket view that nothing watches, so
    backward may add into it and hand autograd None: no post-accumulate hook
    and no tensor hook (register_hook) waits for this gradient. Both hook
    tables are private attributes of torch.Tensor; test_kernel_oracle_gemm
    fails if either is renamed. Restriction that stays: such a weight gets
    no gradient from torch.autograd.grad(), which never touches .grad;
    FlatBucketModel sets the mark and trains through backward() only."""
    return (getattr(weight, "_tok_flat_grad", False)
            and weight.grad is not None
            and not getattr(weight, "_post_accumulate_grad_hooks", None)
            and not getattr(weight, "_backward_hooks", None))


# --------------------------------------------------------------------------
# Input-gradient GEMM: dx = dy @ W as a TN call on a transposed weight copy
# --------------------------------------------------------------------------
_TRANSPOSE_TILE = 64           # tile edge of weight_transpose_kernel
_TRANSPOSE_MAX_ROWS = 65535 * _TRANSPOSE_TILE    # grid.y limit


def _transpose_contract(src: torch.Tensor, out: torch.Tensor) -> str | None:
    """What of transpose_2d_'s contract the operands break, None if nothing."""
    if src.dim() != 2 or out.dim() != 2:
        return "src and out must be 2-D"
    if src.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
        return f"src and out must be bfloat16, got {src.dtype}, {out.dtype}"
    if src.device != out.device:
        return "src and out must be on one device"
    R, C = src.shape
    if tuple(out.shape) != (C, R):
        return f"out must be {(C, R)}, got {tuple(out.shape)}"
    if R < 8 or C < 8 or R % 8 or C % 8:
        return f"R and C must be multiples of 8, got {R}, {C}"
    if R > _TRANSPOSE_MAX_ROWS:
        return f"R must not exceed {_TRANSPOSE_MAX_ROWS}"
    if not (src.is_contiguous() and out.is_contiguous()):
        return "src and out must be contiguous"
    a, b = src.data_ptr(), out.data_ptr()
    if a % 16 or b % 16:
        return "src and out must be 16-byte aligned"
    nbytes = R * C * 2
    if a < b + nbytes and b < a + nbytes:
        return "src and out must not overlap"
    return None


@torch.no_grad()
def transpose_2d_(src: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[C,R] = src[R,C]^T for bf16, row-major, contiguous, 16-byte
    aligned, non-overlapping tensors with R and C multiples of 8; anything
    else raises ValueError. Bit patterns are moved, not numbers. On the GPU
    it is one launch of weight_transpose_kernel on the current stream, which
    neither allocates nor syncs, so it can be captured; CPU tensors do
    out.copy_(src.t())."""
    why = _transpose_contract(src, out)
    if why is not None:
        raise ValueError(f"transpose_2d_: {why}")
    if src.is_cuda:
        _require_ext("transpose_2d_").transpose_2d_(src, out)
    else:
        out.copy_(src.t())
    return out


# Dispatch by weight shape [N, K], from tools/bench_dgrad.py at 32768 tokens
# (profiles/dgrad_wt.log): (a) the library's NN call dy.mm(W) against (d) the
# transposition followed by the TN call F.linear(dy, Wt), fastest-slowest
# round in ms. A shape takes the transposed path only where the slowest round
# of (d) beat the fastest round of (a). A shape that is not listed was not
# measured and stays on dy.mm(W).
_DGRAD_DISPATCH = {
    (28672, 4096): True,     # gate_up  (d) 5.11-5.12 against (a) 5.54-6.16
    (4096, 14336): True,     # down     2.49-2.52 against 2.89-3.05
    (6144, 4096): True,      # qkv      1.08-1.11 against 1.23-1.28
    (4096, 4096): True,      # o        0.72-0.75 against 0.85-0.90
    (128256, 4096): True,    # lm_head  22.32-22.38 against 25.82-25.91
}


def dgrad_impl() -> str:
    """TOK_DGRAD_IMPL, read at every call so one process can run an A/B:
    'wt' (default): the transposed path for the shapes the table gives it;
    'wt_all': the transposed path wherever transpose_2d_ can run (tests,
    measuring new shapes); 'blas': dy.mm(W) everywhere. Independent of
    TOK_WGRAD_IMPL, except that with TOK_WGRAD_IMPL=blas ops.linear is plain
    F.linear and never gets here."""
    impl = os.environ.get("TOK_DGRAD_IMPL", "wt").lower()
    if impl not in ("wt", "wt_all", "blas"):
        raise ValueError(
            f"TOK_DGRAD_IMPL must be wt, wt_all or blas, got {impl!r}")
    return impl


def dgrad_transposed(N: int, K: int) -> bool:
    """True if the current TOK_DGRAD_IMPL sends the dgrad of an [N, K]
    weight through the transposed copy."""
    impl = dgrad_impl()
    if impl == "wt_all":
        return True
    return impl == "wt" and _DGRAD_DISPATCH.get((N, K)) is True


def dgrad(dy2: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """dx[M,K] = dy2[M,N] @ weight[N,K]. Where dgrad_transposed() says so and
    the weight fits transpose_2d_'s contract on the GPU: Wt = weight^T into a
    temporary made in this call from the live weight (so it cannot be stale;
    under capture it comes from the graph's private pool), then the TN call
    F.linear(dy2, Wt). Everything else is dy2.mm(weight)."""
    N, K = weight.shape
    if (weight.is_cuda and weight.dtype == torch.bfloat16
            and dy2.dtype == torch.bfloat16 and weight.is_contiguous()
            and weight.data_ptr() % 16 == 0 and N % 8 == 0 and K % 8 == 0
            and 8 <= N <= _TRANSPOSE_MAX_ROWS and K >= 8
            and dgrad_transposed(N, K)):
        wt = torch.empty((K, N), dtype=weight.dtype, device=weight.device)
        transpose_2d_(weight, wt)
        return torch.nn.functional.linear(dy2, wt)
    return dy2.mm(weight)


class _LinearFn(torch.autograd.Function):
    """y = x @ W^T. Forward is the library call nn.Linear makes; dx goes
    through dgrad (the same library, in the layout it is fastest at); dW
    goes through wgrad_gemm_, straight into W.grad where that is a
    flat-bucket view without hooks (returning None to autograd), into a
    fresh tensor otherwise."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        ctx.param = weight      # the Parameter itself: .grad and its marks
        return torch.nn.functional.linear(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        param = ctx.param
        N, K = weight.shape
        dx = dw = None
        dy2 = dy.reshape(-1, N)
        if ctx.needs_input_grad[0]:
            dx = dgrad(dy2, weight).view(x.shape)
        if ctx.needs_input_grad[1]:
            dy2 = dy2.contiguous()
            x2 = x.reshape(-1, K).contiguous()
            if _grad_in_place(param) and param.grad.dtype == dy2.dtype:
                wgrad_gemm_(dy2, x2, param.grad, True)
            else:
                dw = wgrad_gemm_(dy2, x2, torch.empty_like(weight), False)
        return dx, dw


def linear(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Bias-free linear layer over the last dimension of x. With
    TOK_WGRAD_IMPL=blas it is torch.nn.functional.linear under plain
    autograd."""
    if wgrad_impl() == "blas":
        return torch.nn.functional.linear(x, weight)
    return _LinearFn.apply(x, weight)


__all__ = [
    "linear", "wgrad_gemm_", "wgrad_fast_path", "wgrad_impl", "wgrad_band",
    "wgrad_variant", "wgrad_split",
    "dgrad", "dgrad_impl", "dgrad_transposed", "transpose_2d_",
    "rmsnorm", "rmsnorm_ref", "apply_rope", "rope_ref", "fused_adamw_",
    "attention", "attention_ref", "cross_entropy", "layernorm",
    "qkv_rope", "qkv_rope_ref", "doc_bounds", "doc_end_from_start",
    "validate_doc_bounds", "swiglu", "swiglu_ref",
    "hip_ext_available",
    "grad_sumsq_blocks", "grad_sumsq_", "grad_norm_finalize_",
    "attention_decode_ragged", "qkv_rope_append_",
    "decode_ragged_splits", "decode_ragged_chunk",
    "sample_tokens", "sample_uniform", "philox4x32_10",
]

"""fp64 references and ONE comparison rule for the non-attention kernels.

Plain formulas in float64, independent of ``torch_on_k8s_amd.ops`` (whose
CPU paths are themselves checked against this module by
``test_kernel_oracle.py``). Inputs are the bf16-quantized values the
kernel sees; every reference returns, per output, a ``Spec``:

    ref    the fp64 value
    scale  sum of |terms| the output is formed from (so cancelling outputs
           such as the RoPE halves, dx, or the CE gradient at the label are
           judged against what went into them, not against a small result);
           for row reductions the sum runs over the reduced rows too
    k      fp32 error budget in units of 2^-23 * scale (derived below)
    bf16   whether the output is stored in bf16

The rule, per element:

    |got - ref| <= 2^-8 * |ref| * [bf16]  +  k * 2^-23 * scale

2^-8 |ref| is the worst-case half ulp of a bf16 result (8 significand
bits); it is dropped for fp32 outputs. Results below the smallest normal
number (2^-126, shared by fp32 and bf16) may be flushed to zero, so that
much absolute error is always allowed. A test fails on ANY violation.

How k is counted. One fp32 rounding is at most 2^-24 relative, i.e. 0.5
unit. A reduction whose longest chain has d roundings costs ``kred(d)``
units of sum|terms|: the worst case d/2 for short chains and Higham's
probabilistic bound lambda*sqrt(d)*2^-24 with lambda = 8 for long ones
(independent roundings exceed it with probability ~2*exp(-32)). Fast
intrinsics: v_rsq_f32 / v_exp_f32 / v_log_f32 are 1 ulp (1 unit); __expf(a)
rounds a*log2(e) first, which adds |a| * 2^-24 relative -- that is why the
scales of exp-based outputs carry a factor (1 + |a|). None of the k below
was fitted to a kernel's output.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

U = 2.0 ** -23
BF16_HALF_ULP = 2.0 ** -8
TINY = 2.0 ** -126


@dataclass
class Spec:
    ref: torch.Tensor
    scale: torch.Tensor
    k: float
    bf16: bool
    tiny: float = TINY    # absolute allowance for flush-to-zero


@dataclass
class Result:
    name: str
    ratio: float      # worst |err| / tolerance
    ratio32: float    # share of the k-term provably used (see compare)
    violations: int
    numel: int

    def __str__(self):
        return (f"ORACLE {self.name}: ratio={self.ratio:.3f} "
                f"fp32_part={self.ratio32:.3f} "
                f"violations={self.violations}/{self.numel}")


def f64(t) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64)


def q16(t: torch.Tensor) -> torch.Tensor:
    """Quantize to bf16 (the kernels' I/O format)."""
    return t.to(torch.bfloat16)


def kred(d: int) -> float:
    """Units of 2^-23*sum|terms| for a sum whose longest chain has d
    fp32 roundings."""
    return math.ceil(0.5 * min(d, 8.0 * math.sqrt(d)))


def block_depth(n: int) -> int:
    """Roundings on the longest chain of the 256-thread block sum of n
    elements: 8 per bf16x8 vector per thread sweep, 6 wave shuffle steps,
    3 cross-wave adds."""
    return 8 * math.ceil(n / 2048) + 9


def compare(name: str, got: torch.Tensor, spec: Spec) -> Result:
    got = f64(got).reshape(-1)
    ref = spec.ref.reshape(-1)
    scale = spec.scale.reshape(-1)
    assert got.shape == ref.shape == scale.shape, (name, got.shape,
                                                   ref.shape, scale.shape)
    fp32_tol = spec.k * U * scale
    tol = fp32_tol + (BF16_HALF_ULP * ref.abs() if spec.bf16 else 0.0) + spec.tiny
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err,
                      torch.full_like(err, float("inf")))
    bad = err > tol
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    # A lower bound on the fp32 error alone: the value the kernel rounded
    # to bf16 lies within half a bf16 ulp of `got`, whose binade is known.
    if spec.bf16:
        _, e = torch.frexp(got)            # got = m * 2^e, 0.5 <= |m| < 1
        half = torch.ldexp(torch.ones_like(got), e - 9)
        half = torch.where(got == 0, torch.zeros_like(got), half)
        e32 = (err - half - spec.tiny).clamp_min(0.0)
    else:
        e32 = (err - spec.tiny).clamp_min(0.0)
    r32 = torch.where(e32 == 0, torch.zeros_like(e32), e32 / fp32_tol)
    r32 = torch.where(torch.isfinite(r32), r32, torch.zeros_like(r32))
    return Result(name, float(ratio.max()) if ratio.numel() else 0.0,
                  float(r32.max()) if r32.numel() else 0.0,
                  int(bad.sum()), got.numel())


def check(name: str, got: torch.Tensor, spec: Spec) -> Result:
    """Print the measured ratio, then fail on any violation."""
    r = compare(name, got, spec)
    print(r)
    assert r.violations == 0, str(r)
    return r


def check_all(prefix: str, got: dict, specs: dict) -> dict:
    res = {n: compare(f"{prefix}.{n}", g, specs[n]) for n, g in got.items()}
    for r in res.values():
        print(r)
    bad = [str(r) for r in res.values() if r.violations]
    assert not bad, "\n".join(bad)
    return res


def violates(got: dict, specs: dict) -> list:
    """Names of the outputs that break the rule (for mutant tests)."""
    return [n for n, g in got.items() if compare(n, g, specs[n]).violations]


# --------------------------------------------------------------------------
# Inputs shared by the CPU and GPU tests (seeded, already bf16)
# --------------------------------------------------------------------------
def bf(*shape, scale=1.0, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return q16(torch.randn(*shape, generator=g) * scale + offset)


def ce_inputs(N, V, seed=0):
    logits = bf(N, V, scale=2.0, seed=seed)
    # one row spread over +-80
    logits[1] = q16(torch.linspace(-80, 80, V)[torch.randperm(
        V, generator=torch.Generator().manual_seed(seed))])
    labels = torch.randint(0, V, (N,),
                           generator=torch.Generator().manual_seed(seed + 1))
    labels[0], labels[1], labels[-1] = 0, V - 1, V - 3
    return logits, labels


def decode_inputs(B, T, Hq, Hkv, D, seed=0):
    Tmax = T + 7
    q = bf(B, Hq, D, seed=seed)
    kc = bf(B, Tmax, Hkv, D, seed=seed + 1)
    vc = bf(B, Tmax, Hkv, D, seed=seed + 2)
    # one key that scores far above the rest, for every q head of kv head 0
    kc[:, T // 2, 0] = q16(q[:, 0] * 2.0)
    kc[:, T:] = float("nan")
    vc[:, T:] = float("nan")
    return q, kc, vc


def rope_table(S, D, theta=10000.0):
    half = D // 2
    inv = 1.0 / (theta ** (torch.arange(half, dtype=torch.float64) / half))
    ang = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return ang.cos().float(), ang.sin().float()


def ln_inputs(case):
    if case == "const":
        # two constant rows (var = 0 exactly) and a nearly constant one:
        # one element a bf16 ulp off, var = 2.4e-4 against a mean of 100
        x = torch.full((3, 1024), 100.0)
        x[1] = 100.5
        x[2, 517] = 100.5
        x = q16(x)
    elif isinstance(case, tuple) and case[0] == "offset":
        x = bf(3, 1024, offset=case[1], seed=1)
    else:
        x = bf(*case, seed=1)
    H = x.shape[1]
    return x, bf(H, seed=3), bf(H, seed=4), bf(*x.shape, seed=2)


def swiglu_inputs(rows, I, seed=0):
    gu = bf(rows, 2 * I, seed=seed)
    # gate magnitudes up to +-30 in the first row(s)
    gu[0, :I] = q16(torch.linspace(-30, 30, I))
    return gu, bf(rows, I, seed=seed + 1)


# --------------------------------------------------------------------------
# RMSNorm (plain and fused-residual)
# --------------------------------------------------------------------------
def rms_dw_depth(rows: int, H: int) -> int:
    """Row-reduction chain of the two-stage dw: serial rows per split,
    serial splits per colsum block, then one atomic per colsum block."""
    cblocks = max(1, math.ceil(H / 8 / 256))
    rsplit = max(1, min(rows, 2048 // cblocks))
    rb = max(1, min(rsplit, 2048 // max(1, math.ceil(H / 256))))
    return math.ceil(rows / rsplit) + math.ceil(rsplit / rb) + rb


def k_invr(H: int) -> float:
    # sum x^2 (block_depth), /H, +eps: relative kred(d) on a positive sum;
    # rsqrt halves it; v_rsq_f32 adds 1 ulp.
    return kred(block_depth(H) + 2) / 2 + 1


def residual_sum(x, res) -> Spec:
    """xr = x + res, stored in bf16: one fp32 add (k = 1)."""
    x, res = f64(x), f64(res)
    return Spec(x + res, x.abs() + res.abs(), 1, True)


def rmsnorm(x, w, eps, dy=None, dxr=None, drop_last_vec=False,
            divisor_off=0, no_eps=False) -> dict:
    """x: [rows, H] (for the fused op: the bf16 xr the kernel formed).
    The three flags build deliberately wrong references."""
    x, w = f64(x), f64(w)
    rows, H = x.shape
    xs = x[:, :H - 8] if drop_last_vec else x
    ms = xs.pow(2).sum(-1, keepdim=True) / (H + divisor_off)
    r = 1.0 / torch.sqrt(ms + (0.0 if no_eps else eps))
    ki = k_invr(H)
    y = x * r * w
    out = {"invr": Spec(r.reshape(-1), r.reshape(-1), ki, False),
           # x*r*w: r's error plus two products
           "y": Spec(y, y.abs(), ki + 1, True)}
    if dy is None:
        return out
    dy = f64(dy)
    t = dy * w * x
    c = t.sum(-1, keepdim=True)
    cabs = t.abs().sum(-1, keepdim=True)
    dx = r * (w * dy - x * (r * r / H) * c)
    sdx = r * ((w * dy).abs() + x.abs() * (r * r / H) * cabs)
    if dxr is not None:
        dx = dx + f64(dxr)
        sdx = sdx + f64(dxr).abs()
    # c: one product per term then the fma chain; c*r*r/H, x*k, the
    # subtraction, *r, +dxr: 7 roundings (3.5 -> 4); r enters cubed.
    out["dx"] = Spec(dx, sdx, kred(block_depth(H) + 1) + 3 * ki + 4, True)
    tw = dy * x * r
    # per term: r's error, dy*r and the fma; then the row chain
    out["dw"] = Spec(tw.sum(0), tw.abs().sum(0),
                     kred(rms_dw_depth(rows, H)) + ki + 1, False)
    return out


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------
def ln_dwdb_depth(rows: int, H: int) -> int:
    cblocks = max(1, math.ceil(H / 8 / 256))
    rsplit = max(1, min(rows, 2048 // cblocks))
    return math.ceil(rows / rsplit) + rsplit   # serial rows + atomics


def layernorm(x, w, b, eps, dy=None, drop_last_vec=False, divisor_off=0,
              no_eps=False) -> dict:
    x, w, b = f64(x), f64(w), f64(b)
    rows, H = x.shape
    n = H + divisor_off
    xs = x[:, :H - 8] if drop_last_vec else x
    mu = xs.sum(-1, keepdim=True) / n
    var = (xs - mu).pow(2).sum(-1, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else eps))
    mabs = x.abs().mean(-1, keepdim=True)
    k_mu = kred(block_depth(H) + 1)            # block sum, /H
    # sum (x-mu)^2 about a mean that is off by dmu <= k_mu*U*mean|x| grows
    # by exactly H*dmu^2 (the first-order term sums to zero): rstd moves by
    # 0.5*dmu^2/(var+eps) relative. Folded into the scale as the factor f
    # (any k >= 0.5 then covers it). The subtraction x-mu, /H, +eps and the
    # fma chain are block_depth+3 roundings, halved by rsqrt, +1 ulp.
    f = 1.0 + U * (k_mu * mabs).pow(2) / (var + eps)
    k_rstd = kred(block_depth(H) + 3) / 2 + 1
    # xhat = (x-mu)*rstd: |x-mu| carries rstd's error, mean|x| carries mu's
    xh = (x - mu) * rstd
    xh_s = ((x - mu).abs() * f + mabs) * rstd
    y = xh * w + b
    out = {"mu": Spec(mu.reshape(-1), mabs.reshape(-1), k_mu, False),
           "rstd": Spec(rstd.reshape(-1), (rstd * f).reshape(-1), k_rstd,
                        False),
           # (x-mu)*rstd*w + b: mu, rstd, and 4 roundings
           "y": Spec(y, xh_s * w.abs() + b.abs(), k_mu + k_rstd + 2, True)}
    if dy is None:
        return out
    dy = f64(dy)
    dyw = dy * w
    a1 = dyw.mean(-1, keepdim=True)
    a2 = (dyw * xh).mean(-1, keepdim=True)
    dx = rstd * (dyw - a1 - xh * a2)
    sdx = rstd * f * (dyw.abs() + dyw.abs().mean(-1, keepdim=True) +
                      xh_s * (dyw.abs() * xh_s).mean(-1, keepdim=True))
    # a1, a2: product + chain + /H; xhat appears twice (mu and rstd error
    # each time), rstd once more; 4 roundings to combine (2 units, -> 4)
    out["dx"] = Spec(dx, sdx, kred(block_depth(H) + 2) +
                     2 * (k_mu + k_rstd) + k_rstd + 4, True)
    d = ln_dwdb_depth(rows, H)
    tw = dy * xh
    out["dw"] = Spec(tw.sum(0), (dy.abs() * xh_s).sum(0),
                     kred(d) + k_mu + k_rstd + 1, False)
    out["db"] = Spec(dy.sum(0), dy.abs().sum(0), kred(d), False)
    return out


# --------------------------------------------------------------------------
# Cross-entropy (mean over rows), labels in [0, V)
# --------------------------------------------------------------------------
def cross_entropy(logits, labels, grad_out=1.0, label_shift=0,
                  drop_last_vec=False, divisor_off=0) -> dict:
    x = f64(logits)
    N, V = x.shape
    lab = (labels.detach().cpu().long() + label_shift) % V
    xs = x[:, :V - 8] if drop_last_vec else x
    M = xs.max(-1, keepdim=True).values
    lse = M + torch.log(torch.exp(xs - M).sum(-1, keepdim=True))
    p = torch.exp(x - lse)
    xl = x.gather(1, lab.view(-1, 1))
    # Online softmax: each thread chains 8*ceil(V/2048) exp-and-add steps,
    # then 6 wave and 3 block merges of ~3 roundings each. Every exp(a)
    # carries (1+|a|)*2^-24 from its argument and 1 ulp; weighted by the
    # softmax that is A = sum p*(1+|x-M|). logf: 1 ulp of |lse-M|; M + log:
    # one rounding of |lse|.
    d = 8 * math.ceil(V / 2048) + 27
    k_lse = kred(d) + 3
    A = (torch.exp(x - lse) * (1 + (x - M).abs())).sum(-1, keepdim=True)
    s_lse = M.abs() + (lse - M).abs() + A
    loss_rows = lse - xl
    s_rows = s_lse + xl.abs()
    gs = grad_out / (N + divisor_off)
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    dlog = (p - onehot) * gs
    # exp(x - l): l's absolute error (k_lse units of s_lse) is a relative
    # error of p; x - l rounds relative to |x - l|; 1 ulp; -1; *gs, and gs
    # itself is formed in fp32 (2 roundings): k_lse + 3.
    s_d = abs(gs) * (p * (1 + (x - lse).abs() + s_lse) + onehot)
    return {
        "lse": Spec(lse.reshape(-1), s_lse.reshape(-1), k_lse, False),
        "loss_rows": Spec(loss_rows.reshape(-1), s_rows.reshape(-1),
                          k_lse + 1, False),
        # mean over rows: torch's fp32 pairwise sum (chain <= 16 + log2 N)
        "loss": Spec((loss_rows.sum() / (N + divisor_off)).reshape(1),
                     s_rows.mean().reshape(1),
                     k_lse + 1 + kred(16 + math.ceil(math.log2(max(N, 2)))),
                     False),
        # p below 2^-126 is flushed before it meets gs
        "dlogits": Spec(dlog, s_d, k_lse + 3, True, TINY * max(1.0, abs(gs))),
    }


# --------------------------------------------------------------------------
# RoPE (rotate-half), table row s = position s
# --------------------------------------------------------------------------
K_ROPE = 2  # two products and one add/sub per output: 1.5 units -> 2


def rope(x, cos, sin, sign=1.0, pos_shift=0, swap_halves=False) -> Spec:
    """x: [B,S,H,D]; cos/sin fp32 [>= S, D/2]; only the first S rows
    count. Returns one Spec for the whole [B,S,H,D] output."""
    x = f64(x)
    B, S, H, D = x.shape
    idx = (torch.arange(S) + pos_shift) % cos.shape[0]
    cs = f64(cos)[idx].view(1, S, 1, D // 2)
    sn = f64(sin)[idx].view(1, S, 1, D // 2) * sign
    a, b = x[..., :D // 2], x[..., D // 2:]
    if swap_halves:
        a, b = b, a
    y = torch.cat([a * cs - b * sn, b * cs + a * sn], -1)
    s = torch.cat([(a * cs).abs() + (b * sn).abs(),
                   (b * cs).abs() + (a * sn).abs()], -1)
    return Spec(y, s, K_ROPE, True)


def qkv_split(qkv, Hq, Hkv, D):
    B, S, _ = qkv.shape
    parts = qkv.view(B, S, Hq + 2 * Hkv, D)
    return parts[:, :, :Hq], parts[:, :, Hq:Hq + Hkv], parts[:, :, Hq + Hkv:]


# --------------------------------------------------------------------------
# SwiGLU over packed [rows, 2I]
# --------------------------------------------------------------------------
def swiglu(gu, dout=None) -> dict:
    gu = f64(gu)
    I = gu.shape[-1] // 2
    g, u = gu[:, :I], gu[:, I:]
    sg = torch.sigmoid(g)
    # sigma = 1/(1+exp(-g)): the exp's relative error (1 ulp + |g|*2^-24
    # from its argument) reaches sigma scaled by (1 - sigma).
    ex = 1 + (1 - sg) * g.abs()
    out = g * sg * u
    # exp 1 unit; 1+e, the divide, g*sigma, *u: 2 units -> k = 4 (the
    # argument term needs k >= 0.5 on the ex factor)
    res = {"out": Spec(out, out.abs() * ex, 4, True)}
    if dout is None:
        return res
    d = f64(dout)
    dsilu = sg * (1 + g * (1 - sg))
    # 1 - sigma is formed by subtraction (absolute 2^-24), then times g:
    # the bracket is good to |g|*2^-24, hence the (1+|g|) factor.
    s_dg = (d * u).abs() * sg * (1 + g.abs()) * ex
    du = d * g * sg
    res["dgu"] = Spec(torch.cat([d * u * dsilu, du], -1),
                      torch.cat([s_dg, du.abs() * ex], -1), 6, True)
    return res


# --------------------------------------------------------------------------
# AdamW, ONE step from a given state (p bf16 values, m/v fp32 values)
# --------------------------------------------------------------------------
def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step,
               grad_scale=1.0, no_weight_decay=False) -> dict:
    """The kernel takes its hyperparameters as fp32, so the reference
    rounds them the same way; 1 - beta is exact in fp32 for beta in
    [0.5, 1]."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    lr, b1, b2, eps, wd, gsc = (_f32(a) for a in (
        lr, beta1, beta2, eps, weight_decay, grad_scale))
    if no_weight_decay:
        wd = 0.0
    grad = g * gsc
    mn = b1 * m + (1 - b1) * grad
    vn = b2 * v + (1 - b2) * grad * grad
    bc1 = 1.0 / (1.0 - b1 ** step)
    bc2 = 1.0 / (1.0 - b2 ** step)
    upd = lr * (mn * bc1) / (torch.sqrt(vn * bc2) + eps)
    pn = p - lr * wd * p - upd
    # m: g*gscale, two products, one add (2 units) + 2 units for a path
    # that forms 1 - beta from the double (fp32(0.1) vs 1 - fp32(0.9) is
    # 2.4e-7 relative): k = 4. v has one more product: k = 5.
    # p: the update term carries m (4) and half of v (2.5), each bias
    # correction (powf then 1 - pow cancels: <= 3 units, halved for v),
    # sqrt, +eps, the divide, *lr, and the two subtractions: <= 16.
    return {
        "m": Spec(mn, (b1 * m).abs() + ((1 - b1) * grad).abs(), 4, False),
        "v": Spec(vn, b2 * v.abs() + (1 - b2) * grad * grad, 5, False),
        "p": Spec(pn, p.abs() + lr * wd * p.abs() + upd.abs(), 16, True),
    }


# --------------------------------------------------------------------------
# Single-token attention decode over a KV cache
# --------------------------------------------------------------------------
def attention_decode(q, kcache, vcache, T, kv_head_shift=0) -> Spec:
    """q: [B,Hq,D]; caches [B,Tmax,Hkv,D], rows >= T are never read."""
    q = f64(q)
    B, Hq, D = q.shape
    Hkv = kcache.shape[2]
    rep = Hq // Hkv
    hk = (torch.arange(Hq) // rep + kv_head_shift) % Hkv
    k = f64(kcache[:, :T])[:, :, hk]            # [B,T,Hq,D]
    v = f64(vcache[:, :T])[:, :, hk]
    sc = 1.0 / math.sqrt(D)
    s = torch.einsum("bhd,bthd->bht", q, k) * sc
    sabs = torch.einsum("bhd,bthd->bht", q.abs(), k.abs()) * sc
    M = s.max(-1, keepdim=True).values
    p = torch.softmax(s, -1)
    out = torch.einsum("bht,bthd->bhd", p, v)
    # A score is a D-term dot (<= 2 fma + 6 shuffle steps, *scale): kred(9)
    # units of sum|q k|; that absolute error of s and of the running max
    # is a relative error of p, as is the exp's (1+|s-M|)*2^-24 + 1 ulp.
    # The running (l, o) pair is rescaled and extended ceil(T/8) times per
    # wave (3 roundings each), merged over 8 waves (2 each) and divided.
    w = 1 + (s - M).abs() + 2 * sabs.max(-1, keepdim=True).values
    scale = torch.einsum("bht,bthd->bhd", p * w, v.abs())
    kk = 2 * kred(3 * math.ceil(T / 8) + 17) + kred(9) + 4
    return Spec(out, scale, kk, True)

"""fp64 references for the TRAINING attention kernels of ``attention.hip``
(forward v3/v4, ``attn_bwd_pre``, fused dK+dV, split dV/dK, the three dQ
variants), judged per element by the rule of ``kernel_oracle.py`` (imported,
not changed) with ONE more term.

These kernels round intermediates to bf16, which no other kernel does, so a
spec carries, next to ``ref``, ``scale``, ``k`` and ``bf16`` (as ``kernel_
oracle.Spec``), a tensor ``mid``:

    |got - ref| <= 2^-8 |ref| [bf16 output] + 2^-8 * mid
                   + k * 2^-23 * scale + 2^-126

``mid`` is the sum of |terms| that passed through a bf16 intermediate, each
weighted by the number of such roundings it saw. LSE is an fp32 output with
no bf16 intermediate in front of it: mid = 0 and no 2^-8 |ref|.

Everything is a plain formula in float64 from the bf16-exact q, k, v, dout;
nothing is imported from the package under test. Line numbers refer to
``torch_on_k8s_amd/ops/csrc/attention.hip``.

Notation, per batch b, q head h (kv head h // rep), query row i, key j,
sc = 1/sqrt(D):
    s_ij = sc * q_i.k_j          sabs_ij = sc * sum_d |q_id k_jd|
    M_i = max_j s_ij             lse_i = log sum_j exp(s_ij)
    p_ij = exp(s_ij - lse_i)     O_i = sum_j p_ij v_j
    dP_ij = dO_i.v_j             dPabs_ij = sum_d |dO_id v_jd|
    delta_i = sum_d dO_id O_id   dS_ij = p_ij (dP_ij - delta_i)
    dQ_i = sc sum_j dS_ij k_j    dK_j = sc sum_{h in group} sum_i dS_ij q_i
    dV_j = sum_{h in group} sum_i p_ij dO_i

THE bf16 ROUNDING POINTS (-> mid)
 1. P before P.V and before dV. The forward rounds the unnormalised
    pe = exp(s - m_run) in the P repack (v3: pack_bf16 at 379-393; v4:
    repack_pa at 632-633, defined 204-218); l_run sums the UNROUNDED pe
    (v3 352-358, v4 607-614), so the normaliser adds nothing. The dV
    kernels round p the same way (split 898-899, fused 1308).
        mid_O = sum_j p_ij |v_j|         mid_dV = sum_i p_ij |dO_i|
 2. dS^T before dQ and dK (repack_pa at 1599-1600 and 1725 for dQ, 1059-
    1060 split dK, 1309 fused): 2^-8 |dS_ij| per term.
 3. O as attn_bwd_pre_kernel reads it (735, fma chain 746-750). It reads the
    forward's bf16 output: the output rounding is 2^-8 |O_id| per element,
    and the forward's rounding of P (point 1) is in it as well. Through
    delta_i = sum_d dO_id O_id the latter is sum_j p_ij eps_j dP_ij with
    |eps_j| <= 2^-8 (the sum over d closes to dP before the bound is
    taken). So delta is off by 2^-8 * d16_i,
        d16_i = sum_d |dO_id O_id| + sum_j p_ij |dP_ij|,
    which enters dS as p_ij * err and from there dQ and dK:
        mid_dQ = sc sum_j (|dS_ij| + p_ij d16_i) |k_j|
        mid_dK = sc sum_{h,i} (|dS_ij| + p_ij d16_i) |q_i|
    (The fp32 part of the O rule reaches delta too; it is in d32 below.)

THE fp32 CHAINS (-> k * scale)
One fp32 rounding is half a unit of 2^-23; chains are counted with
``kernel_oracle.kred``. The CDNA programming guide describes the f32 MFMA
as "a k-ordered fmaf chain, one rounding per product, no wider internal
accumulation" and gives no tighter bound for mfma_f32_32x32x16_bf16, so
every MFMA sum here is counted as one rounding per product.

Several chains round against different sums of |terms| (a score chain
against sum|q k|, an accumulator chain against the accumulated terms, ...).
Each is counted on its own as k_c units of scale_c; a spec then holds
    scale = sum_c k_c scale_c / k,   k = the sum of the chains' own counts
so that k * 2^-23 * scale, which is all the rule uses, is exactly the sum
of the chains' budgets (inherited budgets such as t_lse and d32 below are
in the sum, already in units of 2^-23).

 K_SCORE(D) = kred(D) + 2, in units of sabs. The D-term MFMA chain
    (v3 296-303, v4 552-556, dQ 1569-1578, split 869-875 / 1026-1031,
    fused 1260-1268), and the softmax scale: v3 multiplies (317, 327; half
    a unit); v4 and dQ fold it into c2 = scale * LOG2E (512, 1526, fused
    1401): 1/sqrtf, the constant, the product, and the fma that applies it
    (609) - two units. An error of c2 is a relative error of every score,
    hence also in units of sabs.
 K_EXP = 1, in units of (1 + |a|), a the exp argument. v3: the subtraction
    and the multiply inside __expf are half a unit of |a| each, v_exp_f32
    is 1 ulp (353). v4: one fma and a 1-ulp exp2 (608-609).
    Forward: |a| <= |s - M| + 8, because on the defer path (339-346, 591-
    599) m_run trails the true max by up to DEFER_THR = 8 nats.
    Backward: a = s - lse exactly (no defer): 889, 1050, 1300, 1589, 1718.
 Forward accumulators, n_t = ceil(S/64) key tiles:
    o_acc takes 64 products per tile (four 16-key MFMAs, 402-410 / 637-645)
    and one alpha multiply on a tile that rescales (363-371 / 619-627):
    d_o = 65 n_t. l_run takes 32 in-lane adds, one shuffle add and
    l*alpha + rsum (347-358 / 603-614): d_l = 35 n_t. O = o_acc * (1/l) is
    two more roundings (427-433 / 662-679). alpha itself multiplies o_acc
    and l_run alike, so its error cancels in O:
        K_PV = kred(d_o) + kred(d_l) + 1     units of sum_j p_ij |v_j|
    In LSE alpha does not cancel. alpha = exp(a_t), a_t <= 0, is good to
    (1 + |a_t|) units and scales the part of l gathered before tile t,
    l_old e^{a_t} / (l_old e^{a_t} + rsum) of the whole with rsum >= 1 (the
    row's new max is in this tile, or alpha is exactly 1) and l_old <=
    S e^8: (1 + |a|) L e^a / (L e^a + 1) <= 1 + ln L = 9 + ln S per tile:
        K_ALPHA = n_t * ceil(9 + ln S)       units of 1 (absolute, on LSE)
 LSE = m_run [* LN2] + __logf(l_run) (437 / 695). __logf is a 1-ulp
    v_log_f32 and the multiply by ln 2: 2 units of |log l_run| <= |lse - M|
    + 8. v4's m_run * LN2: the constant and the product, 1 unit of |m_run|
    <= |M| + 8. The final add: 1 unit of |lse|.
 Backward. p_ij = exp(s_ij - lse_i) with the lse the FORWARD KERNEL wrote,
    which is within the LSE rule: its whole tolerance t_lse_i (absolute) is
    a relative error of p_ij. dQ forms nl2 = -lse * LOG2E (1527, 1899): 1
    unit of |lse|. The fused dK+dV kernel starts its S accumulator at
    -lse * sqrt(D) (written at 768, loaded 1249-1257, chain 1260-1268, exp2
    at 1300), so every rounding of that D-term chain is relative to
    |lse| sqrt(D) + sum|q k|, i.e. K_SCORE units of |lse| + sabs after the
    scale. That is in the dK and dV scale as |lse|, not in a larger k.
        pe_ij = K_SCORE (sabs_ij [+ |lse_i| for dK, dV]) + |lse_i|
                + K_EXP (1 + |s_ij - lse_i|) + t_lse_i / 2^-23
    dP is a D-term MFMA chain (1576, 1035, 1271) that the fused kernel
    starts at -Dsum (769, 1250): K_DP = kred(D) units of dPabs_ij +
    |delta_i|. dP - delta and p * (.) (1057, 1306, 1596, 1723): 1 unit of
    |dS|. delta (746-750) is 8 fma and log2(D/8) shuffle adds:
    kred(8 + log2(D/8)) units of sum_d |dO O|, plus the fp32 part of the O
    rule through dO: together d32_i.
    Accumulators: dQ sums 64 n_t products and is scaled (1631, 1975):
    K_SUMQ = kred(64 n_t) + 1. dK and dV sum rep * 64 n_t products (all q
    heads of the group into one accumulator, 845-851 / 995-1003 / 1415-
    1416); dK is scaled (1084, 1464): K_SUMK = kred(rep * 64 n_t) + 1.

None of these numbers was fitted to a kernel's output.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from kernel_oracle import BF16_HALF_ULP, TINY, U, f64, kred, q16

BN = 64            # keys per tile of the forward and dQ kernels
DEFER_THR = 8.0    # nats; attention.hip 339 / 591
K_EXP = 1


@dataclass
class AttnSpec:
    ref: torch.Tensor
    mid: torch.Tensor
    scale: torch.Tensor
    k: float
    bf16: bool


@dataclass
class Result:
    name: str
    ratio: float
    violations: int
    numel: int
    shares: tuple    # (2^-8|ref|, 2^-8 mid, k*2^-23*scale) / tol at the worst

    def __str__(self):
        a, b, c = self.shares
        return (f"ORACLE {self.name}: ratio={self.ratio:.3f} "
                f"violations={self.violations}/{self.numel} "
                f"tol_shares[out_bf16/mid/fp32]={a:.2f}/{b:.2f}/{c:.2f}")


def k_score(D: int) -> float:
    return kred(D) + 2


def n_tiles(S: int) -> int:
    return math.ceil(S / BN)


def k_pv(S: int) -> float:
    return kred(65 * n_tiles(S)) + kred(35 * n_tiles(S)) + 1


def k_alpha(S: int) -> float:
    return n_tiles(S) * math.ceil(9 + math.log(S))


def k_dp(D: int) -> float:
    return kred(D)


def k_delta(D: int) -> float:
    return kred(8 + int(math.log2(D // 8)))


def k_sumq(S: int) -> float:
    return kred(64 * n_tiles(S)) + 1


def k_sumk(S: int, rep: int) -> float:
    return kred(rep * 64 * n_tiles(S)) + 1


def _spec(ref, mid, parts, bf16) -> AttnSpec:
    """parts: [(k_c, scale_c)], scale_c broadcastable to ref."""
    k = float(sum(kc for kc, _ in parts))
    tot = sum(kc * sc for kc, sc in parts)
    return AttnSpec(ref, mid, (tot / k).expand_as(ref), k, bf16)


# --------------------------------------------------------------------------
# The comparison
# --------------------------------------------------------------------------
def compare(name: str, got: torch.Tensor, spec: AttnSpec) -> Result:
    got = f64(got).reshape(-1)
    ref = spec.ref.reshape(-1)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    t_out = BF16_HALF_ULP * ref.abs() if spec.bf16 else torch.zeros_like(ref)
    t_mid = BF16_HALF_ULP * spec.mid.reshape(-1)
    t_32 = spec.k * U * spec.scale.reshape(-1)
    tol = t_out + t_mid + t_32 + TINY
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err,
                      torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    if ratio.numel() == 0:
        return Result(name, 0.0, 0, 0, (0.0, 0.0, 0.0))
    w = int(ratio.argmax())
    shares = tuple(float(t[w] / tol[w]) for t in (t_out, t_mid, t_32))
    return Result(name, float(ratio[w]), int((err > tol).sum()), got.numel(),
                  shares)


def check(name: str, got: torch.Tensor, spec: AttnSpec) -> Result:
    """Print the measured ratio and the tolerance's make-up at the worst
    element, then fail on any violation. No element is excluded."""
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
    return [n for n, g in got.items() if compare(n, g, specs[n]).violations]


# --------------------------------------------------------------------------
# Inputs shared by the CPU and GPU tests (seeded, already bf16)
# --------------------------------------------------------------------------
# (B, S, Hq, Hkv, D, causal): the union of the shapes the per-kernel test
# files chose per launch path, then three tile edges.
SHAPES = [
    (1, 40, 2, 2, 64, True),
    (1, 96, 2, 1, 128, True),
    (1, 128, 2, 2, 64, False),
    (1, 200, 2, 1, 64, True),
    (1, 256, 2, 2, 128, True),
    (1, 264, 2, 2, 64, False),
    (1, 320, 2, 1, 128, True),
    (1, 328, 4, 1, 128, True),
    (2, 512, 8, 2, 128, True),
    (2, 576, 8, 2, 128, True),
    (1, 1, 2, 1, 64, True),
    (1, 65, 2, 2, 128, True),      # one key in the second tile
    (2, 264, 4, 2, 64, True),      # fused dK+dV grid of 8 blocks
]
REGIMES = ["flat", "peaked"]
# the older inputs of the per-kernel files, on their shapes
SPECIAL = [
    ("straddle", (1, 256, 1, 1, 128, True)),
    ("spiked256", (1, 256, 2, 2, 128, True)),
    ("spiked328", (1, 328, 2, 2, 128, True)),
]
PEAKED_STD = 3.0
PLANTED_SCORE = 30.0


def _randn(shape, seed, mul):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * mul


def inputs(B, S, Hq, Hkv, D, causal=True, regime="flat", seed=0):
    """bf16 q, k, v, dout.

    flat       randn * 0.5: scaled scores of std 0.25, softmax near uniform.
    peaked     q and k are randn * sqrt(3): scaled scores of std 3. A
               Gaussian score 8 nats above the max of 64 others is a 5-sigma
               event that no seed of this size provides, so the LAST key
               is aligned with the last query row of (batch 0, head 0) to
               score PLANTED_SCORE: that row's max jumps in the last tile,
               and the key a ragged tail or a mask off by one would lose
               carries nearly all of that row's weight.
               ``tile_max_raises`` lets a test assert both kinds of tile
               transition from the fp64 scores.
    straddle, spiked256, spiked328   the inputs of test_attention_fwd_v4_gpu
               and test_attention_bwd_fused_gpu, requantised to bf16."""
    if regime == "straddle":
        c = torch.tensor([0.0, 2.5, 5.5, 5.5]).repeat_interleave(64)
        q = torch.full((B, S, Hq, D), 0.25)
        k = c.view(1, S, 1, 1).expand(B, S, Hkv, D).contiguous()
        v = _randn((B, S, Hkv, D), seed + 2, 0.5)
        do = _randn((B, S, Hq, D), seed + 3, 0.5)
        return q16(q), q16(k), q16(v), q16(do)
    mul = math.sqrt(PEAKED_STD) if regime == "peaked" else 0.5
    q = q16(_randn((B, S, Hq, D), seed, mul))
    k = q16(_randn((B, S, Hkv, D), seed + 1, mul))
    v = q16(_randn((B, S, Hkv, D), seed + 2, 0.5))
    do = q16(_randn((B, S, Hq, D), seed + 3, 0.5))
    if regime == "peaked" and S > 1:
        qr = q[0, S - 1, 0].double()
        c = PLANTED_SCORE * math.sqrt(D) / float(qr.pow(2).sum())
        k[0, S - 1, 0] = q16(qr * c)
    elif regime == "spiked256":
        k[0, 230] = q16(k[0, 230].float() * 30.0)
        q[0, 240] = q16(q[0, 240].float() * 8.0)
    elif regime == "spiked328":
        k[0, 300] = q16(k[0, 300].float() * 30.0)
        q[0, 310] = q16(q[0, 310].float() * 8.0)
    return q, k, v, do


def _allowed(S, causal, mask_shift=0, drop_keys=()):
    i = torch.arange(S).view(S, 1)
    j = torch.arange(S).view(1, S)
    ok = (j <= i + mask_shift) if causal else torch.ones(S, S,
                                                         dtype=torch.bool)
    ok = ok | ((i == 0) & (j == 0) if causal else False)
    for d in drop_keys:
        ok = ok & (j != d)
    return ok


def scores(q, k, causal):
    """fp64 scaled, masked scores [B,Hq,S,S]."""
    qh, kh = _heads(q, k)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(q.shape[-1])
    return s.masked_fill(~_allowed(q.shape[1], causal), float("-inf"))


def tile_max_raises(s: torch.Tensor) -> torch.Tensor:
    """By how many nats each 64-key tile after a row's first raises that
    row's running max; only the transitions that raise it are returned."""
    S = s.shape[-1]
    nt = n_tiles(S)
    pad = torch.full(s.shape[:-1] + (nt * BN - S,), float("-inf"),
                     dtype=s.dtype)
    tm = torch.cat([s, pad], -1).view(*s.shape[:-1], nt, BN).max(-1).values
    run = torch.cummax(tm, -1).values
    rise = run[..., 1:] - run[..., :-1]
    return rise[torch.isfinite(rise) & (rise > 0)]


def _heads(q, k, kv_roll=0):
    Hq, Hkv = q.shape[2], k.shape[2]
    hk = (torch.arange(Hq) // (Hq // Hkv) + kv_roll) % Hkv
    return f64(q).permute(0, 2, 1, 3), f64(k).permute(0, 2, 1, 3)[:, hk]


# --------------------------------------------------------------------------
# The reference
# --------------------------------------------------------------------------
def _compute(q, k, v, dout, causal, *, drop_keys=(), mask_shift=0,
             kv_roll=0, batch_swap_k=False, scale_mul=1.0, lse_log2=False,
             no_delta=False, group_short=False, dq_zero_rows=None,
             dv_unnormalised=False):
    """Plain fp64 attention forward and backward. The keyword switches build
    the deliberately wrong references of test_kernel_oracle_attention.py."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    sc = scale_mul / math.sqrt(D)
    ksrc = k.flip(0) if batch_swap_k else k
    qh, kh = _heads(q, ksrc, kv_roll)
    _, vh = _heads(q, v, kv_roll)
    do = f64(dout).permute(0, 2, 1, 3)
    ok = _allowed(S, causal, mask_shift, drop_keys)
    s = (qh @ kh.transpose(-1, -2) * sc).masked_fill(~ok, float("-inf"))
    M = s.max(-1, keepdim=True).values
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    o = p @ vh
    dP = do @ vh.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = p * (dP if no_delta else dP - delta)
    dq = sc * (dS @ kh)
    if dq_zero_rows is not None:
        dq[:, :, dq_zero_rows[0]:dq_zero_rows[1]] = 0.0
    pv = torch.exp(s - M) if dv_unnormalised else p
    g = rep - 1 if group_short else rep
    dk = sc * (dS.transpose(-1, -2) @ qh)
    dv = pv.transpose(-1, -2) @ do
    dk = dk.view(B, Hkv, rep, S, D)[:, :, :g].sum(2)
    dv = dv.view(B, Hkv, rep, S, D)[:, :, :g].sum(2)
    lse_out = lse.squeeze(-1)
    if lse_log2:
        lse_out = lse_out / math.log(2.0)
    out = {"o": o.permute(0, 2, 1, 3), "lse": lse_out,
           "dq": dq.permute(0, 2, 1, 3), "dk": dk.permute(0, 2, 1, 3),
           "dv": dv.permute(0, 2, 1, 3)}
    inter = dict(qh=qh, kh=kh, vh=vh, do=do, s=s, M=M, lse=lse, p=p, o=o,
                 dP=dP, delta=delta, dS=dS, sc=sc, rep=rep)
    return out, inter


def of_floats(q, k, v, dout, causal) -> dict:
    """``attention`` for float tensors, judged as the bf16 values a kernel
    is handed; dout = None leaves only the forward specs."""
    if dout is None:
        sp = attention(q16(q), q16(k), q16(v), torch.zeros_like(q16(q)),
                       causal)
        return {"o": sp["o"], "lse": sp["lse"]}
    return attention(q16(q), q16(k), q16(v), q16(dout), causal)


def wrong_reference(q, k, v, dout, causal, **wrong) -> dict:
    """The five outputs of a deliberately wrong computation (fp64)."""
    return _compute(q, k, v, dout, causal, **wrong)[0]


def attention(q, k, v, dout, causal) -> dict:
    """Specs of o [B,S,Hq,D], lse [B,Hq,S], dq [B,S,Hq,D], dk and dv
    [B,S,Hkv,D]; see the module docstring for every term."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    out, t = _compute(q, k, v, dout, causal)
    qh, kh, vh, do = t["qh"], t["kh"], t["vh"], t["do"]
    s, M, lse, p, o = t["s"], t["M"], t["lse"], t["p"], t["o"]
    dP, delta, dS, sc, rep = t["dP"], t["delta"], t["dS"], t["sc"], t["rep"]
    KS, KP = k_score(D), k_pv(S)
    live = torch.isfinite(s)
    zero = torch.zeros_like(s)

    sabs = (qh.abs() @ kh.abs().transpose(-1, -2)) * sc
    sbar = (p * sabs).sum(-1, keepdim=True)             # sum_j p_ij sabs_ij
    e_fwd = torch.where(live, 1 + (s - M).abs() + DEFER_THR, zero)
    A = (p * e_fwd).sum(-1, keepdim=True)

    # ---- LSE: fp32, absolute --------------------------------------------
    lse_parts = [(KS, sbar), (K_EXP, A),
                 (kred(35 * n_tiles(S)) + k_alpha(S), torch.ones_like(lse)),
                 (2, (lse - M).abs() + DEFER_THR),
                 (1, M.abs() + DEFER_THR), (1, lse.abs())]
    s_lse = _spec(lse.squeeze(-1), torch.zeros_like(lse.squeeze(-1)),
                  [(kc, x.squeeze(-1)) for kc, x in lse_parts], False)
    t_lse_units = (s_lse.k * s_lse.scale).unsqueeze(-1)   # units of 2^-23

    # ---- O ----------------------------------------------------------------
    mid_o = p @ vh.abs()
    # relative error of p_ij / l in units: own score and the normaliser's
    w_o = KS * (torch.where(live, sabs, zero) + sbar) + \
        K_EXP * (e_fwd + A) + KP
    o32 = (p * w_o) @ vh.abs()                            # units * |terms|
    s_o = AttnSpec(o, mid_o, o32 / (KS + K_EXP + KP), KS + K_EXP + KP, True)

    # ---- delta as attn_bwd_pre_kernel forms it -----------------------------
    d16 = (do * o).abs().sum(-1, keepdim=True) + \
        (p * dP.abs()).sum(-1, keepdim=True)
    d32 = (do.abs() * o32).sum(-1, keepdim=True) + \
        k_delta(D) * (do * o).abs().sum(-1, keepdim=True)

    # ---- p and dS in the backward kernels ----------------------------------
    a_bwd = torch.where(live, (s - lse).abs(), zero)
    pe_q = KS * torch.where(live, sabs, zero) + lse.abs() + \
        K_EXP * (1 + a_bwd) + t_lse_units
    pe_kv = pe_q + KS * lse.abs()                        # fused S accumulator
    dPabs = do.abs() @ vh.abs().transpose(-1, -2)
    dsrc = p * (k_dp(D) * (dPabs + delta.abs()) + d32)   # dP and delta errors
    mid_ds = dS.abs() + p * d16

    KQ, KK = k_sumq(S), k_sumk(S, rep)
    kq_tot = KS + K_EXP + 1 + KQ
    kk_tot = 2 * KS + K_EXP + 1 + KK

    def group(x):          # [B,Hq,S,D] -> [B,Hkv,S,D], summed over the group
        return x.view(B, Hkv, rep, S, D).sum(2)

    w_dq = dS.abs() * (pe_q + 1 + KQ) + dsrc
    s_dq = AttnSpec(out["dq"].permute(0, 2, 1, 3),
                    sc * (mid_ds @ kh.abs()),
                    sc * (w_dq @ kh.abs()) / kq_tot, kq_tot, True)
    w_dk = dS.abs() * (pe_kv + 1 + KK) + dsrc
    s_dk = AttnSpec(out["dk"].permute(0, 2, 1, 3),
                    group(sc * (mid_ds.transpose(-1, -2) @ qh.abs())),
                    group(sc * (w_dk.transpose(-1, -2) @ qh.abs())) / kk_tot,
                    kk_tot, True)
    w_dv = p * (pe_kv + KK)
    s_dv = AttnSpec(out["dv"].permute(0, 2, 1, 3),
                    group(p.transpose(-1, -2) @ do.abs()),
                    group(w_dv.transpose(-1, -2) @ do.abs()) / kk_tot,
                    kk_tot, True)

    def bshd(sp):
        return AttnSpec(sp.ref.permute(0, 2, 1, 3), sp.mid.permute(0, 2, 1, 3),
                        sp.scale.permute(0, 2, 1, 3), sp.k, sp.bf16)
    return {"o": bshd(s_o), "lse": s_lse, "dq": bshd(s_dq),
            "dk": bshd(s_dk), "dv": bshd(s_dv)}

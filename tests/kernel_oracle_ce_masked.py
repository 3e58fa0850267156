"""fp64 reference for the masked cross-entropy kernels, judged by
kernel_oracle's one rule. A row counts iff 0 <= label < V; the others add
nothing, get lse = 0 and a zero gradient and are never read (the reference
zeroes them, so they may hold NaN). n counted rows, l = logsumexp, z in fp32:
    loss    = sum[(l - x[label]) + z l^2] / n                  (0 if n = 0)
    dlogits = (p (1 + 2 z l) - onehot) * grad_out / n,  p = exp(x - l)

k, in units of 2^-23 * scale (see kernel_oracle), none fitted to output:
lse      ce_fwd_masked's sweep is ce_fwd's, element for element: k_lse and
         s_lse of kernel_oracle.cross_entropy, kred(8 ceil(V/2048) + 27) + 3.
loss     per row, l's error reaches l - x_label directly and z l^2 through
         2 z |l|: scale (s_lse + |x_label|) (1 + 2 z |l|) + z l^2. The
         subtraction, the z term's two products and the add of both parts
         are under 2 units of it: k_lse + 2. The fixed-order reduce: ceil(N/G)
         serial rows per block (G = min(N, 4096)), then ceil(G/1024) partials
         per finalize thread, 6 shuffle steps, 15 cross-wave adds and the
         division by the count: kred(ceil(N/G) + ceil(G/1024) + 22).
dlogits  kernel_oracle.cross_entropy's k_lse + 3, plus 1 for f = 1 + 2 z l
         (two roundings) and the product p * f; l's error also enters through
         f, times 2 z. Hence the scale
         |gs| (p ((1 + 2z|l|) (1 + |x - l| + s_lse) + 2 z s_lse) + onehot).
         p below 2^-126 is flushed before it meets f and gs.
"""
import math

import torch

import kernel_oracle as ko

IGNORE = -100


def masked_inputs(N, V, pattern):
    """'half', N > 600: a random half plus row 0, the last row and a run of
    300; smaller N: the even rows (row 0 and the last would be 'all' of N = 2)."""
    logits, labels = ko.ce_inputs(N, V)
    m = torch.rand(N, generator=torch.Generator().manual_seed(7)) < 0.5
    m[0] = m[-1] = True
    m[N // 3:N // 3 + 300] = True
    m = m if N > 600 else torch.arange(N) % 2 == 0
    labels[m if pattern == "half" else torch.full((N,), pattern == "all")] = \
        IGNORE
    return logits, labels


def cross_entropy_masked(logits, labels, grad_out=1.0, z=0.0) -> dict:
    N, V = logits.shape
    lab = labels.detach().cpu().long()
    valid = ((lab >= 0) & (lab < V)).view(-1, 1)
    x = ko.f64(logits).masked_fill(~valid, 0.0)
    z = ko._f32(z)
    inv = 1.0 / max(int(valid.sum()), 1)    # nothing counted: all is 0 anyway
    M = x.max(-1, keepdim=True).values
    lse = M + torch.log(torch.exp(x - M).sum(-1, keepdim=True))
    p = torch.exp(x - lse)
    safe = lab.clamp(0, V - 1).view(-1, 1)
    xl = x.gather(1, safe)
    k_lse = ko.kred(8 * math.ceil(V / 2048) + 27) + 3
    s_lse = M.abs() + (lse - M).abs() + \
        (p * (1 + (x - M).abs())).sum(-1, keepdim=True)
    sf = 1 + 2 * z * lse.abs()
    rows = (lse - xl) + z * lse * lse
    s_rows = (s_lse + xl.abs()) * sf + z * lse * lse
    gs = grad_out * inv
    onehot = torch.zeros_like(x).scatter_(1, safe, 1.0)
    dlog = (p * (1 + 2 * z * lse) - onehot) * gs
    s_d = abs(gs) * (p * (sf * (1 + (x - lse).abs() + s_lse) + 2 * z * s_lse)
                     + onehot)
    G = min(N, 4096)
    k_red = ko.kred(math.ceil(N / G) + math.ceil(G / 1024) + 22)

    def kept(t):            # ignored rows: reference 0, scale 0
        return t.masked_fill(~valid, 0.0)

    return {
        "lse": ko.Spec(kept(lse).view(-1), kept(s_lse).view(-1), k_lse, False),
        "loss": ko.Spec((kept(rows).sum() * inv).view(1),
                        (kept(s_rows).sum() * inv).view(1),
                        k_lse + 2 + k_red, False),
        "dlogits": ko.Spec(kept(dlog), kept(s_d), k_lse + 4, True,
                           ko.TINY * max(1.0, abs(gs) * float(sf.max()))),
    }

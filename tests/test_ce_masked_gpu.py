"""Masked cross-entropy kernels vs fp64 (kernel_oracle_ce_masked.py) at the
shapes of test_cross_entropy_oracle_gpu.py; V = 128256 is 4 backward segments."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ce_masked as kom
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

GRAD_OUT = 3.5
N1, V1, Z1 = 4100, 2056, 1e-4      # the cases that run at one size


def run(logits, labels, z, **kw):    # on a clone, for the in-place backward
    leaf = logits.to("cuda").requires_grad_(True)
    loss = ops.cross_entropy(leaf.clone(), labels.to("cuda"),
                             ignore_index=kom.IGNORE, z_loss=z, **kw)
    (loss * GRAD_OUT).backward()
    return {"loss": loss.detach().reshape(1), "dlogits": leaf.grad}


def same_bits(a, b):
    return all(torch.equal(a[n], b[n]) for n in a)


@pytest.mark.parametrize("z", [0.0, 1e-4, 0.5])
@pytest.mark.parametrize("pattern", ["none", "half", "all", "stray"])
@pytest.mark.parametrize("N,V", [(4100, 2056), (2, 128256)])
def test_masked_ce_vs_fp64(N, V, pattern, z):
    if pattern == "stray":      # >= 8 rows: each value at the flagship V too
        logits, labels = kom.masked_inputs(max(N, 8), V, "half")
        odd = torch.tensor([-1, V, V + 5, 2 ** 31 - 1])
        odd = torch.where(labels == kom.IGNORE,
                          odd[torch.arange(labels.numel()) // 2 % 4], labels)
        assert same_bits(run(logits, labels, z), run(logits, odd, z))
        return
    logits, labels = kom.masked_inputs(N, V, pattern)
    got = run(logits, labels, z)
    _, got["lse"], _, count = ops._C.ce_fwd_masked(
        logits.to("cuda"), labels.to("cuda").int(), z)
    assert int(count) == int((labels != kom.IGNORE).sum())
    ko.check_all(f"ce_masked[{N}x{V},{pattern},z={z}]", got,
                 kom.cross_entropy_masked(logits, labels, GRAD_OUT, z))
    if pattern == "all":
        assert got["loss"].item() == 0.0 and not got["dlogits"].any()


@pytest.mark.parametrize("case", ["dirty_rows", "inplace", "fp32_stray_labels"])
def test_same_bits_as_the_plain_call(case):
    logits, labels = kom.masked_inputs(N1, V1, "half")
    other, odd, kw = logits.clone(), labels.clone(), {}
    rows = torch.nonzero(labels == kom.IGNORE).flatten()
    if case == "inplace":
        kw = {"inplace_backward": True}
    elif case == "fp32_stray_labels":   # the eager GPU path checks no label
        logits = other = logits.float()     # on the host: it must not sync
        odd[rows] = -1
    else:
        other[rows[0::2]] = float("nan")    # never read, so nothing changes
        other[rows[1::2]] = float("inf")
    assert same_bits(run(logits, labels, Z1), run(other, odd, Z1, **kw))


def test_captured_pair_follows_new_labels():
    logits, labels = kom.masked_inputs(N1, V1, "half")
    _, other = kom.masked_inputs(N1, V1, "none")   # other mask and count
    lg = logits.to("cuda").requires_grad_(True)
    lab = labels.to("cuda")

    def step():
        lg.grad = None
        loss = ops.cross_entropy(lg, lab, ignore_index=kom.IGNORE, z_loss=Z1)
        (loss * GRAD_OUT).backward()
        return loss.detach().reshape(1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                           # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    for want in (other, labels, other):
        lab.copy_(want.to("cuda"))
        graph.replay()
        assert same_bits({"loss": loss, "dlogits": lg.grad},
                         run(logits, want, Z1))


def test_defaults_take_the_unmasked_kernels():
    logits, labels = ko.ce_inputs(N1, V1)
    lg = logits.to("cuda").requires_grad_(True)
    lab = labels.to("cuda").int()
    loss = ops.cross_entropy(lg, lab.long())
    (loss * GRAD_OUT).backward()
    loss_rows, lse = ops._C.ce_fwd(lg.detach(), lab)
    assert torch.equal(loss.detach(), loss_rows.mean())
    gscale = torch.tensor(GRAD_OUT, device="cuda") / lg.numel() * V1
    assert torch.equal(lg.grad, ops._C.ce_bwd(lg.detach(), lab, lse, gscale))

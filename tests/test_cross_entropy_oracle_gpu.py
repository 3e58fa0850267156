"""Fused cross-entropy kernels vs fp64 where their loops actually loop:
rows past the 4096-block forward grid, a column sweep of 256+1 vectors,
the backward grid stride, and the flagship vocabulary (62.6 sweeps per
row). Labels sit at 0, at V-1 and inside the ragged last vector; one row
spreads its logits over +-80; the upstream gradient is not 1. Labels
outside [0, V) are not part of the kernel's contract and are not fed.
Rule, references and k: kernel_oracle.py."""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_OUT = 3.5


@pytest.mark.parametrize("N,V", [(4100, 2056), (2, 128256)])
def test_cross_entropy_vs_fp64(N, V):
    logits, labels = ko.ce_inputs(N, V)
    specs = ko.cross_entropy(logits, labels, GRAD_OUT)

    lg = logits.to(DEV)
    loss_rows, lse = ops._C.ce_fwd(lg, labels.to(DEV).int())
    lg.requires_grad_(True)
    loss = ops.cross_entropy(lg, labels.to(DEV))
    (loss * GRAD_OUT).backward()

    ko.check_all(f"ce[{N}x{V}]",
                 {"lse": lse, "loss_rows": loss_rows,
                  "loss": loss.reshape(1), "dlogits": lg.grad}, specs)
    # the gradient at every label is negative, everywhere else positive
    gr = lg.grad.float().cpu()
    at_label = gr.gather(1, labels.view(-1, 1))
    assert (at_label < 0).all()
    assert (gr >= 0).sum() == N * V - N

"""Fused SwiGLU kernels vs fp64, forward and backward: 16388 rows stride
the 16384-row grid cap; I = 2056 needs a second, ragged column block; the
gates of row 0 reach +-30, where exp(-g) spans 26 decades.
Rule, references and k: kernel_oracle.py."""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("rows,I", [(16388, 128), (5, 2056)])
def test_swiglu_vs_fp64(rows, I):
    gu, dout = ko.swiglu_inputs(rows, I)
    gg = gu.to(DEV).requires_grad_(True)
    out = ops.swiglu(gg)
    out.backward(dout.to(DEV))
    ko.check_all(f"swiglu[{rows}x{I}]", {"out": out, "dgu": gg.grad},
                 ko.swiglu(gu, dout))

"""Single-token attention decode vs fp64 (it had no numerics test): T
below, at and above the kernel's 8 waves, NaN in every cache row it must
not read, GQA, one dominant key, and the device-side T of the captured
decode step. Rule, references and k: kernel_oracle.py."""
import pytest
import torch

import kernel_oracle as ko
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5, 8, 9, 100])
def test_attention_decode_vs_fp64(T, D):
    B, Hq, Hkv = 2, 8, 2
    q, kc, vc = ko.decode_inputs(B, T, Hq, Hkv, D)   # rows >= T are NaN
    spec = ko.attention_decode(q, kc, vc, T)
    # the planted key takes (nearly) all the weight in its heads
    assert (spec.ref[:, 0] - vc[:, T // 2, 0].double()).abs().max() < \
        (0.05 if T > 1 else 1e-12)

    qg, kg, vg = q.to(DEV), kc.to(DEV), vc.to(DEV)
    out = ops.attention_decode(qg, kg, vg, T)
    assert torch.isfinite(out.float()).all()
    ko.check(f"decode[T={T},D={D}]", out, spec)

    # hipGraph replay passes T on the device and a host T of 0
    t_dev = torch.tensor(T, dtype=torch.int32, device=DEV)
    out_dev = ops.attention_decode(qg, kg, vg, 0, T_dev=t_dev)
    assert torch.equal(out_dev, out)

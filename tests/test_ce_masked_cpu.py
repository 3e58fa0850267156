"""Masked cross-entropy without a GPU: the CPU path of ops.cross_entropy vs
kernel_oracle_ce_masked, and the trainer's document-end mask on llama-tiny."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_ce_masked as kom
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext


@pytest.mark.parametrize("z", [0.0, 1e-4, 0.5])
@pytest.mark.parametrize("pattern", ["none", "half", "all"])
@pytest.mark.parametrize("N,V", [(70, 2056), (2, 16392)])
def test_cpu_path_vs_fp64(N, V, pattern, z):
    logits, labels = kom.masked_inputs(N, V, pattern)
    logits[labels == kom.IGNORE] = float("nan")     # such rows are not read
    ll = logits.clone().requires_grad_(True)
    loss = ops.cross_entropy(ll, labels, ignore_index=kom.IGNORE, z_loss=z)
    (loss * 3.5).backward()
    ko.check_all(f"cpu.ce_masked[{N}x{V},{pattern},z={z}]",
                 {"loss": loss.reshape(1), "dlogits": ll.grad},
                 kom.cross_entropy_masked(logits, labels, 3.5, z))
    if pattern == "all":
        assert loss.item() == 0.0 and not ll.grad.any()
    labels[1] = -1                      # a stray label raises on CPU tensors
    with pytest.raises(ValueError):
        ops.cross_entropy(ll, labels, ignore_index=kom.IGNORE, z_loss=z)


def test_trainer_masks_labels_at_document_ends():
    EOS = 7
    with pytest.raises(ValueError):
        TrainerConfig(mask_doc_end_labels=True)      # needs doc_eos_id
    tr = Trainer(TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=32,
                               doc_eos_id=EOS, mask_doc_end_labels=True),
                 DistContext())
    inp, lab = (t.clone() for t in tr.data.batch(0))
    inp[0, 5] = inp[0, 20] = inp[1, 31] = EOS
    other = torch.where(inp == EOS, (lab + 11) % tr.model_cfg.vocab_size, lab)

    def run(labels):
        tr.fb.zero_grads()
        loss = tr._loss(inp, labels)
        loss.backward()
        return [loss.detach()] + [b.flat_grad.clone() for b in tr.fb.buckets]

    assert all(torch.equal(x, y) for x, y in zip(run(lab), run(other)))

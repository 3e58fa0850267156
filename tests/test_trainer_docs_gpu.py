"""Packed-document training end to end on the GPU: llama-tiny reading a token
file, with document bounds derived inside the step, captured (hip_graph) and
eager.

A fresh graph trainer's first train_step() runs three optimizer steps (two
warm-up steps on a side stream, then the first replay), so the runs are
lined up by step_count. The graph and eager runs are held together by the
criterion of test_trainer_graph_knobs_gpu.py: they may differ by at most
twice what graph and eager differ by without the feature, on the same file
(0 demands bit equality)."""
import numpy as np
import pytest
import torch

from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.parallel.env import DistContext

pytestmark = pytest.mark.gpu

EOS = 0
STEPS = 3


@pytest.fixture(scope="module")
def token_file(tmp_path_factory):
    """Documents of 5..90 tokens, EOS-terminated, packed end to end."""
    rng = np.random.default_rng(0)
    toks = rng.integers(1, 512, 24 * 129)
    ends = np.cumsum(rng.integers(5, 91, 400))
    toks[ends[ends < len(toks)]] = EOS
    path = tmp_path_factory.mktemp("data") / "tokens.bin"
    toks.astype("<u2").tofile(path)
    return str(path)


def _trainer(path, **kw):
    torch.cuda.set_device(0)
    cfg = TrainerConfig(model="llama-tiny", micro_batch=2, seq_len=128,
                        data_path=path, **kw)
    return Trainer(cfg, DistContext(device=torch.device("cuda", 0)))


def _run(tr):
    losses = []
    while tr.step_count < STEPS:
        losses.append(tr.train_step(sync=False).clone())
    assert tr.step_count == STEPS
    return losses, [b.flat_param.clone() for b in tr.fb.buckets]


def _max_diff(pa, pb):
    return max((a.float() - b.float()).abs().max().item()
               for a, b in zip(pa, pb))


def test_graph_and_eager_agree_and_the_mask_is_in_the_step(token_file):
    _, g0 = _run(_trainer(token_file, hip_graph=True))
    l_plain, e0 = _run(_trainer(token_file))
    d_plain = _max_diff(g0, e0)

    lg, g1 = _run(_trainer(token_file, hip_graph=True, doc_eos_id=EOS))
    le, e1 = _run(_trainer(token_file, doc_eos_id=EOS))
    d_docs = _max_diff(g1, e1)
    print(f"d_plain {d_plain:.3e}  d_docs {d_docs:.3e}")
    assert d_docs <= 2 * d_plain
    # the graph's one call returns step 3's loss, the eager run's last
    assert len(lg) == 1 and len(le) == STEPS
    assert torch.isfinite(lg[0]) and all(torch.isfinite(x) for x in le)
    # same file, same init, same batches: the bounds change every loss
    for a, b in zip(le, l_plain):
        assert a.item() != b.item()
    assert _max_diff(e1, e0) > 0


def test_batches_hold_document_boundaries(token_file):
    tr = _trainer(token_file, doc_eos_id=EOS)
    inp, _ = tr.data.batch(0)
    assert inp.is_cuda and (inp == EOS).sum().item() >= 2

"""Packed-document training above the kernels, on the CPU: the token file,
the model plumbing (mask and RoPE restart together, also through activation
checkpointing), the trainer fields and the refusals."""
import json

import numpy as np
import pytest
import torch

from torch_on_k8s_amd import ops
from torch_on_k8s_amd.engine.data import PackedTokenFile
from torch_on_k8s_amd.engine.trainer import Trainer, TrainerConfig
from torch_on_k8s_amd.models import llama
from torch_on_k8s_amd.models.registry import build_model, get_model_config
from torch_on_k8s_amd.parallel.env import DistContext

EOS = 0


# --------------------------------------------------------------------------
# PackedTokenFile
# --------------------------------------------------------------------------
def write_tokens(path, n, dtype, vocab=512, seed=0, eos_every=None):
    rng = np.random.default_rng(seed)
    toks = rng.integers(1, vocab, n)
    if eos_every:
        pos = np.cumsum(rng.integers(3, eos_every, n // 3))
        toks[pos[pos < n]] = EOS
    toks.astype({"uint16": "<u2", "uint32": "<u4"}[dtype]).tofile(path)
    return toks


@pytest.mark.parametrize("dtype", ["uint16", "uint32"])
def test_packed_token_file_windows(tmp_path, dtype):
    S, mb = 16, 2
    vocab = 512 if dtype == "uint16" else 100000   # needs the wide type
    path = str(tmp_path / "tokens.bin")
    toks = write_tokens(path, 40 * (S + 1) + 5, dtype, vocab=vocab)
    cpu = torch.device("cpu")
    data = PackedTokenFile(path, dtype, mb, S, cpu, rank=0, world=1, seed=3)
    assert data.num_windows == 40
    inp, lab = data.batch(4)
    assert inp.shape == (mb, S) and lab.shape == (mb, S)
    assert inp.dtype == torch.long and inp.is_contiguous()
    assert torch.equal(inp[:, 1:], lab[:, :-1])          # shifted by one
    for i in range(mb):
        w = data.window_index(4, i) * (S + 1)
        assert inp[i].tolist() == toks[w:w + S].tolist()
        assert lab[i].tolist() == toks[w + 1:w + S + 1].tolist()
    # batch(step) repeats: same object, and a fresh one (resume)
    again = PackedTokenFile(path, dtype, mb, S, cpu, rank=0, world=1, seed=3)
    for step in (0, 4, 7):
        a, b = data.batch(step), again.batch(step)
        c = data.batch(step)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    if dtype == "uint32":
        assert int(toks.max()) > 65535 and int(inp.max()) <= int(toks.max())


def test_packed_token_file_ranks_read_disjoint_windows(tmp_path):
    S, mb, world, steps = 8, 2, 4, 5
    path = str(tmp_path / "tokens.bin")
    write_tokens(path, 64 * (S + 1), "uint16")
    seen = {}
    for rank in range(world):
        data = PackedTokenFile(path, "uint16", mb, S, torch.device("cpu"),
                               rank=rank, world=world, seed=11)
        for step in range(steps):
            for i in range(mb):
                w = data.window_index(step, i)
                assert w not in seen, (rank, step, i, seen[w])
                seen[w] = (rank, step, i)
    assert len(seen) == world * steps * mb <= 64
    # another world size covers the same windows in the same global order
    one = PackedTokenFile(path, "uint16", mb * world, S, torch.device("cpu"),
                          rank=0, world=1, seed=11)
    order = [one.window_index(0, i) for i in range(mb * world)]
    by_rank = [w for w, (r, s, i) in sorted(seen.items(),
                                            key=lambda kv: (kv[1][1], kv[1][0],
                                                            kv[1][2]))
               if s == 0]
    assert order == by_rank


def test_packed_token_file_rejects_bad_arguments(tmp_path):
    path = str(tmp_path / "tokens.bin")
    write_tokens(path, 10, "uint16")
    cpu = torch.device("cpu")
    with pytest.raises(ValueError):
        PackedTokenFile(path, "int8", 1, 4, cpu)
    with pytest.raises(ValueError):
        PackedTokenFile(path, "uint16", 1, 32, cpu)      # not one window
    with pytest.raises(ValueError):
        PackedTokenFile(path, "uint16", 1, 4, cpu, rank=2, world=2)


# --------------------------------------------------------------------------
# llama-tiny, packed row [A | B]
# --------------------------------------------------------------------------
LA, LB, S = 21, 27, 48


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    model = build_model(get_model_config("llama-tiny")).eval()
    g = torch.Generator().manual_seed(1)
    A = torch.randint(1, 512, (1, LA), generator=g)
    A[0, -1] = EOS
    B = torch.randint(1, 512, (1, LB), generator=g)
    A2 = torch.randint(1, 512, (1, LA), generator=g)
    A2[0, -1] = EOS
    filler = torch.randint(1, 512, (1, S - LB), generator=g)
    return model, A, B, A2, filler


def test_packed_row_equals_documents_on_their_own(tiny):
    model, A, B, A2, filler = tiny
    row = torch.cat([A, B], 1)
    ds, de = ops.doc_bounds(row, EOS)
    assert ds[0].tolist() == [0] * LA + [LA] * LB
    with torch.no_grad():
        packed = model(row, doc_start=ds, doc_end=de)
        plain = model(row)
        b_first = model(torch.cat([B, filler], 1))
        packed2 = model(torch.cat([A2, B], 1), doc_start=ds, doc_end=de)
        derived = model(row, doc_start=ds)
    # A is the row's first document: the mask changes nothing for it
    torch.testing.assert_close(packed[:, :LA], plain[:, :LA])
    # B, as if it stood at the start of a row of its own
    torch.testing.assert_close(packed[:, LA:], b_first[:, :LB])
    # and B really was looking at A without the bounds
    with pytest.raises(AssertionError):
        torch.testing.assert_close(plain[:, LA:], b_first[:, :LB])
    # nothing of A reaches B
    assert torch.equal(packed2[:, LA:], packed[:, LA:])
    assert not torch.equal(packed2[:, :LA], packed[:, :LA])
    assert torch.equal(derived, packed)


def _layer0_qk(model, monkeypatch, row, **bounds):
    """The roped q and k that the first layer hands to ops.attention."""
    seen = []
    real = ops.attention

    def spy(q, k, v, **kw):
        seen.append((q.detach().clone(), k.detach().clone()))
        return real(q, k, v, **kw)

    monkeypatch.setattr(llama.ops, "attention", spy)
    with torch.no_grad():
        logits = model(row, **bounds)
    monkeypatch.setattr(llama.ops, "attention", real)
    return seen[0], logits


def test_mask_without_rope_restart_is_caught(tiny, monkeypatch):
    """Teeth for the RoPE half of the plumbing: bounds given to attention but
    not to RoPE.

    At the logits this cannot show. RoPE scores depend on i - j alone, so a
    document whose phases are all counted from the row start has, in exact
    arithmetic, the scores it has when they are counted from its own first
    token; with the mask in place B's logits are then the same function of
    B's tokens either way (measured here: max |diff| 7e-7 against logits
    of size 1, inside assert_close's fp32 defaults). What the restart
    changes is the phase itself: the q and k rows that reach attention. So
    the comparison of the test above (assert_close at fp32 defaults, B's
    rows of the packed row against the first L_B rows of [B | filler]) is
    made on the first layer's roped q and k. With the restart it holds;
    with the bounds kept from RoPE it must fail."""
    model, A, B, _, filler = tiny
    row = torch.cat([A, B], 1)
    ds, de = ops.doc_bounds(row, EOS)
    (q_own, k_own), b_first = _layer0_qk(model, monkeypatch,
                                         torch.cat([B, filler], 1))
    (q, k), packed = _layer0_qk(model, monkeypatch, row, doc_start=ds,
                                doc_end=de)
    torch.testing.assert_close(q[:, LA:], q_own[:, :LB])
    torch.testing.assert_close(k[:, LA:], k_own[:, :LB])

    real = ops.qkv_rope
    monkeypatch.setattr(llama.ops, "qkv_rope",
                        lambda *a, doc_start=None, **kw: real(*a, **kw))
    (q, k), masked_only = _layer0_qk(model, monkeypatch, row, doc_start=ds,
                                     doc_end=de)
    with pytest.raises(AssertionError):
        torch.testing.assert_close(q[:, LA:], q_own[:, :LB])
    with pytest.raises(AssertionError):
        torch.testing.assert_close(k[:, LA:], k_own[:, :LB])
    print("logits, restart vs row-start phases: max |diff| "
          f"{float((masked_only - packed)[:, LA:].abs().max()):.2e}")


def test_bounds_pass_through_activation_checkpointing(tiny):
    model, A, B, _, _ = tiny
    row = torch.cat([A, B], 1)
    lab = torch.roll(row, -1, 1)
    ds, de = ops.doc_bounds(row, EOS)
    ck = build_model(get_model_config("llama-tiny"),
                     activation_checkpointing=True)
    ck.load_state_dict(model.state_dict())
    grads = []
    for m in (model, ck):
        m.train()
        m.zero_grad()
        loss = m(row, lab, doc_start=ds, doc_end=de)
        loss.backward()
        grads.append((loss.detach(), m.layers[0].attn.qkv_proj.weight.grad))
    model.eval()
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])
    plain = model(row, lab)
    assert not torch.equal(plain.detach(), grads[0][0])


def test_sdpa_and_gpt2_refuse_bounds():
    row = torch.randint(1, 50, (1, 16))
    ds, de = ops.doc_bounds(row, EOS)
    sdpa = build_model(get_model_config("llama-tiny", attn_impl="sdpa"))
    with pytest.raises(NotImplementedError):
        sdpa(row, doc_start=ds, doc_end=de)
    gpt = build_model(get_model_config("gpt2-tiny"))
    with pytest.raises(NotImplementedError):
        gpt(row, doc_start=ds, doc_end=de)
    gpt(row)                                   # unchanged without bounds


# --------------------------------------------------------------------------
# Trainer
# --------------------------------------------------------------------------
def test_trainer_reads_the_file_and_masks_documents(tmp_path):
    path = str(tmp_path / "tokens.bin")
    write_tokens(path, 12 * 33, "uint16", eos_every=12)
    base = dict(model="llama-tiny", micro_batch=2, seq_len=32,
                data_path=path, data_dtype="uint16")
    # the fields travel as JSON, like the rest of the trainer config
    cfg = TrainerConfig(**json.loads(json.dumps(
        TrainerConfig(doc_eos_id=EOS, **base).to_dict())))
    assert cfg.data_path == path and cfg.doc_eos_id == EOS
    assert TrainerConfig().data_path is None
    assert TrainerConfig().data_dtype == "uint16"
    assert TrainerConfig().doc_eos_id is None

    ctx = DistContext()
    docs = Trainer(cfg, ctx)
    assert isinstance(docs.data, PackedTokenFile)
    inp, _ = docs.data.batch(0)
    assert (inp == EOS).any()                  # the batch holds boundaries
    plain = Trainer(TrainerConfig(**base), ctx)
    l_docs = [docs.train_step() for _ in range(2)]
    l_plain = [plain.train_step() for _ in range(2)]
    assert all(l == l for l in l_docs + l_plain)
    assert l_docs[0] != l_plain[0]             # same init, same batch
    # repeatable
    again = Trainer(cfg, ctx)
    assert [again.train_step() for _ in range(2)] == l_docs

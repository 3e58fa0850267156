"""generate_ragged(weight_dtype="mxfp4"): on the CPU the tokens are bitwise
those of a copy of the model whose projection weights are the dequantized
values (alone, with an fp8 KV cache, with chunked prefill); a changed weight is
requantized; the serve field passes through on ragged requests only; on the
GPU eager equals captured and both follow the fp32 reference over dequantized
weights as far as its margins allow.

Prompts are those of test_generate_chunked; the model seed is 12, not its 158:
the dequantized reference must meet the top-2 margin rule (>= 4 * 2^-7 *
max|logit| at the first two new tokens of every sequence), a condition on the
reference alone. Seed 158 misses it (smallest ratio 3.0), 12 has 5.1; the
fixture asserts it."""
import copy

import pytest
import torch

from test_generate_chunked import LENS, N_NEW, make_prompts
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.serve import InferenceServer, build_app

SEED = 12


def dequantized(model):
    """A deep copy whose five kinds of projection weight hold their MXFP4
    values."""
    ref = copy.deepcopy(model)
    ref.drop_quantized_weights()
    mods = [ref.lm_head] + [m for blk in ref.layers for m in (
        blk.attn.qkv_proj, blk.attn.o_proj, blk.mlp.gate_up_proj,
        blk.mlp.down_proj)]
    with torch.no_grad():
        for m in mods:
            m.weight.copy_(ops.dequant_mxfp4(
                *ops.quantize_weight_mxfp4(m.weight)))
    return ref


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(SEED)
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).bfloat16().float().eval()
    prompts = make_prompts(cfg.vocab_size)
    ref = dequantized(model)
    want = ref.generate_ragged(prompts, max_new_tokens=N_NEW)
    margins, logits = [], []
    with torch.no_grad():
        for b, w in enumerate(want):
            lg = ref(w[None])[0, LENS[b] - 1:-1]
            top = lg.topk(2, -1).values
            assert (top[:2, 0] - top[:2, 1] >=
                    4 * 2.0 ** -7 * lg[:2].abs().amax(-1)).all()
            margins.append((top[:, 0] - top[:, 1]).tolist())
            logits.append(lg)
    return model, ref, prompts, want, margins, logits


@pytest.mark.parametrize("kw", [{}, {"kv_dtype": "fp8"}, {"prefill_chunk": 5}],
                         ids=["alone", "kv_fp8", "chunked"])
def test_mxfp4_tokens_are_the_dequantized_models_cpu(case, kw):
    model, ref, prompts = case[:3]
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                weight_dtype="mxfp4", **kw)
    want = ref.generate_ragged(prompts, max_new_tokens=N_NEW, **kw)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), (got, want)


def test_mxfp4_validation_and_requantization(case):
    model, _, prompts = case[:3]
    with pytest.raises(ValueError, match="weight_dtype"):
        model.generate_ragged(prompts, weight_dtype="int4")
    with pytest.raises(ValueError, match="mxfp4"):
        ops.quantize_weight_mxfp4(torch.zeros(16, 48))
    model = copy.deepcopy(model)
    keys = set(model.state_dict())
    model.generate_ragged(prompts, max_new_tokens=2, weight_dtype="mxfp4")
    model.generate_ragged(prompts, max_new_tokens=2, weight_dtype="fp8")
    assert set(model.state_dict()) == keys
    with torch.no_grad():
        model.layers[0].mlp.down_proj.weight.mul_(-1.5)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                weight_dtype="mxfp4")
    want = dequantized(model).generate_ragged(prompts, max_new_tokens=N_NEW)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), (got, want)
    model.drop_quantized_weights()
    assert "_w8_cache" not in model.__dict__


def test_serve_passes_mxfp4_on_ragged_requests_only():
    from starlette.testclient import TestClient
    torch.manual_seed(0)
    srv = InferenceServer.from_preset("llama-tiny", "cpu")
    client = TestClient(build_app(srv))
    body = {"prompt_ids": [[1, 2, 3, 4, 5], [6, 7]], "max_new_tokens": 3}
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              weight_dtype="mxfp4"))
    assert r.status_code == 200, r.text
    want = srv.model.generate_ragged(body["prompt_ids"], max_new_tokens=3,
                                     weight_dtype="mxfp4")
    assert r.json()["output_ids"] == [t.tolist() for t in want]
    r = client.post("/v1/generate", json=dict(body, weight_dtype="mxfp4",
                                              prompt_ids=[[1, 2], [3, 4]]))
    assert r.status_code == 400 and "ragged" in r.json()["detail"]
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              weight_dtype="int4"))
    assert r.status_code == 400


@pytest.mark.gpu
def test_mxfp4_generation_gpu_eager_captured_and_reference(case):
    """As test_w8_generation_gpu_eager_captured_and_reference: a sequence is
    compared up to the first step whose reference margin is below 4e, e the
    largest logit difference between the bf16 GPU forward over the dequantized
    weights (exact in bf16) and the fp32 CPU forward over them, along the
    reference sequences."""
    ref_model, ref, prompts, want, margins, logits = case
    dev = torch.device("cuda", 0)

    def on_gpu(src):
        m = LlamaModel(src.cfg).bfloat16().eval()
        m.load_state_dict({k: v.bfloat16() for k, v in src.state_dict().items()})
        return m.to(dev)

    deq = on_gpu(ref)
    with torch.no_grad():
        e = max(float((deq(w[None].to(dev))[0, LENS[b] - 1:-1].float().cpu()
                       - logits[b]).abs().max()) for b, w in enumerate(want))
    model = on_gpu(ref_model)
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  weight_dtype="mxfp4", use_graph=False)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  weight_dtype="mxfp4", use_graph=True)
    print(f"W4_GEN e={e:.5f} 4e={4 * e:.5f}")
    for b, (g, c, w) in enumerate(zip(eager, graph, want)):
        assert torch.equal(g, c), (b, g, c)
        n = 0
        while n < N_NEW and margins[b][n] >= 4 * e:
            n += 1
        print(f"W4_GEN seq{b}: compared={n}")
        assert n >= 2, (b, margins[b], e)
        assert torch.equal(g.cpu()[:LENS[b] + n], w[:LENS[b] + n]), (b, g, w)

"""generate_ragged(kv_dtype="fp8_paged") on llama-tiny (prompt 70 crosses a
page in prefill, 63 during decode): the tokens are those of kv_dtype="fp8"
(the same quantized rows, the same math), greedy and sampled; chunked prefill
over the quantized cache does not depend on the chunk size (it is not
compared with the padded prefill, which attends to unquantized k / v); the
pool holds exactly kv_pages_needed pages; the serve field is accepted on a
ragged request only; on the GPU eager equals captured and the first new token
is the bf16 run's."""
import pytest
import torch

from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.serve import InferenceServer, build_app

LENS = [5, 70, 63, 1]
N_NEW = 8


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(171)
    cfg = get_config("llama-tiny")
    g = torch.Generator().manual_seed(1171)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g)
               for n in LENS]
    return LlamaModel(cfg).bfloat16().float().eval(), prompts


@pytest.mark.parametrize("extra", [{}, {"temperature": 0.8, "top_k": 20,
                                        "seed": 7}])
def test_fp8_paged_tokens_equal_fp8(tiny, extra):
    model, prompts = tiny
    want = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                 kv_dtype="fp8", **extra)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                kv_dtype="fp8_paged", **extra)
    for g, w in zip(got, want):
        assert torch.equal(g, w), (g, w)
    assert model._kv_pool_pages == ops.kv_pages_needed(LENS, N_NEW) == 6


def test_chunked_prefill_does_not_depend_on_the_chunk(tiny):
    model, prompts = tiny
    a, b = (model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_dtype="fp8_paged", kv_page_size=64,
                                  prefill_chunk=n) for n in (5, 128))
    for n, x, y in zip(LENS, a, b):
        assert x.numel() == n + N_NEW and torch.equal(x, y), (x, y)


def test_serve_accepts_fp8_paged_on_ragged_requests_only():
    from starlette.testclient import TestClient
    torch.manual_seed(0)
    srv = InferenceServer.from_preset("llama-tiny", "cpu")
    client = TestClient(build_app(srv))
    body = {"prompt_ids": [[1, 2, 3, 4, 5], [6, 7]], "max_new_tokens": 3,
            "kv_dtype": "fp8_paged"}
    for extra in ({}, {"prefill_chunk": 2}):
        r = client.post("/v1/generate", json=dict(body, ragged=True, **extra))
        assert r.status_code == 200, r.text
        want = srv.model.generate_ragged(body["prompt_ids"], max_new_tokens=3,
                                         kv_dtype="fp8_paged", **extra)
        assert r.json()["output_ids"] == [t.tolist() for t in want]
    r = client.post("/v1/generate", json=dict(body, prompt_ids=[[1, 2],
                                                               [3, 4]]))
    assert r.status_code == 400 and "ragged" in r.json()["detail"]


@pytest.mark.gpu
def test_fp8_paged_generation_gpu_eager_equals_captured(tiny):
    ref, prompts = tiny
    dev = torch.device("cuda", 0)
    model = LlamaModel(ref.cfg).bfloat16().eval()
    model.load_state_dict({k: v.bfloat16()
                           for k, v in ref.state_dict().items()})
    model = model.to(dev)
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_dtype="fp8_paged", use_graph=False)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_dtype="fp8_paged", use_graph=True)
    bf16 = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                 use_graph=False)
    for n, e, g, w in zip(LENS, eager, graph, bf16):
        assert e.numel() == n + N_NEW and torch.equal(e, g), (e, g)
        assert torch.equal(e[:n + 1], w[:n + 1]), (e, w)

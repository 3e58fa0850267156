"""generate_ragged(kv_page_size=64) on llama-tiny: the paged run's tokens are
the unpaged run's (padded and chunked prefill, greedy and sampled; prompt 70
crosses a page in prefill, 63 during decode), the pool holds exactly
kv_pages_needed pages, the argument is validated, the serve field is passed
through on a ragged request and refused otherwise; on the GPU eager equals
captured and the first new token is the unpaged run's."""
import pytest
import torch

from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.serve import InferenceServer, build_app

LENS = [5, 70, 63, 1]
N_NEW = 8


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(164)
    cfg = get_config("llama-tiny")
    g = torch.Generator().manual_seed(1164)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g)
               for n in LENS]
    return LlamaModel(cfg).bfloat16().float().eval(), prompts


@pytest.mark.parametrize("extra", [{}, {"prefill_chunk": 5},
                                   {"temperature": 0.8, "top_k": 20,
                                    "seed": 7}])
def test_paged_tokens_equal_unpaged(tiny, extra):
    model, prompts = tiny
    want = model.generate_ragged(prompts, max_new_tokens=N_NEW, **extra)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                kv_page_size=64, **extra)
    for g, w in zip(got, want):
        assert torch.equal(g, w), (g, w)
    assert ops.kv_pages_needed(LENS, N_NEW) == 1 + 2 + 2 + 1
    assert model._kv_pool_pages == 6


def test_kv_page_size_is_validated(tiny):
    model, prompts = tiny
    with pytest.raises(ValueError, match="kv_page_size"):
        model.generate_ragged(prompts, kv_page_size=16)
    with pytest.raises(ValueError, match="kv_dtype"):
        model.generate_ragged(prompts, kv_page_size=64, kv_dtype="fp8")


def test_serve_passes_kv_page_size_on_ragged_requests_only():
    from starlette.testclient import TestClient
    torch.manual_seed(0)
    srv = InferenceServer.from_preset("llama-tiny", "cpu")
    client = TestClient(build_app(srv))
    body = {"prompt_ids": [[1, 2, 3, 4, 5], [6, 7]], "max_new_tokens": 3}
    seen = {}
    real = srv.model.generate_ragged

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)

    srv.model.generate_ragged = spy
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              kv_page_size=64))
    assert r.status_code == 200, r.text
    assert seen["kv_page_size"] == 64
    want = real(body["prompt_ids"], max_new_tokens=3, kv_page_size=64)
    assert r.json()["output_ids"] == [t.tolist() for t in want]
    r = client.post("/v1/generate", json={
        "prompt_ids": [[1, 2], [3, 4]], "max_new_tokens": 3,
        "kv_page_size": 64})
    assert r.status_code == 400 and "ragged" in r.json()["detail"]
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              kv_page_size=16))
    assert r.status_code == 400


@pytest.mark.gpu
def test_paged_generation_gpu_eager_equals_captured(tiny):
    ref, prompts = tiny
    dev = torch.device("cuda", 0)
    model = LlamaModel(ref.cfg).bfloat16().eval()
    model.load_state_dict({k: v.bfloat16()
                           for k, v in ref.state_dict().items()})
    model = model.to(dev)
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_page_size=64, use_graph=False)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_page_size=64, use_graph=True)
    plain = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  use_graph=False)
    for n, e, g, w in zip(LENS, eager, graph, plain):
        assert e.numel() == n + N_NEW and torch.equal(e, g), (e, g)
        assert torch.equal(e[:n + 1], w[:n + 1]), (e, w)

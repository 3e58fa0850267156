"""generate_ragged(kv_dtype="fp8") on llama-tiny: the CPU quantizer obeys the
cache format's bounds; the sequences have the right lengths and their first
new token is the bf16-cache run's (prefill does not read the cache); the
argument is validated; the serve field is passed through on a ragged request
and refused otherwise; on the GPU eager equals captured."""
import pytest
import torch

import kernel_oracle as ko
import kernel_oracle_fp8 as k8
from torch_on_k8s_amd import ops
from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.serve import InferenceServer, build_app

LENS = [5, 12, 9, 1]
N_NEW = 8


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(158)
    cfg = get_config("llama-tiny")
    g = torch.Generator().manual_seed(1158)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g)
               for n in LENS]
    return LlamaModel(cfg).bfloat16().float().eval(), prompts


@pytest.mark.parametrize("D", [64, 128])
def test_cpu_quantizer_obeys_the_format(D):
    B, Tq, Hkv, Tmax = 3, 4, 2, 6
    k, v = ko.bf(B, Tq, Hkv, D, seed=1), ko.bf(B, Tq, Hkv, D, seed=2)
    k[1, 0, 1] = 0
    v[1, 1, 0, 3] = -9.0
    pos = torch.tensor([-4, 1, 4], dtype=torch.int32)
    qlens = torch.tensor([4, 3, 4], dtype=torch.int32)
    kc = torch.full((B, Tmax, Hkv, D), 0x55, dtype=torch.uint8).view(k8.F8)
    vc = kc.clone()
    ks, vs = torch.full((B, Tmax, Hkv), -1.0), torch.full((B, Tmax, Hkv), -1.0)
    ops.kv_quantize_append_(k, v, pos, qlens, kc, vc, ks, vs)
    at = pos.long().view(B, 1) + torch.arange(Tq).view(1, Tq)
    live = (torch.arange(Tq).view(1, Tq) < qlens.view(B, 1)) & (at >= 0) \
        & (at < Tmax)
    bi, ti = torch.nonzero(live, as_tuple=True)
    written = torch.zeros(B, Tmax, dtype=torch.bool)
    written[bi, at[bi, ti]] = True
    for x, c, s in ((k, kc, ks), (v, vc, vs)):
        assert (c.view(torch.uint8)[~written] == 0x55).all()
        assert (s[~written] == -1.0).all()
        k8.check_quantizer(
            x[bi, ti].reshape(-1, D),
            c.view(torch.uint8)[bi, at[bi, ti]].reshape(-1, D).view(k8.F8),
            s[bi, at[bi, ti]].reshape(-1))
    assert ks[1, 1, 1] == 0
    assert float(vs[1, 2, 0]) == pytest.approx(9.0 / 448, rel=2.0 ** -22)


def test_fp8_generation_lengths_and_first_token(tiny):
    model, prompts = tiny
    want = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW, kv_dtype="fp8")
    for n, g, w in zip(LENS, got, want):
        assert g.numel() == n + N_NEW
        assert torch.equal(g[:n + 1], w[:n + 1]), (g, w)


def test_kv_dtype_is_validated(tiny):
    model, prompts = tiny
    with pytest.raises(ValueError, match="chunked prefill"):
        model.generate_ragged(prompts, kv_dtype="fp8", prefill_chunk=4)
    with pytest.raises(ValueError, match="kv_dtype"):
        model.generate_ragged(prompts, kv_dtype="int4")


def test_serve_passes_kv_dtype_on_ragged_requests_only():
    from starlette.testclient import TestClient
    torch.manual_seed(0)
    srv = InferenceServer.from_preset("llama-tiny", "cpu")
    client = TestClient(build_app(srv))
    body = {"prompt_ids": [[1, 2, 3, 4, 5], [6, 7]], "max_new_tokens": 3}
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              kv_dtype="fp8"))
    assert r.status_code == 200, r.text
    want = srv.model.generate_ragged(body["prompt_ids"], max_new_tokens=3,
                                     kv_dtype="fp8")
    assert r.json()["output_ids"] == [t.tolist() for t in want]
    r = client.post("/v1/generate", json={
        "prompt_ids": [[1, 2], [3, 4]], "max_new_tokens": 3,
        "kv_dtype": "fp8"})
    assert r.status_code == 400 and "ragged" in r.json()["detail"]
    r = client.post("/v1/generate", json=dict(body, ragged=True,
                                              kv_dtype="int4"))
    assert r.status_code == 400


@pytest.mark.gpu
def test_fp8_generation_gpu_eager_equals_captured(tiny):
    ref, prompts = tiny
    dev = torch.device("cuda", 0)
    model = LlamaModel(ref.cfg).bfloat16().eval()
    model.load_state_dict({k: v.bfloat16()
                           for k, v in ref.state_dict().items()})
    model = model.to(dev)
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_dtype="fp8", use_graph=False)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  kv_dtype="fp8", use_graph=True)
    bf16 = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                 use_graph=False)
    for n, e, g, w in zip(LENS, eager, graph, bf16):
        assert e.numel() == n + N_NEW and torch.equal(e, g), (e, g)
        assert torch.equal(e[:n + 1], w[:n + 1]), (e, w)

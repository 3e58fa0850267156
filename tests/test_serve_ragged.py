"""/v1/generate with "ragged": true: prompts of different lengths in one
request, per-sequence results, per-prompt context cap, eos validation; and
the same request without the flag is still refused."""
import pytest
import torch

from torch_on_k8s_amd.serve import InferenceServer, build_app

PROMPTS = [[1, 2, 3, 4, 5], [6, 7], [8, 9, 10]]


@pytest.fixture(scope="module")
def srv():
    torch.manual_seed(0)
    return InferenceServer.from_preset("llama-tiny", "cpu")


@pytest.fixture(scope="module")
def client(srv):
    from starlette.testclient import TestClient
    return TestClient(build_app(srv))


def test_ragged_request_matches_generate_ragged(srv, client):
    r = client.post("/v1/generate", json={
        "prompt_ids": PROMPTS, "max_new_tokens": 5, "ragged": True})
    assert r.status_code == 200, r.text
    out = r.json()
    want = [t.tolist() for t in
            srv.model.generate_ragged(PROMPTS, max_new_tokens=5)]
    assert out["output_ids"] == want
    assert out["new_ids"] == [w[len(p):] for w, p in zip(want, PROMPTS)]
    assert [len(o) for o in out["output_ids"]] == [10, 7, 8]
    assert out["new_tokens"] == 15

    # eos: the true count of new tokens is reported
    eos = want[1][len(PROMPTS[1]) + 1]        # sequence 1's second new token
    r = client.post("/v1/generate", json={
        "prompt_ids": PROMPTS, "max_new_tokens": 5, "ragged": True,
        "eos_token_id": eos})
    assert r.status_code == 200, r.text
    out = r.json()
    want_eos = [t.tolist() for t in srv.model.generate_ragged(
        PROMPTS, max_new_tokens=5, eos_token_id=eos)]
    assert out["output_ids"] == want_eos
    assert out["new_ids"][1][-1] == eos and len(out["new_ids"][1]) <= 2
    assert out["new_tokens"] == sum(len(n) for n in out["new_ids"]) < 15


def test_without_the_flag_unequal_prompts_are_still_refused(client):
    r = client.post("/v1/generate", json={
        "prompt_ids": PROMPTS, "max_new_tokens": 5})
    assert r.status_code == 400
    assert "share one length" in r.json()["detail"]
    r = client.post("/v1/generate", json={
        "prompt_ids": PROMPTS, "max_new_tokens": 5, "ragged": False})
    assert r.status_code == 400


def test_context_cap_applies_per_prompt(srv, client):
    max_seq = srv.meta["model_config"]["max_seq_len"]
    r = client.post("/v1/generate", json={
        "prompt_ids": [[1, 2], [1] * (max_seq - 4)], "max_new_tokens": 16,
        "ragged": True})
    assert r.status_code == 400 and "context" in r.json()["detail"]
    # exactly at the limit is allowed
    r = client.post("/v1/generate", json={
        "prompt_ids": [[1, 2], [1] * (max_seq - 2)], "max_new_tokens": 2,
        "ragged": True})
    assert r.status_code == 200, r.text


def test_ragged_request_validation(srv, client):
    vocab = srv.meta["model_config"]["vocab_size"]
    base = {"prompt_ids": PROMPTS, "max_new_tokens": 2, "ragged": True}
    assert client.post("/v1/generate", json=dict(
        base, eos_token_id=vocab)).status_code == 400
    assert client.post("/v1/generate", json=dict(
        base, eos_token_id=-1)).status_code == 400
    assert client.post("/v1/generate", json=dict(
        base, eos_token_id=vocab - 1)).status_code == 200
    assert client.post("/v1/generate", json=dict(
        base, prompt_ids=[[1, 2], []])).status_code == 400
    assert client.post("/v1/generate", json=dict(
        base, prompt_ids=[[1, 2], [vocab]])).status_code == 400

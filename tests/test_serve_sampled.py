"""/v1/generate with "ragged": true and temperature / top_k / top_p / seed:
the request reaches generate_ragged, the response carries the seed that was
used, and sampling controls without the flag are refused."""
import pytest
import torch

from torch_on_k8s_amd.serve import InferenceServer, build_app

PROMPTS = [[1, 2, 3, 4, 5], [6, 7], [8, 9, 10]]
SAMPLE = {"temperature": 0.8, "top_k": 50, "top_p": 0.95}


@pytest.fixture(scope="module")
def srv():
    torch.manual_seed(0)
    return InferenceServer.from_preset("llama-tiny", "cpu")


@pytest.fixture(scope="module")
def client(srv):
    from starlette.testclient import TestClient
    return TestClient(build_app(srv))


def post(client, **kw):
    body = {"prompt_ids": PROMPTS, "max_new_tokens": 5, "ragged": True}
    body.update(kw)
    return client.post("/v1/generate", json=body)


def test_sampled_request_matches_generate_ragged(srv, client):
    r = post(client, seed=1234, **SAMPLE)
    assert r.status_code == 200, r.text
    out = r.json()
    assert out["seed"] == 1234
    want = [t.tolist() for t in srv.model.generate_ragged(
        PROMPTS, max_new_tokens=5, seed=1234, **SAMPLE)]
    assert out["output_ids"] == want
    assert out["new_tokens"] == 15
    greedy = post(client).json()
    assert greedy["seed"] is None
    assert greedy["output_ids"] != want
    # the same request again
    assert post(client, seed=1234, **SAMPLE).json()["output_ids"] == want
    assert post(client, seed=1235, **SAMPLE).json()["output_ids"] != want


def test_returned_seed_reproduces_the_call(client):
    first = post(client, **SAMPLE).json()
    assert isinstance(first["seed"], int)
    again = post(client, seed=first["seed"], **SAMPLE).json()
    assert again["output_ids"] == first["output_ids"]
    assert again["seed"] == first["seed"]
    assert post(client, **SAMPLE).json()["seed"] != first["seed"]


def test_out_of_range_controls_are_refused(client):
    for bad in ({"top_p": 0.0}, {"top_p": 1.5}, {"top_p": -0.1},
                {"top_k": -1}, {"seed": 2 ** 63}):
        r = post(client, temperature=0.8, **bad)
        assert r.status_code == 400, (bad, r.status_code)
    assert post(client, temperature=0.8, top_p=1.0, top_k=0).status_code == 200


def test_sampling_controls_need_ragged(client):
    same_len = [[1, 2, 3], [4, 5, 6]]
    for ctl in ({"top_k": 5}, {"top_p": 0.9}, {"seed": 1}):
        r = client.post("/v1/generate", json=dict(
            {"prompt_ids": same_len, "max_new_tokens": 3, "temperature": 0.8},
            **ctl))
        assert r.status_code == 400, (ctl, r.status_code)
        assert "ragged" in r.json()["detail"]
    r = client.post("/v1/generate", json={
        "prompt_ids": same_len, "max_new_tokens": 3, "temperature": 0.8})
    assert r.status_code == 200, r.text

"""generate_ragged(prefill_chunk=N): prefill through the cache in chunks
gives the tokens of the padded prefill, whatever N, with eos and with a
seeded temperature; the serve field is passed through on a ragged request
and refused otherwise; on the GPU eager equals captured and both follow the
fp32 reference as far as its margins allow.

Model seed and prompts are those of test_generate_ragged.GPU_REF_SEED, chosen
there by the top-2 margin rule (>= 4 * 2^-7 * max|logit| at the first two
new tokens of every sequence); the margin is asserted on the reference here."""
import pytest
import torch

from torch_on_k8s_amd.models.llama import LlamaModel, get_config
from torch_on_k8s_amd.serve import InferenceServer, build_app

SEED = 158
LENS = [5, 12, 9, 1]
S0, N_NEW = max(LENS), 6


def make_prompts(vocab):
    g = torch.Generator().manual_seed(SEED + 1000)
    return [torch.randint(0, vocab, (n,), generator=g) for n in LENS]


@pytest.fixture(scope="module")
def ref_case():
    """fp32 CPU model, prompts, padded-prefill tokens, per-step top-2 margins
    and logits of each prompt alone along its reference sequence."""
    torch.manual_seed(SEED)
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).bfloat16().float().eval()
    prompts = make_prompts(cfg.vocab_size)
    want = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    margins, logits = [], []
    with torch.no_grad():
        for b, w in enumerate(want):
            lg = model(w[None])[0, LENS[b] - 1:-1]          # [N_NEW, V]
            top = lg.topk(2, -1).values
            assert torch.equal(lg.argmax(-1), w[LENS[b]:])
            assert (top[:2, 0] - top[:2, 1] >=
                    4 * 2.0 ** -7 * lg[:2].abs().amax(-1)).all()
            margins.append((top[:, 0] - top[:, 1]).tolist())
            logits.append(lg)
    return model, prompts, want, margins, logits


@pytest.mark.parametrize("chunk", [1, 3, 5, S0, S0 + 4])
def test_chunked_prefill_gives_the_padded_tokens_cpu(ref_case, chunk):
    model, prompts, want, _, _ = ref_case
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                prefill_chunk=chunk)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), (got, want)


@pytest.mark.parametrize("kw", [{"eos": True}, {"temperature": 0.8, "seed": 7}],
                         ids=["eos", "sampled"])
def test_chunked_prefill_with_eos_and_sampling_cpu(ref_case, kw):
    model, prompts, want, _, _ = ref_case
    if kw.pop("eos", False):
        kw = {"eos_token_id": int(want[1][LENS[1] + 2])}
    a = model.generate_ragged(prompts, max_new_tokens=N_NEW, **kw)
    b = model.generate_ragged(prompts, max_new_tokens=N_NEW, prefill_chunk=5,
                              **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)
    if "eos_token_id" in kw:
        assert len(a[1]) <= LENS[1] + 3


def test_prefill_chunk_zero_raises(ref_case):
    with pytest.raises(ValueError, match="prefill_chunk"):
        ref_case[0].generate_ragged(ref_case[1], prefill_chunk=0)


def test_serve_passes_prefill_chunk_on_ragged_requests_only():
    from starlette.testclient import TestClient
    torch.manual_seed(0)
    srv = InferenceServer.from_preset("llama-tiny", "cpu")
    client = TestClient(build_app(srv))
    body = {"prompt_ids": [[1, 2, 3, 4, 5], [6, 7]], "max_new_tokens": 3}
    r = client.post("/v1/generate",
                    json=dict(body, ragged=True, prefill_chunk=2))
    assert r.status_code == 200, r.text
    want = srv.model.generate_ragged(body["prompt_ids"], max_new_tokens=3,
                                     prefill_chunk=2)
    assert r.json()["output_ids"] == [t.tolist() for t in want]
    r = client.post("/v1/generate", json={
        "prompt_ids": [[1, 2], [3, 4]], "max_new_tokens": 3,
        "prefill_chunk": 2})
    assert r.status_code == 400 and "ragged" in r.json()["detail"]


@pytest.mark.gpu
def test_chunked_prefill_gpu_eager_captured_and_reference(ref_case):
    """As test_generate_ragged.test_ragged_gpu_vs_fp32_reference: a sequence
    is compared up to the first step whose reference margin is below 4e, e
    the largest logit difference between the bf16 GPU forward and the fp32
    CPU forward over the reference sequences."""
    ref_model, prompts, want, margins, logits = ref_case
    dev = torch.device("cuda", 0)
    model = LlamaModel(ref_model.cfg).bfloat16().eval()
    model.load_state_dict({k: v.bfloat16()
                           for k, v in ref_model.state_dict().items()})
    model = model.to(dev)
    with torch.no_grad():
        e = max(float((model(w[None].to(dev))[0, LENS[b] - 1:-1].float().cpu()
                       - logits[b]).abs().max()) for b, w in enumerate(want))
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  prefill_chunk=4, use_graph=False)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  prefill_chunk=4, use_graph=True)
    print(f"CHUNKED_GEN e={e:.5f} 4e={4 * e:.5f}")
    for b, (g, c, w) in enumerate(zip(eager, graph, want)):
        assert torch.equal(g, c), (b, g, c)
        n = 0
        while n < N_NEW and margins[b][n] >= 4 * e:
            n += 1
        print(f"CHUNKED_GEN seq{b}: compared={n}")
        assert n >= 2, (b, margins[b], e)
        assert torch.equal(g.cpu()[:LENS[b] + n], w[:LENS[b] + n]), (b, g, w)

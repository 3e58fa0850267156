"""Sampled ragged generation: temperature / top_k / top_p / seed on
LlamaModel.generate_ragged. The draw of a token depends on (row seed,
position in the sequence) alone, so a sequence does not care about its
batch slot, its neighbours, or whether a step ran eagerly or as a replay."""
import pytest
import torch

from torch_on_k8s_amd.models.llama import LlamaModel, get_config

LENS = [5, 12, 9, 1]
N_NEW = 8
SAMPLE = dict(temperature=0.8, top_k=50, top_p=0.95)


def make_prompts(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in LENS]


def naive_greedy(model, ids, n):
    out = ids
    for _ in range(n):
        out = torch.cat([out, model(out)[:, -1].argmax(-1, keepdim=True)], 1)
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def cpu_case():
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).eval()
    prompts = make_prompts(cfg.vocab_size, 1)
    with torch.no_grad():
        greedy = [naive_greedy(model, p[None], N_NEW)[0] for p in prompts]
    return model, prompts, greedy


def test_defaults_are_the_greedy_path_cpu(cpu_case):
    model, prompts, greedy = cpu_case
    assert same(model.generate_ragged(prompts, max_new_tokens=N_NEW), greedy)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                temperature=0.0, top_k=0, top_p=1.0, seed=5)
    assert same(got, greedy)


def test_seed_decides_the_tokens_cpu(cpu_case):
    model, prompts, greedy = cpu_case
    a = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11, **SAMPLE)
    b = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11, **SAMPLE)
    c = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=12, **SAMPLE)
    assert same(a, b)
    assert not same(a, c)
    assert not same(a, greedy)
    for g, p in zip(a, prompts):
        assert g.numel() == p.numel() + N_NEW
        assert torch.equal(g[:p.numel()], p)
    # no seed: one is drawn, and two calls differ
    d = model.generate_ragged(prompts, max_new_tokens=N_NEW, **SAMPLE)
    e = model.generate_ragged(prompts, max_new_tokens=N_NEW, **SAMPLE)
    assert not same(d, e)


def test_copies_of_one_prompt_diverge_cpu(cpu_case):
    model, prompts, _ = cpu_case
    a, b = model.generate_ragged([prompts[1], prompts[1]],
                                 max_new_tokens=N_NEW, seed=3, **SAMPLE)
    assert not torch.equal(a, b)
    # ... and agree when given one seed each
    a, b = model.generate_ragged([prompts[1], prompts[1]],
                                 max_new_tokens=N_NEW, seed=[3, 3], **SAMPLE)
    assert torch.equal(a, b)


def test_top_k_1_is_greedy_cpu(cpu_case):
    model, prompts, greedy = cpu_case
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                temperature=1.3, top_k=1, seed=4)
    assert same(got, greedy)
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                temperature=1.3, top_p=0.0, seed=4)
    assert same(got, greedy)


def test_batch_equals_each_prompt_alone_cpu(cpu_case):
    model, prompts, _ = cpu_case
    both = model.generate_ragged(prompts[:2], max_new_tokens=N_NEW, seed=21,
                                 **SAMPLE)
    for b in range(2):
        alone = model.generate_ragged([prompts[b]], max_new_tokens=N_NEW,
                                      seed=21 + b, **SAMPLE)
        assert torch.equal(both[b], alone[0]), (b, both[b], alone[0])
    # per-row parameters: a greedy row between sampled rows stays greedy
    mixed = model.generate_ragged(
        prompts[:3], max_new_tokens=N_NEW, seed=21,
        temperature=[0.8, 0.0, 1.2], top_k=[50, 0, 0], top_p=[0.95, 1.0, 0.9])
    assert torch.equal(mixed[0], both[0])
    assert torch.equal(mixed[1], cpu_case[2][1])
    with pytest.raises(ValueError):
        model.generate_ragged(prompts, temperature=[0.8, 0.0])


def test_eos_ends_one_sequence_only_cpu(cpu_case):
    model, prompts, _ = cpu_case
    full = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11,
                                 **SAMPLE)
    eos = int(full[1][LENS[1] + 2])          # sequence 1's third new token
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11,
                                eos_token_id=eos, **SAMPLE)
    for b, (g, w) in enumerate(zip(got, full)):
        new = w[LENS[b]:].tolist()
        end = new.index(eos) + 1 if eos in new else N_NEW
        assert torch.equal(g, w[:LENS[b] + end]), (b, g, w)
    assert int(got[1][-1]) == eos and len(got[1]) <= LENS[1] + 3


# ---------------------------------------------------------------- GPU ----
@pytest.fixture(scope="module")
def gpu_case():
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).bfloat16().to(torch.device("cuda", 0)).eval()
    return model, make_prompts(cfg.vocab_size, 1)


@pytest.mark.gpu
def test_graph_replay_equals_eager_sampled_gpu(gpu_case):
    model, prompts = gpu_case
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11,
                                  use_graph=True, **SAMPLE)
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=11,
                                  use_graph=False, **SAMPLE)
    other = model.generate_ragged(prompts, max_new_tokens=N_NEW, seed=12,
                                  use_graph=True, **SAMPLE)
    greedy = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    for b, (g, e) in enumerate(zip(graph, eager)):
        assert g.numel() == LENS[b] + N_NEW
        assert torch.equal(g, e), (b, g, e)
    assert not same(graph, other)
    assert not same(graph, greedy)


@pytest.mark.gpu
def test_mixed_batch_keeps_greedy_rows_gpu(gpu_case):
    model, prompts = gpu_case
    greedy = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    mixed = model.generate_ragged(
        prompts, max_new_tokens=N_NEW, seed=11,
        temperature=[0.8, 0.0, 1.2, 0.0], top_k=[50, 0, 0, 0],
        top_p=[0.95, 1.0, 0.9, 1.0])
    assert torch.equal(mixed[1], greedy[1])
    assert torch.equal(mixed[3], greedy[3])
    assert not torch.equal(mixed[0], greedy[0])

"""Ragged-batch generation: prompts of different lengths in one batch give
what each prompt gives alone, a sequence ends at its first eos, and on the
GPU the captured step, the pad token and other sequences' eos change
nothing."""
import pytest
import torch

from torch_on_k8s_amd.models.llama import LlamaModel, get_config

LENS = [5, 12, 9, 1]
N_NEW = 8

# Model seed of the GPU-vs-fp32 test (prompts: seed + 1000), chosen from the
# fp32 CPU reference alone. Of 0..199, ten seeds (2, 48, 52, 56, 108, 128,
# 153, 158, 163, 181) have a top-2 margin >= 4 * 2^-7 * max|logit| at the
# first two new tokens of all four sequences; 158 has the widest (1.87x).
GPU_REF_SEED = 158


def naive_greedy(model, ids, n):
    out = ids
    for _ in range(n):
        logits = model(out)  # full forward, no cache
        out = torch.cat([out, logits[:, -1].argmax(-1, keepdim=True)], dim=1)
    return out


def make_prompts(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in LENS]


@pytest.fixture(scope="module")
def cpu_case():
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).eval()
    prompts = make_prompts(cfg.vocab_size, 1)
    with torch.no_grad():
        want = [naive_greedy(model, p[None], N_NEW)[0] for p in prompts]
    return model, prompts, want


def test_ragged_matches_each_prompt_alone_cpu(cpu_case):
    model, prompts, want = cpu_case
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    assert len(got) == len(prompts)
    for g, w in zip(got, want):
        assert torch.equal(g, w), (g, w)
    # lists of ids are accepted too
    got2 = model.generate_ragged([p.tolist() for p in prompts],
                                 max_new_tokens=N_NEW)
    assert all(torch.equal(a, b) for a, b in zip(got, got2))


def test_ragged_eos_cpu(cpu_case):
    model, prompts, want = cpu_case
    n1 = LENS[1]
    eos = int(want[1][n1 + 2])           # sequence 1's third new token
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                eos_token_id=eos)
    for b, (g, w) in enumerate(zip(got, want)):
        new = w[LENS[b]:].tolist()
        end = new.index(eos) + 1 if eos in new else N_NEW
        assert torch.equal(g, w[:LENS[b] + end]), (b, g, w)
    first = want[1][n1:].tolist().index(eos)
    assert len(got[1]) == n1 + first + 1 <= n1 + 3
    assert int(got[1][-1]) == eos


def test_ragged_rejects_empty_prompt():
    cfg = get_config("llama-tiny")
    model = LlamaModel(cfg).eval()
    with pytest.raises(ValueError):
        model.generate_ragged([[1, 2], []], max_new_tokens=2)


def test_gpt2_ragged_not_implemented():
    from torch_on_k8s_amd.models.registry import (build_model,
                                                  get_model_config)
    model = build_model(get_model_config("gpt2-tiny"))
    with pytest.raises(NotImplementedError, match="ragged"):
        model.generate_ragged([[1, 2], [3]])


# ---------------------------------------------------------------- GPU ----
@pytest.fixture(scope="module")
def gpu_case():
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    dev = torch.device("cuda", 0)
    model = LlamaModel(cfg).bfloat16().to(dev).eval()
    prompts = make_prompts(cfg.vocab_size, 1)
    graph = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  use_graph=True)
    return model, prompts, graph


@pytest.mark.gpu
def test_graph_replay_equals_eager_gpu(gpu_case):
    model, prompts, graph = gpu_case
    eager = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  use_graph=False)
    for b, (g, e) in enumerate(zip(graph, eager)):
        assert g.numel() == LENS[b] + N_NEW
        assert torch.equal(g, e), (b, g, e)


@pytest.mark.gpu
def test_pad_token_does_not_matter_gpu(gpu_case):
    model, prompts, graph = gpu_case
    other = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                  use_graph=True, pad_token_id=7)
    for g, o in zip(graph, other):
        assert torch.equal(g, o), (g, o)


@pytest.mark.gpu
def test_eos_leaves_other_sequences_alone_gpu(gpu_case):
    model, prompts, graph = gpu_case
    eos = int(graph[1][LENS[1] + 2])
    got = model.generate_ragged(prompts, max_new_tokens=N_NEW,
                                eos_token_id=eos, use_graph=True)
    for b, (g, w) in enumerate(zip(got, graph)):
        new = w[LENS[b]:].tolist()
        end = new.index(eos) + 1 if eos in new else N_NEW
        assert torch.equal(g, w[:LENS[b] + end]), (b, g, w)
    assert int(got[1][-1]) == eos and len(got[1]) <= LENS[1] + 3


@pytest.mark.gpu
def test_ragged_gpu_vs_fp32_reference():
    """bf16 GPU ragged generation against the fp32 CPU reference of the
    same bf16-rounded weights, each prompt alone. Argmax chains part at
    near-ties, so a sequence is compared up to the first step whose
    reference top-2 margin is below 4e, e being the largest difference
    between the existing bf16 GPU forward and the fp32 CPU forward over the
    reference sequences' logits (2e keeps an ordering; the other factor 2
    because the decode path rounds differently from the prefill path e is
    taken on). Asserted: the first two new tokens of every sequence are
    among the compared ones."""
    torch.manual_seed(GPU_REF_SEED)
    cfg = get_config("llama-tiny")
    dev = torch.device("cuda", 0)
    model = LlamaModel(cfg).bfloat16().eval()
    ref_model = LlamaModel(cfg).eval()
    ref_model.load_state_dict(
        {k: v.float() for k, v in model.state_dict().items()})
    model = model.to(dev)
    prompts = make_prompts(cfg.vocab_size, GPU_REF_SEED + 1000)

    refs, margins, e = [], [], 0.0
    with torch.no_grad():
        for p in prompts:
            out, mar = p[None], []
            for _ in range(N_NEW):
                lg = ref_model(out)[0, -1]
                top = lg.topk(2).values
                mar.append(float(top[0] - top[1]))
                out = torch.cat([out, lg.argmax().view(1, 1)], dim=1)
            refs.append(out[0])
            margins.append(mar)
            lg_cpu = ref_model(out)
            lg_gpu = model(out.to(dev)).float().cpu()
            e = max(e, float((lg_gpu - lg_cpu).abs().max()))

    got = model.generate_ragged(prompts, max_new_tokens=N_NEW)
    print(f"RAGGED_GEN e={e:.5f} 4e={4 * e:.5f}")
    for b, (g, w) in enumerate(zip(got, refs)):
        n = 0
        while n < N_NEW and margins[b][n] >= 4 * e:
            n += 1
        print(f"RAGGED_GEN seq{b}: compared={n} "
              f"margins={[round(m, 4) for m in margins[b]]}")
        assert n >= 2, (b, margins[b], e)
        assert torch.equal(g.cpu()[:LENS[b] + n], w[:LENS[b] + n]), (b, g, w)


@pytest.mark.gpu
def test_ragged_agrees_with_generate_on_equal_lengths_gpu():
    # the inputs of test_generate.test_generate_matches_naive_gpu
    torch.manual_seed(0)
    cfg = get_config("llama-tiny")
    dev = torch.device("cuda", 0)
    model = LlamaModel(cfg).bfloat16().to(dev).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 12), device=dev)
    want = model.generate(ids, max_new_tokens=8)
    got = model.generate_ragged([ids[0], ids[1]], max_new_tokens=8)
    for b in range(2):
        assert torch.equal(got[b][:12 + 4], want[b, :12 + 4]), (got, want)

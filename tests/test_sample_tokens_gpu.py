"""ops.sample_tokens on the GPU against the fp64 reference of
sampler_oracle.py: the grid of vocabularies, batch sizes and per-row
parameter mixes, the planted cases, the generator's draws, determinism and
a captured call that follows new contents."""
import pytest
import torch

import sampler_oracle as so
from torch_on_k8s_amd import ops

pytestmark = pytest.mark.gpu

ROW = ("temperature", "top_k", "top_p", "seed", "counter")


def run_gpu(c, logits=None):
    dev = torch.device("cuda", 0)
    lg = c["logits"].to(dev) if logits is None else logits
    u = c.get("u")
    return ops.sample_tokens(lg, *(c[n].to(dev) for n in ROW),
                             u=None if u is None else u.to(dev)).cpu()


@pytest.mark.parametrize("V", so.VOCABS)
def test_grid_against_the_oracle(V):
    cases = so.grid_cases(V)
    assert sorted({c["logits"].shape[0] for c in cases}) == [1, 3, 8]
    for i, c in enumerate(cases):
        tok = run_gpu(c)
        assert tok.dtype == torch.long and tok.shape == (c["logits"].shape[0],)
        so.check(f"gpu.V{V}.case{i}", tok, c["specs"])
        greedy = c["temperature"] <= 0
        want = c["logits"].float().argmax(-1)
        assert torch.equal(tok[greedy], want[greedy])
        # the same call again, and the rows in another order
        assert torch.equal(run_gpu(c), tok)
        B = tok.numel()
        if B > 1:
            perm = torch.roll(torch.arange(B), 1)
            pc = {n: c[n][perm] for n in ROW + ("logits",)}
            assert torch.equal(run_gpu(pc), tok[perm])


@pytest.mark.parametrize("name", ["tie_at_k", "neg_inf", "neg_inf_tail", "tiny_T",
                                  "explicit_u"])
def test_planted_cases(name):
    c = so.planted_cases()[name]
    so.check(f"gpu.{name}", run_gpu(c), c["specs"])


def test_bad_inputs_stay_in_range():
    """NaN and +inf logits: the token is unspecified, but it is an index
    of the row and the call returns."""
    c = so.bad_input_case()
    tok = run_gpu(c)
    assert bool(((tok >= 0) & (tok < c["logits"].shape[1])).all()), tok
    assert torch.equal(run_gpu(c), tok)


def test_row_stride_and_alignment():
    """Rows cut out of a wider buffer: a row stride that is no multiple of
    8 elements, so the rows start at every 2-byte offset of a 16-byte
    line; and a column offset on top."""
    dev = torch.device("cuda", 0)
    for V in (1001, 32000):
        c = [x for x in so.grid_cases(V) if x["logits"].shape[0] == 8][0]
        want = run_gpu(c)
        wide = torch.full((8, V + 37), float("nan"), dtype=torch.bfloat16,
                          device=dev)
        wide[:, 3:3 + V] = c["logits"].to(dev)
        view = wide[:, 3:3 + V]
        assert view.stride() == (V + 37, 1) and not view.is_contiguous()
        assert torch.equal(run_gpu(c, view), want)
        so.check(f"gpu.stride.V{V}", run_gpu(c, view), c["specs"])


def test_generator_draws_match_philox():
    """V = 2^19 equal logits: every mass is 1, every sum is an integer and
    exact, so the token is floor(u * V): the top 19 of u's 24 bits, read
    straight off the kernel's generator.

    Known limit: the op returns a token, never u, and V is capped at
    2^20 - 8, so no row can expose the low 5 bits of u (of the generator's
    word, bits 8..12). All 32 bits of the Philox word are checked against
    the known answers on the host implementations only; a wrong shift or
    scale in the kernel would still move the 19 bits compared here."""
    dev = torch.device("cuda", 0)
    V, B = 1 << 19, 256
    logits = torch.zeros(1, V, dtype=torch.bfloat16, device=dev).expand(B, V)
    ones = torch.ones(B, dtype=torch.float32, device=dev)
    zk = torch.zeros(B, dtype=torch.int32, device=dev)
    big = (1 << 40) + 12345
    runs = [
        ([7] * B, list(range(B)), torch.int32),
        ([big] * B, [big + i for i in range(B)], torch.long),
        ([i * 7919 - 3 for i in range(B)], [5] * B, torch.int32),
        ([big * 3 + i for i in range(B)], [big] * B, torch.long),
        ([-1 - i for i in range(B)], list(range(B)), torch.long),
    ]
    for seeds, ctrs, cdt in runs:
        tok = ops.sample_tokens(
            logits, ones, zk, ones,
            torch.tensor(seeds, dtype=torch.long, device=dev),
            torch.tensor(ctrs, dtype=cdt, device=dev)).cpu().tolist()
        want = [int(so.uniform(s, c) * V) for s, c in zip(seeds, ctrs)]
        assert tok == want
        assert len(set(tok)) > B // 2


def test_fp32_logits_raise_type_error():
    dev = torch.device("cuda", 0)
    c = so.grid_cases(512)[0]
    with pytest.raises(TypeError, match="sample_tokens"):
        run_gpu(c, c["logits"].float().to(dev))


def test_captured_call_follows_new_contents():
    dev = torch.device("cuda", 0)
    a, b = [x for x in so.grid_cases(32000) if x["logits"].shape[0] == 8][:2]
    st = {n: a[n].to(dev).clone() for n in ROW + ("logits",)}

    def call():
        return ops.sample_tokens(st["logits"], *(st[n] for n in ROW))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    assert torch.equal(out.cpu(), run_gpu(a))
    for n in ROW + ("logits",):                   # in place, same storage
        st[n].copy_(b[n])
    graph.replay()
    got = out.cpu()
    assert torch.equal(got, run_gpu(b))
    so.check("gpu.replay", got, b["specs"])
    assert not torch.equal(got, run_gpu(a))

"""Llama-family transformer, MI355X-first.

This is the flagship model of the data plane (SURVEY.md §7 step 2 /
BASELINE.json: gang-scheduled Llama-3-8B tokens/sec is the headline
metric). Design choices for MI355X:

  * bf16 weights/activations end-to-end; fp32 accumulation inside the
    fused HIP ops (RMSNorm, RoPE, flash attention, AdamW).
  * Projections go through ops.linear: forward and dgrad are
    hipBLASLt/rocBLAS calls, the weight gradient is the gfx950 kernel of
    ops/csrc/wgrad_gemm.hip, accumulated straight into the flat grads;
    everything fusable is a handwritten gfx950 kernel in ops/.
  * RoPE cos/sin tables precomputed on host (fp32) -- no device trig.
  * 288 GB HBM3E per GPU: default training config holds the whole model,
    grads and fp32 Adam state resident without sharding; activation
    checkpointing is optional and off by default.
"""
from __future__ import annotations

import secrets
from dataclasses import dataclass, asdict

import torch
import torch.nn as nn
import torch.nn.functional as F

from torch_on_k8s_amd import ops


@dataclass
class LlamaConfig:
    name: str = "llama3-8b"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    max_seq_len: int = 8192
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    tie_embeddings: bool = False
    # "hip": fused gfx950 flash-attention kernel (CPU: fp32 reference);
    # "sdpa": torch scaled_dot_product_attention (used for A/B comparison).
    attn_impl: str = "hip"
    init_std: float = 0.02

    def to_dict(self):
        return asdict(self)


PRESETS = {
    # The headline config named by BASELINE.json.
    "llama3-8b": LlamaConfig(),
    # Single-layer-scale configs for tests / smoke.
    "llama-tiny": LlamaConfig(
        name="llama-tiny", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=64, max_seq_len=256, rope_theta=10000.0),
    # Mid-size config for single-GPU kernel iteration.
    "llama-1b": LlamaConfig(
        name="llama-1b", vocab_size=32000, hidden_size=2048,
        intermediate_size=5504, num_layers=16, num_heads=16, num_kv_heads=8,
        head_dim=128, max_seq_len=4096, rope_theta=500000.0),
}


def get_config(name: str, **overrides) -> LlamaConfig:
    cfg = PRESETS[name]
    if overrides:
        d = cfg.to_dict()
        d.update(overrides)
        cfg = LlamaConfig(**d)
    return cfg


class RMSNorm(nn.Module):
    def __init__(self, hidden: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.eps = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.eps)


def build_rope_table(cfg: LlamaConfig, seq_len: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """Host-precomputed fp32 [S, D/2] cos/sin tables."""
    half = cfg.head_dim // 2
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    t = torch.arange(seq_len, dtype=torch.float64)
    ang = torch.outer(t, inv_freq)
    return (ang.cos().float().contiguous().to(device),
            ang.sin().float().contiguous().to(device))


class Attention(nn.Module):
    """q/k/v projections PACKED into one GEMM (fewer, larger hipBLASLt
    calls — ROADMAP §1a); the packed output is split + roped by the
    single-pass qkv_rope kernel. Head order in qkv_proj's output:
    [q heads | k heads | v heads]."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        H, D = cfg.num_heads, cfg.head_dim
        Hkv = cfg.num_kv_heads
        self.qkv_proj = nn.Linear(cfg.hidden_size, (H + 2 * Hkv) * D,
                                  bias=False)
        self.o_proj = nn.Linear(H * D, cfg.hidden_size, bias=False)

    def project_qkv(self, x, cos, sin, doc_start=None):
        """Packed projection -> roped contiguous q, k, v."""
        cfg = self.cfg
        qkv = ops.linear(x, self.qkv_proj.weight)
        return ops.qkv_rope(qkv, cos, sin, cfg.num_heads, cfg.num_kv_heads,
                            cfg.head_dim, doc_start=doc_start)

    def forward(self, x, cos, sin, doc_start=None, doc_end=None):
        """doc_start / doc_end: packed-document bounds (ops.doc_bounds);
        both RoPE positions and the attention mask restart per document."""
        B, S, _ = x.shape
        cfg = self.cfg
        if doc_start is not None and cfg.attn_impl == "sdpa":
            raise NotImplementedError(
                "document bounds need attn_impl='hip'; the sdpa path has no "
                "document mask")
        q, k, v = self.project_qkv(x, cos, sin, doc_start)
        if cfg.attn_impl == "sdpa" and x.is_cuda:
            rep = cfg.num_heads // cfg.num_kv_heads
            qt = q.transpose(1, 2)
            kt = k.transpose(1, 2).repeat_interleave(rep, dim=1)
            vt = v.transpose(1, 2).repeat_interleave(rep, dim=1)
            o = F.scaled_dot_product_attention(qt, kt, vt, is_causal=True)
            o = o.transpose(1, 2).contiguous()
        else:
            o = ops.attention(q, k, v, causal=True, doc_start=doc_start,
                              doc_end=doc_end)
        return ops.linear(o.reshape(B, S, cfg.num_heads * cfg.head_dim),
                          self.o_proj.weight)


class MLP(nn.Module):
    """gate/up packed into one GEMM; fused SwiGLU kernel reads the
    packed output directly (one pass fwd, one pass bwd, no silu
    intermediate in HBM)."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.gate_up_proj = nn.Linear(cfg.hidden_size,
                                      2 * cfg.intermediate_size, bias=False)
        self.down_proj = nn.Linear(cfg.intermediate_size, cfg.hidden_size, bias=False)

    def forward(self, x):
        gu = ops.linear(x, self.gate_up_proj.weight)
        return ops.linear(ops.swiglu(gu), self.down_proj.weight)


class Block(nn.Module):
    """Residual stream threaded as (branch, residual) pairs so every
    residual-add fuses into the NEXT RMSNorm's read (ops.rmsnorm_residual:
    one kernel does add + norm fwd, and norm-dx + residual-grad add bwd).
    forward(x, res) returns (mlp_out, x_after_attn_add): the caller (next
    block or final norm) performs the pending add inside its fused norm."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.input_norm = RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.attn = Attention(cfg)
        self.post_attn_norm = RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.mlp = MLP(cfg)

    def forward(self, x, res, cos, sin, doc_start=None, doc_end=None):
        h, xr = ops.rmsnorm_residual(x, res, self.input_norm.weight,
                                     self.input_norm.eps)
        a = self.attn(h, cos, sin, doc_start, doc_end)
        h2, xr2 = ops.rmsnorm_residual(a, xr, self.post_attn_norm.weight,
                                       self.post_attn_norm.eps)
        return self.mlp(h2), xr2


class LlamaModel(nn.Module):
    """Decoder-only Llama. forward() returns mean next-token CE loss."""

    def __init__(self, cfg: LlamaConfig, activation_checkpointing: bool = False):
        super().__init__()
        self.cfg = cfg
        self.activation_checkpointing = activation_checkpointing
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList(Block(cfg) for _ in range(cfg.num_layers))
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        if cfg.tie_embeddings:
            self.lm_head.weight = self.embed_tokens.weight
        self._rope_cache: tuple[int, torch.Tensor, torch.Tensor] | None = None
        self.reset_parameters()

    def reset_parameters(self):
        std = self.cfg.init_std
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0.0, std=std)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, mean=0.0, std=std)
            elif isinstance(m, RMSNorm):
                nn.init.ones_(m.weight)
        # scale down output projections per residual-branch count
        scale = (2 * self.cfg.num_layers) ** -0.5
        for blk in self.layers:
            with torch.no_grad():
                blk.attn.o_proj.weight.mul_(scale)
                blk.mlp.down_proj.weight.mul_(scale)

    def _rope(self, S: int, device):
        if self._rope_cache is None or self._rope_cache[0] != S or \
                self._rope_cache[1].device != device:
            cos, sin = build_rope_table(self.cfg, S, device)
            self._rope_cache = (S, cos, sin)
        return self._rope_cache[1], self._rope_cache[2]

    def forward_hidden(self, input_ids: torch.Tensor,
                       doc_start: torch.Tensor | None = None,
                       doc_end: torch.Tensor | None = None) -> torch.Tensor:
        B, S = input_ids.shape
        if doc_start is None and doc_end is not None:
            raise ValueError("doc_end needs doc_start")
        if doc_start is not None and self.cfg.attn_impl == "sdpa":
            raise NotImplementedError(
                "document bounds need attn_impl='hip'; the sdpa path has no "
                "document mask")
        if doc_start is not None and doc_end is None:
            # once per forward, not once per layer
            doc_end = ops.doc_end_from_start(doc_start)
        cos, sin = self._rope(S, input_ids.device)
        x = self.embed_tokens(input_ids)
        res = None  # pending residual, consumed by each fused norm
        for blk in self.layers:
            if self.activation_checkpointing and self.training:
                x, res = torch.utils.checkpoint.checkpoint(
                    blk, x, res, cos, sin, doc_start, doc_end,
                    use_reentrant=False)
            else:
                x, res = blk(x, res, cos, sin, doc_start, doc_end)
        y, _ = ops.rmsnorm_residual(x, res, self.norm.weight, self.norm.eps)
        return y

    def forward(self, input_ids: torch.Tensor,
                labels: torch.Tensor | None = None,
                doc_start: torch.Tensor | None = None,
                doc_end: torch.Tensor | None = None,
                ignore_index: int | None = None, z_loss: float = 0.0):
        """doc_start / doc_end: packed-document bounds of input_ids
        (ops.doc_bounds). ignore_index / z_loss: as ops.cross_entropy;
        tokens whose label is ignore_index are left out of the loss, whose
        mean is over the rest."""
        x = self.forward_hidden(input_ids, doc_start, doc_end)
        logits = ops.linear(x, self.lm_head.weight)
        if labels is None:
            return logits
        return ops.cross_entropy(logits, labels, ignore_index=ignore_index,
                                 z_loss=z_loss)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 32,
                 temperature: float = 0.0,
                 use_graph: bool | None = None) -> torch.Tensor:
        """Greedy (temperature=0) or sampled autoregressive generation —
        the serving path. Prefill runs through the flash-attention
        kernel; each decode step uses the KV-cache single-token decode
        kernel (ops.attention_decode)."""
        cfg = self.cfg
        B, S0 = input_ids.shape
        dev = input_ids.device
        dtype = self.embed_tokens.weight.dtype
        Tmax = S0 + max_new_tokens
        Hkv, Hq, D = cfg.num_kv_heads, cfg.num_heads, cfg.head_dim
        kc = [torch.zeros(B, Tmax, Hkv, D, dtype=dtype, device=dev)
              for _ in self.layers]
        vc = [torch.zeros(B, Tmax, Hkv, D, dtype=dtype, device=dev)
              for _ in self.layers]
        cos, sin = build_rope_table(cfg, Tmax, dev)

        def run_block(blk, i, x, pos0, T):
            """One block over x ([B,s,H]); writes this slice's K/V into
            the caches and attends over cache[:T]."""
            B_, s, _ = x.shape
            h = blk.input_norm(x)
            q, k, v = blk.attn.project_qkv(
                h, cos[pos0:pos0 + s].contiguous(),
                sin[pos0:pos0 + s].contiguous())
            kc[i][:, pos0:pos0 + s] = k
            vc[i][:, pos0:pos0 + s] = v
            if s > 1:  # prefill
                o = ops.attention(q, k, v, causal=True)
            else:      # single-token decode over the cache
                o = ops.attention_decode(q[:, 0], kc[i], vc[i], T)
                o = o.view(B_, 1, Hq, D)
            x = x + blk.attn.o_proj(o.reshape(B_, s, Hq * D))
            x = x + blk.mlp(blk.post_attn_norm(x))
            return x

        def next_token(logits):
            if temperature and temperature > 0:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                return torch.multinomial(probs, 1)
            return logits.argmax(-1, keepdim=True)

        # prefill
        x = self.embed_tokens(input_ids)
        for i, blk in enumerate(self.layers):
            x = run_block(blk, i, x, 0, S0)
        logits = self.lm_head(self.norm(x[:, -1:]))[:, -1]
        tokens = [next_token(logits)]

        # Greedy GPU decode is launch-bound (hundreds of tiny kernels per
        # token); capture one whole decode step in a hipGraph and replay
        # it per token. Position/length live on-device (index_copy_/
        # index_select + the decode kernel's T_dev) so replay stays
        # correct; the graph is self-feeding (argmax writes the token
        # buffer the next replay embeds).
        if use_graph is None:
            use_graph = (dev.type == "cuda" and not temperature and
                         max_new_tokens >= 8)

        if not use_graph:
            for step in range(1, max_new_tokens):
                pos = S0 + step - 1
                x = self.embed_tokens(tokens[-1])
                for i, blk in enumerate(self.layers):
                    x = run_block(blk, i, x, pos, pos + 1)
                logits = self.lm_head(self.norm(x))[:, -1]
                tokens.append(next_token(logits))
            return torch.cat([input_ids] + tokens, dim=1)

        token_buf = tokens[0].clone()                       # [B, 1]
        pos_long = torch.tensor([S0], dtype=torch.long, device=dev)
        t32 = torch.zeros((), dtype=torch.int32, device=dev)

        def decode_step():
            t32.copy_((pos_long[0] + 1).to(torch.int32))
            x = self.embed_tokens(token_buf)
            cs = torch.index_select(cos, 0, pos_long).contiguous()
            sn = torch.index_select(sin, 0, pos_long).contiguous()
            for i, blk in enumerate(self.layers):
                h = blk.input_norm(x)
                q, k, v = blk.attn.project_qkv(h, cs, sn)
                kc[i].index_copy_(1, pos_long, k)
                vc[i].index_copy_(1, pos_long, v)
                o = ops.attention_decode(q[:, 0], kc[i], vc[i], 0, T_dev=t32)
                x = x + blk.attn.o_proj(o.view(B, 1, Hq * D))
                x = x + blk.mlp(blk.post_attn_norm(x))
            logits = self.lm_head(self.norm(x))[:, -1]
            nxt = logits.argmax(-1, keepdim=True)
            token_buf.copy_(nxt)       # self-feed the next replay
            pos_long.add_(1)

        graph = None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        n_warm = min(2, max_new_tokens - 1)
        with torch.cuda.stream(side):
            for _ in range(n_warm):    # real decode steps (allocator/rng warm)
                decode_step()
                tokens.append(token_buf.clone())
        torch.cuda.current_stream().wait_stream(side)
        if max_new_tokens - 1 > n_warm:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                decode_step()          # capture only; not executed
            for _ in range(max_new_tokens - 1 - n_warm):
                graph.replay()
                tokens.append(token_buf.clone())
        return torch.cat([input_ids] + tokens, dim=1)

    @torch.no_grad()
    def generate_ragged(self, prompts, max_new_tokens: int = 32,
                        eos_token_id: int | None = None,
                        use_graph: bool | None = None,
                        pad_token_id: int = 0, *,
                        temperature=0.0, top_k=0, top_p=1.0,
                        seed=None,
                        prefill_chunk: int | None = None,
                        kv_dtype: str | None = None,
                        weight_dtype: str | None = None,
                        kv_page_size: int | None = None
                        ) -> list[torch.Tensor]:
        """Generation for prompts of different lengths (each a 1-D id
        tensor or a list of ids, length >= 1). Returns one 1-D tensor per
        sequence: the prompt followed by its new tokens, ending at the
        first eos_token_id (inclusive) if one is given and emitted.

        temperature / top_k / top_p / seed are scalars or one value per
        prompt. With every temperature 0 (the default) the tokens are the
        argmax. Otherwise every token is drawn by ops.sample_tokens, also
        inside the captured step; a row with temperature 0 stays greedy.
        An int seed s gives row b the seed s + b; seed=None draws one from
        `secrets`. The draw for the token at index i of a sequence depends
        on (that row's seed, i) alone: not on the batch slot, the step
        number or whether the step ran eagerly or as a graph replay.

        Prefill right-pads to the longest prompt and runs the causal
        flash-attention kernel: a valid row never sees a pad key, and the
        pad rows' K/V land in cache rows >= len_b, which decode never
        reads before it overwrites them. Decode keeps per-sequence
        lengths on the device (ops.qkv_rope_append_ +
        ops.attention_decode_ragged), so one captured step serves every
        sequence whatever its length.

        prefill_chunk=N (>= 1) prefills through the cache instead, in
        ceil(S0 / N) chunks of N tokens per sequence: each chunk is appended
        by ops.qkv_rope_append_chunk_ and attends to the cache by
        ops.attention_extend, with per-sequence positions and lengths on
        the device, so no pad key is ever written or read and the
        activations are [B, N] wide. None (the default) is the padded
        prefill above.

        kv_dtype="fp8" keeps the KV cache as OCP e4m3 codes with one fp32
        scale per (token, kv head) row: (D + 4) / (2 D) of the bf16 cache.
        The padded prefill attends to its bf16 q/k/v as before and stores
        them through ops.kv_quantize_append_ (pad rows are not written); the
        decode step is ops.qkv_rope_append_fp8_ + the fp8
        ops.attention_decode_ragged, also inside the captured step. None
        (the default) is the bf16 cache. Not available with prefill_chunk.

        weight_dtype="fp8" runs the five projections (qkv_proj, o_proj,
        gate_up_proj, down_proj, lm_head) of the prefill and of the decode
        step, eager and captured, through ops.linear_w8 on e4m3 weight codes
        with one fp32 scale per output channel: a decode step reads half the
        weight bytes. The codes are built on first use by
        ops.quantize_weight_fp8 and kept on the model outside state_dict,
        per weight and keyed by (data_ptr, _version), so a changed weight is
        requantized; drop_quantized_weights() frees them. The bf16 weights
        stay resident, and the embedding lookup stays bf16 also with
        tie_embeddings. None (the default) is the bf16 path. Combines with
        kv_dtype, prefill_chunk and the sampling arguments.

        weight_dtype="mxfp4" is the same with OCP MXFP4 weights (e2m1 codes,
        one e8m0 scale per 32 elements, 4.25 bits per weight) from
        ops.quantize_weight_mxfp4 through ops.linear_w4: a decode step reads
        a good quarter of the bf16 weight bytes. The hidden sizes must be
        multiples of 32. It combines with everything "fp8" combines with; the
        two modes share the cache of quantized copies.

        kv_page_size=64 keeps the KV cache in pages of 64 tokens instead of
        a [B, S0max + max_new_tokens] rectangle: per layer a pool
        [P, Hkv, 64, D] of exactly ops.kv_pages_needed(lens, max_new_tokens)
        pages, and one int32 page table [B, NP] on the device shared by all
        layers (unused entries -1; a sequence's pages are dealt round-robin
        over the sequences). The padded prefill stores its k / v into the
        pool; prefill_chunk and the decode step, eager and captured, go
        through ops.qkv_rope_append_paged_ + ops.attention_paged. None (the
        default) is the rectangle. Combines with prefill_chunk, weight_dtype
        and the sampling arguments; not with kv_dtype="fp8".

        kv_dtype="fp8_paged" is both at once: per layer e4m3 code pools
        [P, Hkv, 64, D] and fp32 scale pools [P, Hkv, 64] of exactly
        ops.kv_pages_needed pages under the page table of the bf16 paged
        mode, each row quantized as kv_dtype="fp8" quantizes it. The padded
        prefill stores through ops.kv_quantize_append_paged_; prefill_chunk
        and the decode step, eager and captured, go through
        ops.qkv_rope_append_paged_fp8_ + the fp8 ops.attention_paged.
        Combines with prefill_chunk, weight_dtype and the sampling
        arguments; kv_page_size may be None or 64 with it."""
        if kv_page_size is not None and kv_page_size != ops.KV_PAGE:
            raise ValueError(f"kv_page_size must be None or {ops.KV_PAGE}, "
                             f"got {kv_page_size!r}")
        if kv_dtype not in (None, "fp8", "fp8_paged"):
            raise ValueError(f"kv_dtype must be None, 'fp8' or 'fp8_paged', "
                             f"got {kv_dtype!r}")
        fp8p = kv_dtype == "fp8_paged"
        paged = kv_page_size is not None and not fp8p   # the bf16 pool
        if paged and kv_dtype is not None:
            raise ValueError("kv_page_size does not combine with kv_dtype: "
                             "the paged pool is bf16 (the e4m3 pool is "
                             "kv_dtype='fp8_paged')")
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("prefill_chunk must be >= 1 or None")
        if weight_dtype not in (None, "fp8", "mxfp4"):
            raise ValueError(f"weight_dtype must be None, 'fp8' or 'mxfp4', "
                             f"got {weight_dtype!r}")
        wq = weight_dtype is not None        # quantized projections
        qlinear = ops.linear_w4 if weight_dtype == "mxfp4" else ops.linear_w8
        fp8 = kv_dtype == "fp8"
        if fp8 and prefill_chunk is not None:
            raise ValueError("kv_dtype='fp8' has no chunked prefill: "
                             "attention_extend reads a bf16 cache "
                             "(kv_dtype='fp8_paged' has one)")
        cfg = self.cfg
        dev = self.embed_tokens.weight.device
        dtype = self.embed_tokens.weight.dtype
        B = len(prompts)

        def per_row(name, value):
            if isinstance(value, (list, tuple)):
                if len(value) != B:
                    raise ValueError(f"{name}: {len(value)} values for {B} "
                                     f"prompts")
                return list(value)
            return [value] * B

        temps = [float(t) for t in per_row("temperature", temperature)]
        sampled = any(t > 0 for t in temps)
        if sampled:
            # host RNG before any GPU work; int64 two's complement
            if seed is None:
                seed = secrets.randbits(63)
            seeds = (list(seed) if isinstance(seed, (list, tuple))
                     else [int(seed) + b for b in range(B)])
            if len(seeds) != B:
                raise ValueError(f"seed: {len(seeds)} values for {B} prompts")
            seeds = [(int(s) + 2 ** 63) % 2 ** 64 - 2 ** 63 for s in seeds]

        seqs = [torch.as_tensor(p, dtype=torch.long).reshape(-1).to(dev)
                for p in prompts]
        if not seqs or any(s.numel() < 1 for s in seqs):
            raise ValueError("generate_ragged needs >= 1 prompt, each of "
                             "length >= 1")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if sampled:
            temp_t = torch.tensor(temps, dtype=torch.float32, device=dev)
            topk_t = torch.tensor([int(k) for k in per_row("top_k", top_k)],
                                  dtype=torch.int32, device=dev)
            topp_t = torch.tensor([float(p) for p in per_row("top_p", top_p)],
                                  dtype=torch.float32, device=dev)
            seed_t = torch.tensor(seeds, dtype=torch.long, device=dev)

        def lin(mod, x):
            """A projection: the module's own call, or ops.linear_w8 /
            ops.linear_w4 over its quantized weight."""
            if not wq:
                return mod(x)
            return qlinear(x, *self._quantized(mod.weight, weight_dtype))

        def mlp(blk, x):
            if not wq:
                return blk.mlp(x)
            return lin(blk.mlp.down_proj,
                       ops.swiglu(lin(blk.mlp.gate_up_proj, x)))

        def pick(logits, index):
            """Next token per row of logits [B, V]; index [B] is where in
            its sequence each token will sit (the draw's counter)."""
            if not sampled:
                return logits.argmax(-1)
            return ops.sample_tokens(logits, temp_t, topk_t, topp_t, seed_t,
                                     index)

        lens0 = torch.tensor([s.numel() for s in seqs], device=dev)
        S0 = int(max(s.numel() for s in seqs))
        Tmax = S0 + max_new_tokens
        Hkv, Hq, D = cfg.num_kv_heads, cfg.num_heads, cfg.head_dim
        input_ids = torch.full((B, S0), pad_token_id, dtype=torch.long,
                               device=dev)
        for b, s in enumerate(seqs):
            input_ids[b, :s.numel()] = s
        cache_dtype = torch.float8_e4m3fn if fp8 or fp8p else dtype
        if paged or fp8p:
            # kc / vc are the pools; pages dealt round-robin over sequences
            PG = ops.KV_PAGE
            need = [-(-(s.numel() + max_new_tokens) // PG) for s in seqs]
            n_pages = ops.kv_pages_needed([s.numel() for s in seqs],
                                          max_new_tokens)
            table = [[-1] * max(need) for _ in range(B)]
            nxt = 0
            for j in range(max(need)):
                for b in range(B):
                    if j < need[b]:
                        table[b][j] = nxt
                        nxt += 1
            page_table = torch.tensor(table, dtype=torch.int32, device=dev)
            assert nxt == n_pages
            self._kv_pool_pages = nxt         # pages dealt by the last call
            Tmax = PG * max(need)             # the table's span (rope rows)
            cache_shape = (n_pages, Hkv, PG, D)
            one32 = torch.ones(B, dtype=torch.int32, device=dev)
        else:
            cache_shape = (B, Tmax, Hkv, D)
        kc = [torch.zeros(cache_shape, dtype=cache_dtype, device=dev)
              for _ in self.layers]
        vc = [torch.zeros(cache_shape, dtype=cache_dtype, device=dev)
              for _ in self.layers]
        if fp8:
            ks = [torch.zeros(B, Tmax, Hkv, device=dev) for _ in self.layers]
            vs = [torch.zeros(B, Tmax, Hkv, device=dev) for _ in self.layers]
            zero32 = torch.zeros(B, dtype=torch.int32, device=dev)
            one32 = torch.ones(B, dtype=torch.int32, device=dev)
        if fp8p:
            ks = [torch.zeros(cache_shape[:3], device=dev)
                  for _ in self.layers]
            vs = [torch.zeros(cache_shape[:3], device=dev)
                  for _ in self.layers]
            zero32 = torch.zeros(B, dtype=torch.int32, device=dev)
        cos, sin = build_rope_table(cfg, Tmax, dev)

        if prefill_chunk is None:
            # prefill over the padded rectangle
            x = self.embed_tokens(input_ids)
            if paged:  # where every prompt row goes: (page, slot)
                bi = torch.cat([torch.full((s.numel(),), b)
                                for b, s in enumerate(seqs)]).to(dev)
                ti = torch.cat([torch.arange(s.numel()) for s in seqs]).to(dev)
                pg_i = page_table[bi, ti // PG].long()
            cs0, sn0 = cos[:S0].contiguous(), sin[:S0].contiguous()
            for i, blk in enumerate(self.layers):
                if wq:
                    q, k, v = ops.qkv_rope(
                        lin(blk.attn.qkv_proj, blk.input_norm(x)), cs0, sn0,
                        Hq, Hkv, D)
                else:
                    q, k, v = blk.attn.project_qkv(blk.input_norm(x), cs0,
                                                   sn0)
                if fp8:
                    ops.kv_quantize_append_(k, v, zero32,
                                            lens0.to(torch.int32), kc[i],
                                            vc[i], ks[i], vs[i])
                elif fp8p:
                    ops.kv_quantize_append_paged_(
                        k, v, zero32, lens0.to(torch.int32), kc[i], vc[i],
                        ks[i], vs[i], page_table)
                elif paged:
                    kc[i][pg_i, :, ti % PG] = k[bi, ti]
                    vc[i][pg_i, :, ti % PG] = v[bi, ti]
                else:
                    kc[i][:, :S0] = k
                    vc[i][:, :S0] = v
                o = ops.attention(q, k, v, causal=True)
                x = x + lin(blk.attn.o_proj, o.reshape(B, S0, Hq * D))
                x = x + mlp(blk, blk.post_attn_norm(x))
            last = x[torch.arange(B, device=dev), lens0 - 1].unsqueeze(1)
        else:
            # prefill through the cache, N tokens per sequence at a time
            N = int(prefill_chunk)
            len32 = lens0.to(torch.int32)
            last = torch.zeros(B, 1, cfg.hidden_size, dtype=dtype, device=dev)
            rows = torch.arange(B, device=dev)
            for c0 in range(0, S0, N):
                ids = input_ids[:, c0:c0 + N]
                if ids.shape[1] < N:  # the last chunk: same shape, dead tail
                    ids = torch.nn.functional.pad(ids, (0, N - ids.shape[1]),
                                                  value=pad_token_id)
                cpos = torch.full((B,), c0, dtype=torch.int32, device=dev)
                cql = (len32 - c0).clamp(0, N)
                clen = len32.clamp(max=c0 + N)
                x = self.embed_tokens(ids)
                for i, blk in enumerate(self.layers):
                    qkv = lin(blk.attn.qkv_proj, blk.input_norm(x))
                    if fp8p:
                        q = ops.qkv_rope_append_paged_fp8_(
                            qkv, cos, sin, cpos, cql, kc[i], vc[i], ks[i],
                            vs[i], page_table, Hq, Hkv, D)
                        o = ops.attention_paged(
                            q, kc[i], vc[i], page_table, clen, cql,
                            kscale=ks[i], vscale=vs[i])
                    elif paged:
                        q = ops.qkv_rope_append_paged_(
                            qkv, cos, sin, cpos, cql, kc[i], vc[i],
                            page_table, Hq, Hkv, D)
                        o = ops.attention_paged(q, kc[i], vc[i], page_table,
                                                clen, cql)
                    else:
                        q = ops.qkv_rope_append_chunk_(
                            qkv, cos, sin, cpos, cql, kc[i], vc[i], Hq, Hkv,
                            D)
                        o = ops.attention_extend(q, kc[i], vc[i], clen, cql)
                    x = x + lin(blk.attn.o_proj, o.reshape(B, N, Hq * D))
                    x = x + mlp(blk, blk.post_attn_norm(x))
                # the chunk that holds a sequence's last prompt token
                at = lens0 - 1 - c0
                here = ((at >= 0) & (at < N)).view(B, 1, 1)
                last = torch.where(here, x[rows, at.clamp(0, N - 1)]
                                   .unsqueeze(1), last)
        first = pick(lin(self.lm_head, self.norm(last))[:, -1],
                     lens0).unsqueeze(1)

        # Decode state, all on the device. token_buf holds the token to
        # feed; it sits at position pos = lens - 1 and attends to lens rows.
        # A finished sequence has pos = -1 (no cache write, zero q), a
        # length that no longer grows and a buffer slot that stays at eos.
        eos = -1 if eos_token_id is None else int(eos_token_id)
        token_buf = first.clone()                           # [B, 1]
        finished = (token_buf[:, 0] == eos)
        lens = (lens0 + (~finished)).to(torch.int32)
        pos = torch.where(finished, -1, lens0).to(torch.int32)
        tokens = [token_buf.clone()]

        def decode_step():
            x = self.embed_tokens(token_buf)
            for i, blk in enumerate(self.layers):
                h = blk.input_norm(x)
                qkv = lin(blk.attn.qkv_proj, h)
                if fp8:
                    q = ops.qkv_rope_append_fp8_(
                        qkv, cos, sin, pos, one32, kc[i], vc[i], ks[i],
                        vs[i], Hq, Hkv, D).view(B, Hq, D)
                    o = ops.attention_decode_ragged(
                        q, kc[i], vc[i], lens, kscale=ks[i], vscale=vs[i])
                elif fp8p:
                    q = ops.qkv_rope_append_paged_fp8_(
                        qkv, cos, sin, pos, one32, kc[i], vc[i], ks[i],
                        vs[i], page_table, Hq, Hkv, D)
                    o = ops.attention_paged(
                        q, kc[i], vc[i], page_table, lens, one32,
                        kscale=ks[i], vscale=vs[i])
                elif paged:
                    q = ops.qkv_rope_append_paged_(
                        qkv, cos, sin, pos, one32, kc[i], vc[i], page_table,
                        Hq, Hkv, D)
                    o = ops.attention_paged(q, kc[i], vc[i], page_table,
                                            lens, one32)
                else:
                    q = ops.qkv_rope_append_(
                        qkv.view(B, (Hq + 2 * Hkv) * D), cos, sin, pos,
                        kc[i], vc[i], Hq, Hkv, D)
                    o = ops.attention_decode_ragged(q, kc[i], vc[i], lens)
                x = x + lin(blk.attn.o_proj, o.view(B, 1, Hq * D))
                x = x + mlp(blk, blk.post_attn_norm(x))
            nxt = pick(lin(self.lm_head, self.norm(x))[:, -1], lens)
            nxt = torch.where(finished, eos, nxt)
            finished.logical_or_(nxt == eos)
            token_buf.copy_(nxt.unsqueeze(1))  # self-feed the next replay
            lens.add_((~finished).to(torch.int32))
            pos.copy_(torch.where(finished, -1, lens - 1))

        if use_graph is None:
            use_graph = dev.type == "cuda" and max_new_tokens >= 8

        if not use_graph:
            for _ in range(max_new_tokens - 1):
                decode_step()
                tokens.append(token_buf.clone())
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            n_warm = min(2, max_new_tokens - 1)
            with torch.cuda.stream(side):
                for _ in range(n_warm):  # real steps (allocator warm-up)
                    decode_step()
                    tokens.append(token_buf.clone())
            torch.cuda.current_stream().wait_stream(side)
            if max_new_tokens - 1 > n_warm:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    decode_step()        # capture only; not executed
                for _ in range(max_new_tokens - 1 - n_warm):
                    graph.replay()
                    tokens.append(token_buf.clone())

        new = torch.cat(tokens, dim=1).tolist()             # one host read
        out = []
        for b, s in enumerate(seqs):
            row = new[b]
            if eos_token_id is not None and eos in row:
                row = row[:row.index(eos) + 1]
            out.append(torch.cat([s, torch.tensor(row, dtype=torch.long,
                                                  device=dev)]))
        return out

    def _quantized(self, weight: torch.Tensor, mode: str = "fp8"):
        """(codes, scales) of a projection weight for weight_dtype=mode,
        built on first use and again after the weight changed. One cache for
        both modes, keyed by (weight, mode)."""
        cache = self.__dict__.setdefault("_w8_cache", {})
        key = (weight.data_ptr(), mode)
        ent = cache.get(key)
        if ent is None or ent[0] != weight._version:
            quantize = (ops.quantize_weight_mxfp4 if mode == "mxfp4"
                        else ops.quantize_weight_fp8)
            ent = (weight._version, *quantize(weight))
            cache[key] = ent
        return ent[1], ent[2]

    def drop_quantized_weights(self) -> None:
        """Free the copies that weight_dtype="fp8" and "mxfp4" built."""
        self.__dict__.pop("_w8_cache", None)

    def num_params(self) -> int:
        seen, total = set(), 0
        for p in self.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                total += p.numel()
        return total

"""GPT-2 decoder (nanoGPT-compatible parameter names) on the orion_amd op layer.

Parameter names follow the public nanoGPT/HF-GPT-2 layout (``transformer.wte``,
``transformer.h.{i}.attn.c_attn`` ...) so ``ckpt.pt`` files written by
``orion_amd.train.ckpt`` load into nanoGPT-style code and vice versa.

MI355X-first choices (not in the reference, which has no model at all --
SURVEY.md §2.11 [north-star]):

* the QKV projection output ``(B, T, 3C)`` is consumed by the flash-attention
  kernel in place (no head transposes); the kernel writes ``(B, T, C)`` for
  ``c_proj``;
* ``c_fc`` bias + GELU-tanh run as one fused HIP kernel after a bias-less GEMM;
* the loss is a fused softmax-cross-entropy that emits dlogits in its forward
  pass, so the ``(B*T, 50304)`` fp32 probabilities are never materialised.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .generation import Generation, dense, session_weights
from .kv_cache import KVCache


@dataclass
class GPTConfig:
    block_size: int = 1024
    vocab_size: int = 50304  # GPT-2's 50257 padded to a multiple of 64
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    dropout: float = 0.0
    bias: bool = True

    def to_dict(self):
        return asdict(self)

    @property
    def head_dim(self):
        return self.n_embd // self.n_head


PRESETS = {
    # BASELINE.json config 1: CPU plumbing model
    "gpt2-tiny": dict(n_layer=2, n_head=2, n_embd=128, block_size=256),  # head dim 64 (HIP attention: 64/128)
    "gpt2": dict(n_layer=12, n_head=12, n_embd=768),            # 124M
    "gpt2-medium": dict(n_layer=24, n_head=16, n_embd=1024),    # 350M
    "gpt2-large": dict(n_layer=36, n_head=20, n_embd=1280),     # 774M
    "gpt2-xl": dict(n_layer=48, n_head=25, n_embd=1600),        # 1558M
}


class LayerNorm(nn.Module):
    def __init__(self, ndim, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(ndim))
        self.bias = nn.Parameter(torch.zeros(ndim)) if bias else None

    def forward(self, x):
        return ops.layer_norm(x, self.weight, self.bias, 1e-5)


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.c_attn = nn.Linear(cfg.n_embd, 3 * cfg.n_embd, bias=cfg.bias)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd, bias=cfg.bias)
        self.n_head = cfg.n_head
        self.dropout = cfg.dropout

    def attend(self, x):
        """QKV projection + attention, before the output projection (B, T, C); the QKV bias
        gradient is summed inside the attention backward on the HIP path."""
        return ops.linear_attention_qkv(x, self.c_attn.weight, self.c_attn.bias, self.n_head)

    def forward(self, x, fuse_out_bias=False):
        y = self.attend(x)
        # with fuse_out_bias the caller adds c_proj.bias inside its add+LayerNorm kernel
        y = ops.linear(y, self.c_proj.weight, None if fuse_out_bias else self.c_proj.bias)
        if self.dropout and self.training:
            y = F.dropout(y, self.dropout)
        return y


class MLP(nn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.c_fc = nn.Linear(cfg.n_embd, 4 * cfg.n_embd, bias=cfg.bias)
        self.c_proj = nn.Linear(4 * cfg.n_embd, cfg.n_embd, bias=cfg.bias)
        self.dropout = cfg.dropout

    def forward(self, x, fuse_out_bias=False):
        y = ops.mlp(x, self.c_fc.weight, self.c_fc.bias, self.c_proj.weight,
                    None if fuse_out_bias else self.c_proj.bias)
        if self.dropout and self.training:
            y = F.dropout(y, self.dropout)
        return y


class Block(nn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.ln_1 = LayerNorm(cfg.n_embd, cfg.bias)
        self.attn = CausalSelfAttention(cfg)
        self.ln_2 = LayerNorm(cfg.n_embd, cfg.bias)
        self.mlp = MLP(cfg)

    def forward(self, x):
        x = x + self.attn(self.ln_1(x))
        x = x + self.mlp(self.ln_2(x))
        return x


class GPT(nn.Module, Generation):
    """GPT-2 language model.  ``forward(idx, targets)`` -> (logits|None, loss|None)."""

    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.config = cfg
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(cfg.vocab_size, cfg.n_embd),
            wpe=nn.Embedding(cfg.block_size, cfg.n_embd),
            h=nn.ModuleList([Block(cfg) for _ in range(cfg.n_layer)]),
            ln_f=LayerNorm(cfg.n_embd, cfg.bias),
        ))
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.transformer.wte.weight = self.lm_head.weight  # weight tying
        self.apply(self._init_weights)
        for pn, p in self.named_parameters():
            if pn.endswith("c_proj.weight"):
                nn.init.normal_(p, mean=0.0, std=0.02 / math.sqrt(2 * cfg.n_layer))

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)

    def num_params(self, non_embedding=True):
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.transformer.wpe.weight.numel()
        return n

    def flops_per_token(self, seq_len=None):
        """Training FLOPs per token (6N + attention), as in the PaLM MFU formula."""
        cfg = self.config
        T = seq_len or cfg.block_size
        N = self.num_params()
        return 6 * N + 12 * cfg.n_layer * cfg.n_embd * T

    def forward(self, idx, targets=None):
        B, T = idx.shape
        assert T <= self.config.block_size, f"sequence {T} > block_size {self.config.block_size}"
        blocks = self.transformer.h
        if self.config.dropout and self.training:
            tok = self.transformer.wte(idx)
            x = ops.add_broadcast(tok, self.transformer.wpe.weight[:T])
            x = F.dropout(x, self.config.dropout)
            h = blocks[0].ln_1(x)
        else:
            # token + position embedding and block 0's ln_1 in one op (ops/embedding.py)
            ln = blocks[0].ln_1
            x, h = ops.embed_layer_norm(idx, self.transformer.wte.weight, self.transformer.wpe.weight,
                                        ln.weight, ln.bias)
        # Residual stream with every "x = x + branch; h = LN(x)" pair fused into one kernel
        # (forward and backward): block i's second add feeds block i+1's ln_1 (ln_f at the end).
        # The branch output-projection biases are folded into the same kernel
        # (forward: added before the residual sum; backward: their gradient is a
        # column sum of the residual-stream gradient the kernel already holds).
        # Without dropout the branch output projections do the residual add themselves (one
        # GEMM with the bias and the old stream in its epilogue; the LayerNorm then reads only
        # the new stream: ops/residual.py).
        fused_sites = not (self.config.dropout and self.training)
        for i, block in enumerate(blocks):
            nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else self.transformer.ln_f
            at, ml = block.attn, block.mlp
            if fused_sites:
                x, h = ops.linear_residual_layer_norm(x, at.attend(h), at.c_proj.weight, at.c_proj.bias,
                                                      block.ln_2.weight, block.ln_2.bias)
                x, h = ops.mlp_residual_layer_norm(x, h, ml.c_fc.weight, ml.c_fc.bias, ml.c_proj.weight,
                                                   ml.c_proj.bias, nxt.weight, nxt.bias)
                continue
            a = at(h, fuse_out_bias=True)
            x, h = ops.add_layer_norm(x, a, block.ln_2.weight, block.ln_2.bias, r_bias=at.c_proj.bias)
            m = ml(h, fuse_out_bias=True)
            x, h = ops.add_layer_norm(x, m, nxt.weight, nxt.bias, r_bias=ml.c_proj.bias)
        x = h
        if targets is not None:
            loss = ops.linear_cross_entropy(x.reshape(B * T, -1), self.lm_head.weight,
                                            targets.reshape(-1), ignore_index=-1)
            return None, loss
        logits = self.lm_head(x[:, [-1], :])
        return logits, None

    @property
    def context_len(self):
        return self.config.block_size

    def new_cache(self, batch, max_len=None, kv_dtype="bf16"):
        """An empty :class:`KVCache` for this model on its device (``max_len`` <= block_size);
        ``kv_dtype="fp8"`` stores e4m3 bytes with one scale per (token, head)."""
        cfg = self.config
        w = self.lm_head.weight
        return KVCache(cfg.n_layer, batch, min(max_len or cfg.block_size, cfg.block_size), cfg.n_head,
                       cfg.head_dim, device=w.device, dtype=w.dtype, kv_dtype=kv_dtype)

    @torch.no_grad()
    def forward_cached(self, idx, cache, weights=None):
        """Logits (B, vocab) of the last position of ``idx`` (B, T), given the ``cache.pos`` tokens
        already in ``cache``; appends this call's keys / values.  T > 1 is a (chunked) prefill
        through the flash forward, T == 1 a decode step through ``ops.attention_decode``.  Plain
        ops throughout: the training-time fused residual sites have no place at M = B.
        ``weights`` maps names of :meth:`decode_projections` to quantised weights (anything with
        ``dequant``: ``ops.Fp8Weight``, ``ops.Mxfp4Weight``): such a
        projection runs on its dequantised weight, one transient at a time (the embedding tables
        stay the model's).  An FP8 ``cache`` (``new_cache(kv_dtype="fp8")``) takes the
        appended keys / values quantised with their scales, and a T > 1 call attends the stored
        values dequantised (``cache.dense_layer``): what the decode steps will read."""
        B, T = idx.shape
        cfg, tr = self.config, self.transformer
        assert cache.pos + T <= cfg.block_size, f"sequence {cache.pos + T} > block_size {cfg.block_size}"
        pos = cache.begin(T)
        blocks = tr.h
        H, D = cfg.n_head, cfg.head_dim
        x = ops.add_broadcast(F.embedding(idx, tr.wte.weight), tr.wpe.weight[pos:pos + T])
        h = blocks[0].ln_1(x)
        ws = session_weights(self, weights)
        for i, block in enumerate(blocks):
            at, ml = block.attn, block.mlp
            w_qkv, w_o, w_fc, w_pr = (at.c_attn.weight, at.c_proj.weight, ml.c_fc.weight, ml.c_proj.weight) \
                if ws is None else ws[4 * i:4 * i + 4]
            qkv = ops.linear(h, dense(w_qkv, h.dtype), at.c_attn.bias).view(B, T, 3, H, D)
            kc, vc = cache.layer(i)
            ks, vs = cache.layer_scales(i)  # (None, None) unless the cache is FP8
            ops.kv_append(qkv[:, :, 1], qkv[:, :, 2], kc, vc, cache.start, k_scale=ks, v_scale=vs)
            end = pos + T  # the host's bound of the length: the key split is planned from it
            if T == 1:
                if ks is not None:
                    ks, vs = ks[:, :, :end], vs[:, :, :end]
                y = ops.attention_decode(qkv[:, 0, 0], kc[:, :end], vc[:, :end], cache.lens, k_scale=ks, v_scale=vs)
            else:  # an FP8 cache is attended as stored (dequantised): what the decode steps will see
                y = ops.attention(qkv[:, :, 0], *cache.dense_layer(i, end, h.dtype), causal=True)
            a = ops.linear(y.reshape(B, T, H * D), dense(w_o, h.dtype), at.c_proj.bias)
            x, h = ops.add_layer_norm(x, a, block.ln_2.weight, block.ln_2.bias)
            m = ops.mlp(h, dense(w_fc, h.dtype), ml.c_fc.bias, dense(w_pr, h.dtype), ml.c_proj.bias)
            nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else tr.ln_f
            x, h = ops.add_layer_norm(x, m, nxt.weight, nxt.bias)
        w_head = self.lm_head.weight if ws is None else ws[-1]
        return ops.linear(h[:, -1, :].contiguous(), dense(w_head, h.dtype))

    def decode_projections(self):
        """(name, weight) of every projection of :meth:`decode_step`."""
        for i, blk in enumerate(self.transformer.h):
            yield f"h.{i}.attn.c_attn", blk.attn.c_attn.weight
            yield f"h.{i}.attn.c_proj", blk.attn.c_proj.weight
            yield f"h.{i}.mlp.c_fc", blk.mlp.c_fc.weight
            yield f"h.{i}.mlp.c_proj", blk.mlp.c_proj.weight
        yield "lm_head", self.lm_head.weight

    def decode_step(self, tokens, cache, logits_out, weights=None):
        """:meth:`forward_cached` at T = 1 for a :class:`DecodeSession`, on device state only:
        the logits of ``tokens`` (B, 1) at position ``cache.start`` go into ``logits_out``.  Every
        projection is one ``ops.linear_decode`` with the norm in its prologue and the bias /
        GELU / residual in its epilogue; the session has advanced ``cache.start`` / ``cache.lens``.
        A projection named in ``weights`` (name -> ``ops.Fp8Weight`` or ``ops.Mxfp4Weight``) streams
        that weight.

        ``tokens`` (B, Tq) with B Tq <= 16 is a speculative verify step: token t of row b sits at
        position ``cache.start[b] + t``, every projection runs on the B Tq rows, the Tq keys /
        values are appended by one ``ops.kv_append`` and attended by one
        ``ops.attention_decode_multi``, and ``logits_out`` is (B Tq, vocab).  A position past the
        end of the cache (near the context limit) takes the last position's embedding and is
        skipped by the append: its logits are finite and never used."""
        cfg, tr = self.config, self.transformer
        (B, Tq), H, D = tokens.shape, cfg.n_head, cfg.head_dim
        if Tq == 1:
            x = F.embedding(tokens[:, 0], tr.wte.weight) + F.embedding(cache.start, tr.wpe.weight)
        else:
            pos = cache.start.view(B, 1) + torch.arange(Tq, device=tokens.device, dtype=cache.start.dtype)
            x = F.embedding(tokens, tr.wte.weight) + F.embedding(pos.clamp_(max=cfg.block_size - 1), tr.wpe.weight)
            x = x.view(B * Tq, -1)
        ws = session_weights(self, weights)
        for i, blk in enumerate(tr.h):
            at, ml = blk.attn, blk.mlp
            w_qkv, w_o, w_fc, w_pr = (at.c_attn.weight, at.c_proj.weight, ml.c_fc.weight, ml.c_proj.weight) \
                if ws is None else ws[4 * i:4 * i + 4]
            qkv = ops.linear_decode(x, w_qkv, at.c_attn.bias, norm="layer", norm_weight=blk.ln_1.weight,
                                    norm_bias=blk.ln_1.bias).view(B, Tq, 3, H, D)
            kc, vc = cache.layer(i)
            ks, vs = cache.layer_scales(i)
            ops.kv_append(qkv[:, :, 1], qkv[:, :, 2], kc, vc, cache.start, k_scale=ks, v_scale=vs)
            # the whole cache view: the key split is planned from max_len once and never changes
            if Tq == 1:
                y = ops.attention_decode(qkv[:, 0, 0], kc, vc, cache.lens, k_scale=ks, v_scale=vs)
            else:
                y = ops.attention_decode_multi(qkv[:, :, 0], kc, vc, cache.lens)
            x = ops.linear_decode(y.view(B * Tq, H * D), w_o, at.c_proj.bias, residual=x)
            h = ops.linear_decode(x, w_fc, ml.c_fc.bias, norm="layer", norm_weight=blk.ln_2.weight,
                                  norm_bias=blk.ln_2.bias, act="gelu")
            x = ops.linear_decode(h, w_pr, ml.c_proj.bias, residual=x)
        w_head = self.lm_head.weight if ws is None else ws[-1]
        ops.linear_decode(x, w_head, norm="layer", norm_weight=tr.ln_f.weight, norm_bias=tr.ln_f.bias,
                          out=logits_out)


def build_gpt2(preset="gpt2", **overrides):
    kw = dict(PRESETS[preset])
    kw.update(overrides)
    return GPT(GPTConfig(**kw))

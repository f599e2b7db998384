"""Llama-family decoder (RMSNorm, RoPE, SwiGLU, GQA) on the orion_amd op layer.

BASELINE.json configs 4/5 name a Llama-2-7B-shape model at seq 4096 (SURVEY.md
§2.11: L=32, d=4096, H=32, head_dim=128, FFN 11008, vocab 32000, RoPE theta
1e4).  MI355X-first layout:

* ONE fused QKV projection ``(B, T, (Hq + 2 Hkv) D)``; RoPE reads the q/k
  slices through strides and writes contiguous rotated copies; V is consumed
  in place by the flash-attention kernel (strided view) -- no split/transpose;
* ONE fused gate|up projection ``(B, T, 2F)`` feeding the packed SwiGLU kernel;
* residual add + RMSNorm fused (one kernel forward, one backward), like GPT-2's
  add+LayerNorm;
* parameter names follow the Hugging Face Llama layout where the shapes allow
  (``model.layers.{i}.self_attn.o_proj`` ...), with the fused ``qkv_proj`` /
  ``gate_up_proj`` documented in :func:`split_fused_state_dict`.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops import reference as ref
from .generation import Generation, dense, session_weights
from .kv_cache import KVCache


@dataclass
class LlamaConfig:
    vocab_size: int = 32000
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 32
    ffn_dim: int = 11008
    max_seq_len: int = 4096
    rope_theta: float = 10000.0
    norm_eps: float = 1e-5
    tie_embeddings: bool = False

    @property
    def head_dim(self):
        return self.dim // self.n_heads

    def to_dict(self):
        return asdict(self)


PRESETS = {
    "llama-tiny": dict(vocab_size=512, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn_dim=512,
                       max_seq_len=256),
    "llama2-7b": dict(),
    "llama2-13b": dict(dim=5120, n_layers=40, n_heads=40, n_kv_heads=40, ffn_dim=13824),
    "llama3-8b": dict(vocab_size=128256, n_kv_heads=8, ffn_dim=14336, max_seq_len=8192,
                      rope_theta=500000.0),
    "llama-1b-gqa": dict(dim=2048, n_layers=16, n_heads=16, n_kv_heads=4, ffn_dim=5632),
}


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        return ops.rms_norm(x, self.weight, self.eps)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.n_heads, self.n_kv, self.hd = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        self.qkv_proj = nn.Linear(cfg.dim, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim, bias=False)
        self.o_proj = nn.Linear(cfg.n_heads * cfg.head_dim, cfg.dim, bias=False)

    def attend(self, x, cos, sin, pos0=0):
        """QKV projection + RoPE + attention, before o_proj: (B, T, Hq * D).  On the GPU with
        D = 128 the rotation rides in the projection's epilogue."""
        B, T, _ = x.shape
        o = ops.linear_rope_attention(x, self.qkv_proj.weight, self.n_heads, self.n_kv, cos, sin, pos0)
        return o.reshape(B, T, -1)

    def forward(self, x, cos, sin, pos0=0):
        return ops.linear(self.attend(x, cos, sin, pos0), self.o_proj.weight)


class FeedForward(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.gate_up_proj = nn.Linear(cfg.dim, 2 * cfg.ffn_dim, bias=False)
        self.down_proj = nn.Linear(cfg.ffn_dim, cfg.dim, bias=False)

    def forward(self, x):
        return ops.swiglu_mlp(x, self.gate_up_proj.weight, self.down_proj.weight)


class DecoderLayer(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.input_layernorm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.self_attn = Attention(cfg)
        self.post_attention_layernorm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.mlp = FeedForward(cfg)


class Llama(nn.Module, Generation):
    """``forward(idx, targets)`` -> (logits|None, loss|None), same contract as GPT."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.config = cfg
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.dim)
        self.layers = nn.ModuleList([DecoderLayer(cfg) for _ in range(cfg.n_layers)])
        self.norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.lm_head = nn.Linear(cfg.dim, cfg.vocab_size, bias=False)
        if cfg.tie_embeddings:
            self.lm_head.weight = self.embed_tokens.weight
        cos, sin = ref.rope_tables(cfg.max_seq_len, cfg.head_dim, cfg.rope_theta)
        self.register_buffer("rope_cos", cos, persistent=False)
        self.register_buffer("rope_sin", sin, persistent=False)
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self):
        std = 0.02
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0)
            elif name.endswith(("o_proj.weight", "down_proj.weight")):
                p.normal_(0.0, std / math.sqrt(2 * self.config.n_layers))
            else:
                p.normal_(0.0, std)

    def num_params(self, non_embedding=False):
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.embed_tokens.weight.numel()
        return n

    def flops_per_token(self, seq_len=None):
        cfg = self.config
        T = seq_len or cfg.max_seq_len
        return 6 * self.num_params(non_embedding=True) + 12 * cfg.n_layers * cfg.dim * T

    def forward(self, idx, targets=None, pos0=0):
        B, T = idx.shape
        assert pos0 + T <= self.config.max_seq_len
        x = ops.token_embedding(idx, self.embed_tokens.weight)
        cos, sin = self.rope_cos, self.rope_sin
        layers = self.layers
        h = layers[0].input_layernorm(x)
        # the o_proj / down_proj GEMMs add the residual stream in their epilogue and the
        # RMSNorm reads only the new stream (ops/residual.py; other backends: add_rms_norm)
        for i, layer in enumerate(layers):
            at, ff, pln = layer.self_attn, layer.mlp, layer.post_attention_layernorm
            x, h = ops.linear_residual_rms_norm(x, at.attend(h, cos, sin, pos0), at.o_proj.weight,
                                                pln.weight, pln.eps)
            nxt = layers[i + 1].input_layernorm if i + 1 < len(layers) else self.norm
            x, h = ops.swiglu_residual_rms_norm(x, h, ff.gate_up_proj.weight, ff.down_proj.weight,
                                                nxt.weight, nxt.eps)
        if targets is not None:
            loss = ops.linear_cross_entropy(h.reshape(B * T, -1), self.lm_head.weight,
                                            targets.reshape(-1), ignore_index=-1)
            return None, loss
        logits = ops.linear(h[:, [-1], :], self.lm_head.weight)
        return logits, None

    @property
    def context_len(self):
        return self.config.max_seq_len

    def new_cache(self, batch, max_len=None, kv_dtype="bf16"):
        """An empty :class:`KVCache` for this model on its device (``max_len`` <= max_seq_len);
        ``kv_dtype="fp8"`` stores e4m3 bytes with one scale per (token, KV head)."""
        cfg = self.config
        w = self.lm_head.weight
        return KVCache(cfg.n_layers, batch, min(max_len or cfg.max_seq_len, cfg.max_seq_len), cfg.n_kv_heads,
                       cfg.head_dim, device=w.device, dtype=w.dtype, kv_dtype=kv_dtype)

    @torch.no_grad()
    def forward_cached(self, idx, cache, weights=None):
        """Logits (B, vocab) of the last position of ``idx`` (B, T), given the ``cache.pos`` tokens
        already in ``cache``; appends this call's rotated keys and values.  T > 1 is a (chunked)
        prefill through the flash forward, T == 1 a decode step through ``ops.attention_decode``.
        Plain ops throughout: the training-time fused residual sites have no place at M = B.
        ``weights`` maps names of :meth:`decode_projections` to quantised weights (anything with
        ``dequant``: ``ops.Fp8Weight``, ``ops.Mxfp4Weight``): such a
        projection runs on its dequantised weight, one transient at a time (the embedding table
        stays the model's).  An FP8 ``cache`` (``new_cache(kv_dtype="fp8")``) takes the
        appended keys / values quantised with their scales, and a T > 1 call attends the stored
        values dequantised (``cache.dense_layer``): what the decode steps will read."""
        B, T = idx.shape
        cfg = self.config
        assert cache.pos + T <= cfg.max_seq_len
        pos = cache.begin(T)
        end = pos + T  # the host's bound of the length: the key split is planned from it
        Hq, Hkv, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        cos, sin = self.rope_cos, self.rope_sin
        layers = self.layers
        x = ops.token_embedding(idx, self.embed_tokens.weight)
        h = layers[0].input_layernorm(x)
        ws = session_weights(self, weights)
        for i, layer in enumerate(layers):
            at, ff, pln = layer.self_attn, layer.mlp, layer.post_attention_layernorm
            w_qkv, w_o, w_gu, w_dn = (at.qkv_proj.weight, at.o_proj.weight, ff.gate_up_proj.weight,
                                      ff.down_proj.weight) if ws is None else ws[4 * i:4 * i + 4]
            qkv = ops.linear(h, dense(w_qkv, h.dtype)).view(B, T, Hq + 2 * Hkv, D)
            kc, vc = cache.layer(i)
            ks, vs = cache.layer_scales(i)  # (None, None) unless the cache is FP8
            q = ops.kv_append(qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], kc, vc, cache.start,
                              q=qkv[:, :, :Hq], cos=cos, sin=sin, k_scale=ks, v_scale=vs)
            if T == 1:
                if ks is not None:
                    ks, vs = ks[:, :, :end], vs[:, :, :end]
                y = ops.attention_decode(q[:, 0], kc[:, :end], vc[:, :end], cache.lens, k_scale=ks, v_scale=vs)
            else:  # an FP8 cache is attended as stored (dequantised): what the decode steps will see
                y = ops.attention(q, *cache.dense_layer(i, end, h.dtype), causal=True)
            a = ops.linear(y.reshape(B, T, Hq * D), dense(w_o, h.dtype))
            x, h = ops.add_rms_norm(x, a, pln.weight, pln.eps)
            m = ops.swiglu_mlp(h, dense(w_gu, h.dtype), dense(w_dn, h.dtype))
            nxt = layers[i + 1].input_layernorm if i + 1 < len(layers) else self.norm
            x, h = ops.add_rms_norm(x, m, nxt.weight, nxt.eps)
        w_head = self.lm_head.weight if ws is None else ws[-1]
        return ops.linear(h[:, -1, :].contiguous(), dense(w_head, h.dtype))

    def decode_projections(self):
        """(name, weight) of every projection of :meth:`decode_step`."""
        for i, layer in enumerate(self.layers):
            yield f"layers.{i}.self_attn.qkv_proj", layer.self_attn.qkv_proj.weight
            yield f"layers.{i}.self_attn.o_proj", layer.self_attn.o_proj.weight
            yield f"layers.{i}.mlp.gate_up_proj", layer.mlp.gate_up_proj.weight
            yield f"layers.{i}.mlp.down_proj", layer.mlp.down_proj.weight
        yield "lm_head", self.lm_head.weight

    def decode_step(self, tokens, cache, logits_out, weights=None):
        """:meth:`forward_cached` at T = 1 for a :class:`DecodeSession`, on device state only:
        the logits of ``tokens`` (B, 1) at position ``cache.start`` go into ``logits_out``.  Every
        projection is one ``ops.linear_decode`` with the norm in its prologue and the SwiGLU /
        residual in its epilogue; the session has advanced ``cache.start`` / ``cache.lens``.
        A projection named in ``weights`` (name -> ``ops.Fp8Weight`` or ``ops.Mxfp4Weight``) streams
        that weight.

        ``tokens`` (B, Tq) with B Tq <= 16 is a speculative verify step: token t of row b sits at
        position ``cache.start[b] + t``, every projection runs on the B Tq rows, the Tq keys /
        values are appended (and rotated) by one ``ops.kv_append`` and attended by one
        ``ops.attention_decode_multi``, and ``logits_out`` is (B Tq, vocab).  A position past the
        end of the cache is skipped by the append (its q is zero): its logits are never used."""
        cfg = self.config
        (B, Tq), Hq, Hkv, D = tokens.shape, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        cos, sin = self.rope_cos, self.rope_sin
        x = F.embedding(tokens[:, 0] if Tq == 1 else tokens.reshape(B * Tq), self.embed_tokens.weight)
        ws = session_weights(self, weights)
        for i, layer in enumerate(self.layers):
            at, ff = layer.self_attn, layer.mlp
            ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
            w_qkv, w_o, w_gu, w_dn = (at.qkv_proj.weight, at.o_proj.weight, ff.gate_up_proj.weight,
                                      ff.down_proj.weight) if ws is None else ws[4 * i:4 * i + 4]
            qkv = ops.linear_decode(x, w_qkv, norm="rms", norm_weight=ln1.weight,
                                    eps=ln1.eps).view(B, Tq, Hq + 2 * Hkv, D)
            kc, vc = cache.layer(i)
            ks, vs = cache.layer_scales(i)
            q = ops.kv_append(qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], kc, vc, cache.start,
                              q=qkv[:, :, :Hq], cos=cos, sin=sin, k_scale=ks, v_scale=vs)
            if Tq == 1:
                y = ops.attention_decode(q[:, 0], kc, vc, cache.lens, k_scale=ks, v_scale=vs)
            else:
                y = ops.attention_decode_multi(q, kc, vc, cache.lens)
            x = ops.linear_decode(y.view(B * Tq, Hq * D), w_o, residual=x)
            h = ops.linear_decode(x, w_gu, norm="rms", norm_weight=ln2.weight, eps=ln2.eps,
                                  act="swiglu")
            x = ops.linear_decode(h, w_dn, residual=x)
        w_head = self.lm_head.weight if ws is None else ws[-1]
        ops.linear_decode(x, w_head, norm="rms", norm_weight=self.norm.weight, eps=self.norm.eps,
                          out=logits_out)


def build_llama(preset="llama2-7b", **overrides):
    kw = dict(PRESETS[preset])
    kw.update(overrides)
    return Llama(LlamaConfig(**kw))


def split_fused_state_dict(sd, cfg: LlamaConfig):
    """Fused qkv_proj / gate_up_proj -> Hugging Face q/k/v_proj, gate/up_proj tensors."""
    out = {}
    hq, hk, hd = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    for k, v in sd.items():
        if k.endswith("qkv_proj.weight"):
            base = k[: -len("qkv_proj.weight")]
            q, kk, vv = torch.split(v, [hq * hd, hk * hd, hk * hd], dim=0)
            out[base + "q_proj.weight"], out[base + "k_proj.weight"], out[base + "v_proj.weight"] = q, kk, vv
        elif k.endswith("gate_up_proj.weight"):
            base = k[: -len("gate_up_proj.weight")]
            g, u = v.chunk(2, dim=0)
            out[base + "gate_proj.weight"], out[base + "up_proj.weight"] = g, u
        else:
            out[k] = v
    return out

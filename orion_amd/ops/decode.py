"""Generation-time ops over the HIP kernels of csrc/attn_decode.hip: single-query attention
against a key/value cache (split over keys, lengths read on the device) and the cache append
with optional RoPE.  Inference only: there is no backward, and an input that requires grad
while gradients are enabled is an error rather than a silently dropped graph."""
from __future__ import annotations

import math

import torch

from ._ext import C


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("attention_decode / kv_append are inference-only ops: inputs must not "
                           "require grad (run under torch.no_grad())")


def attention_decode_hip(q, k_cache, v_cache, kv_lens, scale=None, splits=0):
    """q (B, Hq, D), caches (B, Tmax, Hkv, D), kv_lens (B,) int32 on the device -> (B, Hq, D).
    ``splits = 0`` lets the host pick the key split from Tmax: pass a view of the cache cut at
    the host's upper bound of the length."""
    _no_grad(q, k_cache, v_cache)
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    return C().attn_decode(q, k_cache, v_cache, kv_lens, scale, int(splits))


def kv_append_hip(k_new, v_new, k_cache, v_cache, kv_lens, q=None, cos=None, sin=None):
    """One launch: k_new / v_new into the caches at kv_lens[b] + t (k rotated when tables are
    given); returns the rotated q, or None without q."""
    _no_grad(k_new, v_new, k_cache, v_cache, q)
    q_rot = C().kv_append(k_new, v_new, k_cache, v_cache, kv_lens, q, cos, sin)
    return q_rot if q is not None else None


def attention_decode_torch(q, k_cache, v_cache, kv_lens, scale=None):
    """Stock PyTorch: SDPA on each row's valid slice (reads the lengths on the host)."""
    _no_grad(q, k_cache, v_cache)
    B, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=q.dtype, device=q.device)
    for b, n in enumerate(kv_lens.tolist()):
        n = max(0, min(int(n), Tmax))
        if n == 0:
            continue
        k = k_cache[b, :n].transpose(0, 1)  # (Hkv, n, D)
        v = v_cache[b, :n].transpose(0, 1)
        if rep > 1:
            k, v = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
        out[b] = torch.nn.functional.scaled_dot_product_attention(
            q[b][None, :, None, :], k[None], v[None], scale=scale)[0, :, 0]
    return out

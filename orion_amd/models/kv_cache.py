"""Key/value cache for generation: one buffer for every layer, lengths on the device.

``GPT.forward_cached`` / ``Llama.forward_cached`` call :meth:`KVCache.begin` once per model
forward; every layer then appends at ``cache.start`` (``ops.kv_append``) and attends up to
``cache.lens`` (``ops.attention_decode``), so a decode loop changes no launch parameter and
reads nothing back from the device.
"""
from __future__ import annotations

import torch


KV_DTYPES = ("bf16", "fp8")


class KVCache:
    """``buf`` (n_layer, 2, B, Tmax, Hkv, D) holds k (index 0) and v (index 1) of every layer.

    ``lens`` (B,) int32 on the device is each row's valid length *including* the tokens of the
    forward in progress, ``start`` (B,) the position its first token is appended at.  Both are
    updated once per forward by :meth:`begin`, not per layer.  ``pos`` is the host mirror of the
    (uniform) length; it is what raises, before any launch, when a forward would not fit.

    ``kv_dtype="fp8"`` keeps ``buf`` as ``float8_e4m3fn`` bytes (zero-filled, the same shape) with
    ``scales`` (n_layer, 2, B, Hkv, Tmax) fp32 (filled with 1): one scale per (token, KV head),
    value = scale * byte (``ops.quantize_kv_fp8``), (D + 4) / 2D of the bf16 bytes.  Tokens are
    innermost in ``scales``: the keys one wave of the decode kernel walks are consecutive tokens of
    one head, so their scales are one contiguous run.  With the default ``"bf16"``, ``scales`` is
    None and ``dtype`` is the buffer's dtype as always."""

    def __init__(self, n_layer, batch, max_len, n_kv_heads, head_dim, device=None, dtype=torch.bfloat16,
                 kv_dtype="bf16"):
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        self.max_len = int(max_len)
        self.kv_dtype = kv_dtype
        self.scales = None
        if kv_dtype == "fp8":
            dtype = torch.float8_e4m3fn
            self.scales = torch.ones(n_layer, 2, batch, n_kv_heads, self.max_len, device=device, dtype=torch.float32)
        self.buf = torch.zeros(n_layer, 2, batch, self.max_len, n_kv_heads, head_dim, device=device, dtype=dtype)
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.start = torch.zeros(batch, dtype=torch.int32, device=device)
        self.pos = 0

    @property
    def n_layer(self):
        return self.buf.shape[0]

    @property
    def batch(self):
        return self.buf.shape[2]

    @property
    def nbytes(self):
        """Bytes held by the keys and values: the buffer and, for FP8, the scales."""
        n = self.buf.numel() * self.buf.element_size()
        if self.scales is not None:
            n += self.scales.numel() * self.scales.element_size()
        return n

    def layer(self, i):
        """(k_cache, v_cache) of layer i, each (B, Tmax, Hkv, D): bf16 values or FP8 bytes."""
        return self.buf[i, 0], self.buf[i, 1]

    def layer_scales(self, i):
        """(k_scale, v_scale) of layer i, each (B, Hkv, Tmax) fp32; (None, None) for a bf16 cache."""
        if self.scales is None:
            return None, None
        return self.scales[i, 0], self.scales[i, 1]

    def dense_layer(self, i, end, dtype):
        """k and v of the first ``end`` positions of layer i as plain tensors (B, end, Hkv, D): the
        views themselves for a bf16 cache; for FP8 ``bytes.float() * scale`` cast once to ``dtype``,
        transients made with torch ops."""
        k, v = self.buf[i, 0, :, :end], self.buf[i, 1, :, :end]
        if self.scales is None:
            return k, v
        from ..ops.fp8 import dequantize_kv_fp8
        return (dequantize_kv_fp8(k, self.scales[i, 0, :, :, :end], dtype),
                dequantize_kv_fp8(v, self.scales[i, 1, :, :, :end], dtype))

    def check_room(self, T):
        """Raise ``ValueError``, on the host and before any launch, unless T >= 1 more tokens fit."""
        if T < 1 or self.pos + T > self.max_len:
            raise ValueError(f"KVCache overflow: {self.pos} cached + {T} new tokens > max_len {self.max_len}")

    def begin(self, T):
        """Reserve T positions for one model forward; returns the position of its first token."""
        T = int(T)
        self.check_room(T)
        pos = self.pos
        self.start.copy_(self.lens)
        self.lens.add_(T)
        self.pos = pos + T
        return pos

    def reset(self):
        self.lens.zero_()
        self.start.zero_()
        self.pos = 0

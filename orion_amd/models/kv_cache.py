"""Key/value cache for generation: one buffer for every layer, lengths on the device.

``GPT.forward_cached`` / ``Llama.forward_cached`` call :meth:`KVCache.begin` once per model
forward; every layer then appends at ``cache.start`` (``ops.kv_append``) and attends up to
``cache.lens`` (``ops.attention_decode``), so a decode loop changes no launch parameter and
reads nothing back from the device.
"""
from __future__ import annotations

import torch


class KVCache:
    """``buf`` (n_layer, 2, B, Tmax, Hkv, D) holds k (index 0) and v (index 1) of every layer.

    ``lens`` (B,) int32 on the device is each row's valid length *including* the tokens of the
    forward in progress, ``start`` (B,) the position its first token is appended at.  Both are
    updated once per forward by :meth:`begin`, not per layer.  ``pos`` is the host mirror of the
    (uniform) length; it is what raises, before any launch, when a forward would not fit."""

    def __init__(self, n_layer, batch, max_len, n_kv_heads, head_dim, device=None, dtype=torch.bfloat16):
        self.max_len = int(max_len)
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

    def layer(self, i):
        """(k_cache, v_cache) of layer i, each (B, Tmax, Hkv, D)."""
        return self.buf[i, 0], self.buf[i, 1]

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

"""What :class:`GPT` and :class:`Llama` share in generation: the sampling rule and the loop that
hands over from the key/value cache (or a :class:`DecodeSession`) to the sliding window.

A model inherits :class:`Generation` and says what is its own: ``context_len``, ``new_cache``,
``forward_cached``, and for the fused decode step ``decode_step`` and ``decode_projections``.
"""
from __future__ import annotations

import torch


def session_weights(model, weights):
    """The weights of ``model.decode_projections()`` in that order, each replaced by the entry of
    the mapping ``weights`` (name -> ``ops.Fp8Weight`` or ``ops.Mxfp4Weight``) that carries its
    name; None without a mapping, and the caller then reads the parameters as it always did."""
    if weights is None:
        return None
    return [weights.get(name, p) for name, p in model.decode_projections()]


def dense(weight, dtype):
    """A weight that the plain ops take: a quantised one (anything with ``dequant``: an
    ``ops.Fp8Weight``, an ``ops.Mxfp4Weight``) dequantised to ``dtype`` (a transient), anything
    else as it is."""
    return weight.dequant(dtype) if hasattr(weight, "dequant") else weight


def sample_logits(logits, temperature=1.0, top_k=None):
    """The models' sampling rule on (B, vocab) logits -> (B, 1) token ids: temperature, the top-k
    threshold (ties kept), softmax, one draw per row from torch's default generator."""
    logits = logits.float() / max(temperature, 1e-6)
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits[logits < v[:, [-1]]] = -float("inf")
    return torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1)


class Generation:
    """``generate`` and ``decode_session`` of a model with a :class:`KVCache`."""

    def decode_session(self, batch, max_len=None, graph=False, sampler="torch", weights="bf16", kv="bf16",
                       speculative=None, ngram=3, draft="ngram"):
        """A :class:`DecodeSession` for this model: the fused decode step, captured when ``graph``;
        ``sampler="device"`` draws the tokens with ``ops.sample_tokens`` inside that step,
        ``weights="fp8"`` decodes from per-row e4m3 copies of the projection weights,
        ``weights="mxfp4"`` from MXFP4 copies (e2m1 codes, one e8m0 scale per 32 along K), and
        ``kv="fp8"`` keeps the key/value cache as e4m3 bytes with one scale per (token, KV head).
        ``speculative=k`` verifies k guessed tokens per step (``draft="ngram"`` with ``ngram``, or a
        (batch, L) tensor of guesses by position) and emits the plain loop's tokens."""
        from .decode_session import DecodeSession
        if speculative is None:
            return DecodeSession(self, batch, max_len, graph=graph, sampler=sampler, weights=weights, kv=kv)
        return DecodeSession(self, batch, max_len, graph=graph, sampler=sampler, weights=weights, kv=kv,
                             speculative=speculative, ngram=ngram, draft=draft)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, temperature=1.0, top_k=None, use_cache=False, sampler="torch",
                 weights="bf16", kv="bf16", speculative=None, ngram=3, draft="ngram"):
        """nanoGPT's sampling loop.  ``use_cache=True`` keeps every layer's keys / values
        (:class:`KVCache`): the prompt is prefilled once and each new token costs one single-token
        forward.  Tokens beyond the context limit (``block_size`` / ``max_seq_len``) take the
        uncached sliding-window loop below: cropping the window shifts the positions, which
        invalidates a cache.  ``use_cache="fused"`` runs the cached tokens through a
        :class:`DecodeSession` (the fused skinny-linear decode step), ``"graph"`` additionally
        replays that step from one captured HIP graph.  With either, ``sampler="device"`` draws
        the session's tokens with ``ops.sample_tokens`` inside the step (seeded from torch's
        default generator) instead of stock torch ops between the steps, and ``weights="fp8"``
        makes the session quantise the projection weights once (``ops.quantize_fp8``) and run the
        prompt and every cached token on them; ``weights="mxfp4"`` does so with
        ``ops.quantize_mxfp4`` (4.25 bits per weight, every projection's K % 32 == 0).  The
        sliding-window loop beyond the context limit keeps using the model's own (unquantised)
        weights, as it keeps clear of the session.
        ``kv="fp8"`` (with ``use_cache`` True, ``"fused"`` or ``"graph"``) keeps the cache as e4m3
        bytes with one fp32 scale per (token, KV head): about half the cache's memory and bytes per
        step; the sliding-window loop has no cache and does not change.
        ``speculative=k`` (``use_cache`` ``"fused"`` or ``"graph"``, ``sampler="device"``, a bf16
        cache, B (k + 1) <= 16) makes the session verify k guessed tokens per step and keep those
        that equal its own draws (:class:`DecodeSession`): the same tokens as without it under the
        same ``torch.manual_seed``, in fewer steps when the guesses are good.  ``draft="ngram"``
        guesses the continuation of the latest earlier occurrence of the last ``ngram`` tokens;
        a (B, L) int64 tensor gives the guesses by sequence position.  The sliding-window loop
        does not change."""
        fused = isinstance(use_cache, str)
        if fused and use_cache not in ("fused", "graph"):
            raise ValueError(f"use_cache must be False, True, 'fused' or 'graph', got {use_cache!r}")
        if sampler not in ("torch", "device"):
            raise ValueError(f"sampler must be 'torch' or 'device', got {sampler!r}")
        if sampler == "device" and not fused:
            raise ValueError("sampler='device' samples inside the fused decode step: use_cache must be 'fused' "
                             f"or 'graph', got {use_cache!r}")
        if weights not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"weights must be 'bf16', 'fp8' or 'mxfp4', got {weights!r}")
        if weights != "bf16" and not fused:
            raise ValueError(f"weights='{weights}' decodes through the fused decode step: use_cache must be 'fused' "
                             f"or 'graph', got {use_cache!r}")
        if kv not in ("bf16", "fp8"):
            raise ValueError(f"kv must be 'bf16' or 'fp8', got {kv!r}")
        if kv == "fp8" and not use_cache:
            raise ValueError("kv='fp8' is the key/value cache's format: use_cache must be True, 'fused' or "
                             f"'graph', got {use_cache!r}")
        B, T = idx.shape
        if speculative is not None:
            from .decode_session import check_speculative
            if not fused:
                raise ValueError("speculative decoding runs through the fused decode step: use_cache must be "
                                 f"'fused' or 'graph', got {use_cache!r}")
            check_speculative(speculative, ngram, draft, B, sampler, kv)
        limit = self.context_len
        if use_cache and max_new_tokens > 0 and T < limit:
            n = min(max_new_tokens, limit - T + 1)  # the n-th token is drawn from position limit - 1's logits
            if fused:
                sess = self.decode_session(B, T + n - 1, graph=use_cache == "graph", sampler=sampler,
                                           weights=weights, kv=kv, speculative=speculative, ngram=ngram, draft=draft)
                idx = sess.generate(idx, n, temperature, top_k)
            else:
                cache = self.new_cache(B, T + n - 1, kv_dtype=kv)
                logits = self.forward_cached(idx, cache)
                for step in range(n):
                    nxt = sample_logits(logits, temperature, top_k)
                    idx = torch.cat((idx, nxt), dim=1)
                    if step + 1 < n:
                        logits = self.forward_cached(nxt, cache)
            max_new_tokens -= n
        for _ in range(max_new_tokens):
            logits, _ = self(idx[:, -limit:])
            idx = torch.cat((idx, sample_logits(logits[:, -1, :], temperature, top_k)), dim=1)
        return idx

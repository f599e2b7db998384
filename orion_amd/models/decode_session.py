"""The decode step on the fused skinny-linear kernels, optionally replayed from a HIP graph.

``forward_cached`` runs a single-token step as ~9 launches per layer through plain ops, library
GEMMs among them, and is bound by the host's launch rate.  :class:`DecodeSession` runs the same
step as 6-7 in-tree launches per layer (``ops.linear_decode`` with the norm in its prologue and
the bias / activation / residual in its epilogue, ``ops.kv_append``, ``ops.attention_decode``)
and, with ``graph=True``, captures it once and replays it per token.  Everything the step reads
that changes from token to token lives in device memory: the token in a static buffer, the
append position and the attention length in ``cache.start`` / ``cache.lens`` (advanced inside
the step), so a replay needs no new launch parameter.  Prefill is the model's ``forward_cached``
on the session's cache and is never captured.
"""
from __future__ import annotations

import torch

from .. import ops
from ..ops.decode import MAX_ROWS as MAX_GRAPH_BATCH  # rows of ops.linear_decode's kernel
from . import generation


def check_speculative(speculative, ngram, draft, batch, sampler, kv):
    """Raise ``ValueError`` unless ``speculative`` is None or a speculative session of ``batch`` rows
    can be built with these settings."""
    if speculative is None:
        return
    k = int(speculative)
    if sampler != "device":
        raise ValueError(f"speculative decoding verifies the device sampler's draws: sampler must be 'device', "
                         f"got {sampler!r}")
    if kv != "bf16":
        raise ValueError(f"speculative decoding needs a bf16 key/value cache (the multi-query attention kernel "
                         f"has no FP8 variant), got kv={kv!r}")
    if k < 1 or int(batch) * (k + 1) > MAX_GRAPH_BATCH:
        raise ValueError(f"speculative must be >= 1 with batch * (speculative + 1) <= {MAX_GRAPH_BATCH} (the rows "
                         f"of the skinny linear kernel), got speculative={speculative} at batch {batch}")
    if isinstance(draft, torch.Tensor):
        if draft.dim() != 2 or draft.shape[0] != int(batch) or draft.dtype != torch.int64 or draft.shape[1] < 1:
            raise ValueError(f"draft must be 'ngram' or an int64 (batch, L) tensor, got {tuple(draft.shape)} "
                             f"{draft.dtype}")
    elif draft != "ngram":
        raise ValueError(f"draft must be 'ngram' or an int64 (batch, L) tensor, got {draft!r}")
    elif int(ngram) < 1:
        raise ValueError(f"ngram must be >= 1, got {ngram}")


class DecodeSession:
    """One key/value cache, a static (B, 1) token buffer and a static (B, vocab) logits buffer for
    a model that has ``new_cache``, ``forward_cached``, ``decode_step`` and ``decode_projections``
    (:class:`GPT`, :class:`Llama`).

    ``prefill(idx)`` feeds a prompt (in one or several chunks); ``step(tokens)`` appends one token
    per row and returns the logits buffer, which the next step overwrites.  With ``graph=True`` on
    the GPU the first ``step`` warms up on a side stream and captures the step on a single stream
    (a linear chain of in-tree kernels: no library GEMM is inside); every later ``step`` copies
    the tokens in and replays.  ``captures`` counts the graphs captured, ``replays`` the replays;
    :meth:`reset` empties the cache and keeps the graphs.

    ``sampler="device"`` makes :meth:`generate` draw the tokens with ``ops.sample_tokens`` on the
    device: the session then owns ``rng_seed`` (1,) int64, ``sample_params`` (2,) int32
    (temperature bits, top-k) and ``history`` (batch, max_len + 1) int64, and with ``graph=True``
    a second graph, the step followed by the sampling launch, that writes each new token into
    ``tokens`` for the next replay.  ``step`` and its step-only graph do not change; a session
    holds at most one graph of each kind.

    ``weights="fp8"`` quantises every weight of ``model.decode_projections()``, the LM head
    included, once at construction (``ops.quantize_fp8``: e4m3 bytes and one fp32 scale per row)
    and keeps them as ``qweights``, name -> ``ops.Fp8Weight``; ``weight_bytes`` is what they
    hold.  The step then streams those bytes (csrc/linear_decode_fp8.hip) and the prefill runs
    on their dequantised values, so the prompt and the generated tokens see one model.  The
    model's parameters are not modified and the embedding tables stay as they are (GPT-2's tied
    ``wte`` is quantised as the head only); activations, the cache, attention and sampling do
    not change.  ``weights="mxfp4"`` does the same with ``ops.quantize_mxfp4`` (OCP MXFP4: e2m1
    codes, one e8m0 scale per 32 along K, 4.25 bits per weight; ``qweights`` holds
    ``ops.Mxfp4Weight`` and the step runs csrc/linear_decode_mxfp4.hip); every projection then
    needs K % 32 == 0, checked at construction.  With the default ``"bf16"``, ``qweights`` is
    None, ``weight_bytes`` counts the model's own projection weights and the models are called
    exactly as without the keyword.

    ``kv="fp8"`` makes the cache a :class:`KVCache` with ``kv_dtype="fp8"``: the append quantises
    each head row to e4m3 bytes with one fp32 scale (csrc/attn_decode.hip) and the decode
    attention streams those bytes, (D + 4) / 2D of the bf16 cache's; ``cache_bytes`` is what the
    cache holds.  The step keeps its launches (the two cache ops change kernels), so a captured
    step stays one linear chain.  A prefill of more than one token attends the stored values of
    each layer dequantised to a transient (``KVCache.dense_layer``), so a chunked prompt and the
    decode steps see the same keys and values; the transient is one layer's k and v in the
    activation dtype at a time.  With the default ``"bf16"`` the cache is built as without the
    keyword.

    ``speculative=k`` (with ``sampler="device"``, a bf16 cache and batch (k + 1) <= 16) makes
    :meth:`generate` emit up to k + 1 tokens per step: k guesses are verified by one
    ``decode_step`` over the current token and the guesses, the target token of every one of the
    k + 1 positions is drawn with the Philox counter the plain loop uses at that position, and the
    longest prefix of guesses that equal those draws is kept (``ops.spec_accept``).  The tokens are
    therefore those of the plain ``sampler="device"`` loop under the same seed, token for token.
    The guesses come from ``ops.spec_draft`` on ``history`` (``draft="ngram"``: the continuation
    of the latest earlier occurrence of the last ``ngram`` tokens) or from ``draft`` (B, L) int64,
    guesses indexed by sequence position (read at clamped columns).  The session then also owns
    ``spec_tokens`` / ``spec_target`` (B, k + 1) int64, ``spec_logits`` (B (k + 1), vocab) and
    ``stop`` (B,) int32, ``history`` also receives the prompt at :meth:`prefill`, and the step
    (draft, forward, draws, accept) is one captured linear chain with ``graph=True``.  The rows'
    lengths differ between steps: the host reads ``cache.lens`` back once per step (the step's one
    synchronisation) and keeps ``cache.pos`` at their maximum.  ``spec_steps`` counts the verify
    steps and ``spec_emitted`` the tokens they produced.  With the default ``None`` nothing
    changes."""

    def __init__(self, model, batch, max_len=None, graph=False, sampler="torch", weights="bf16", kv="bf16",
                 speculative=None, ngram=3, draft="ngram"):
        if sampler not in ("torch", "device"):
            raise ValueError(f"sampler must be 'torch' or 'device', got {sampler!r}")
        if weights not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"weights must be 'bf16', 'fp8' or 'mxfp4', got {weights!r}")
        if kv not in ("bf16", "fp8"):
            raise ValueError(f"kv must be 'bf16' or 'fp8', got {kv!r}")
        check_speculative(speculative, ngram, draft, batch, sampler, kv)
        cfg = model.config
        self.model = model
        self.batch = int(batch)
        w = model.lm_head.weight
        self.on_gpu = w.is_cuda
        self.graph = bool(graph)
        self.weights = weights
        self.qweights = None
        projections = list(model.decode_projections())
        if weights == "fp8":
            self.qweights = {name: ops.quantize_fp8(pw) for name, pw in projections}
            projections = list(self.qweights.items())
        elif weights == "mxfp4":
            for name, pw in projections:  # the format's own condition, with or without a graph
                if pw.shape[1] % 32:
                    raise ValueError(f"DecodeSession(weights='mxfp4', graph={self.graph}): {name} {tuple(pw.shape)} "
                                     "needs K % 32 == 0, one block scale per 32 elements of K")
            self.qweights = {name: ops.quantize_mxfp4(pw) for name, pw in projections}
            projections = list(self.qweights.items())
        self.weight_bytes = sum(pw.nbytes for _, pw in projections)
        # what the model's calls get beyond their usual arguments: nothing for a bf16 session
        self._model_kw = {} if self.qweights is None else {"weights": self.qweights}
        self.speculative = None if speculative is None else int(speculative)
        rows = self.batch * (1 + (self.speculative or 0))  # of a step's linear layers
        if self.graph and self.on_gpu:
            if self.batch > MAX_GRAPH_BATCH:
                raise ValueError(f"DecodeSession(graph=True): batch {self.batch} > {MAX_GRAPH_BATCH}, the most "
                                 "rows the skinny linear kernel takes")
            probes = {}  # one input of the step's shape per K
            for name, pw in projections:
                K = pw.shape[1]
                if K not in probes:
                    probes[K] = torch.empty(rows, K, device=w.device, dtype=w.dtype)
                if not ops.linear_decode_eligible(probes[K], pw):
                    kind = {"bf16": (f"{getattr(pw, 'dtype', None)}", "K % 8 == 0"),
                            "fp8": ("fp8 (e4m3, bf16 activations)", "K % 16 == 0"),
                            "mxfp4": ("mxfp4 (e2m1, bf16 activations)", "K % 32 == 0")}[weights]
                    raise ValueError(f"DecodeSession(graph=True): {name} {tuple(pw.shape)} {kind[0]} is not "
                                     f"eligible for ops.linear_decode (bf16 on the HIP backend, {kind[1]}, "
                                     "contiguous weight), and a library GEMM must not be captured")
        self.kv = kv
        self.cache = model.new_cache(self.batch, max_len, kv_dtype=kv)  # at most the model's context limit
        self.cache_bytes = self.cache.nbytes
        self.max_len = self.cache.max_len
        self.tokens = torch.zeros(self.batch, 1, dtype=torch.long, device=w.device)
        self.logits = torch.zeros(self.batch, cfg.vocab_size, dtype=w.dtype, device=w.device)
        self.captures = 0
        self.replays = 0
        self._graph = None
        self.sampler = sampler
        self.rng_seed = self.sample_params = self.history = None
        self._sample_graph = None
        if sampler == "device":
            from ..ops.decode import sample_params
            self.rng_seed = torch.zeros(1, dtype=torch.int64, device=w.device)
            self.sample_params = sample_params(1.0, None, w.device)
            self.history = torch.zeros(self.batch, self.max_len + 1, dtype=torch.long, device=w.device)
        self.ngram = int(ngram)
        self.draft = None
        self.spec_steps = self.spec_emitted = 0
        self._spec_graph = None
        if self.speculative is not None:
            k1 = self.speculative + 1
            if isinstance(draft, torch.Tensor):
                self.draft = draft.to(w.device)
                self._draft_cols = torch.arange(k1, device=w.device).view(1, k1)
            self.spec_tokens = torch.zeros(self.batch, k1, dtype=torch.long, device=w.device)
            self.spec_target = torch.zeros(self.batch, k1, dtype=torch.long, device=w.device)
            self.spec_logits = torch.zeros(self.batch * k1, cfg.vocab_size, dtype=w.dtype, device=w.device)
            self.stop = torch.zeros(self.batch, dtype=torch.int32, device=w.device)

    # ------------------------------------------------------------------ prompt
    @torch.no_grad()
    def prefill(self, idx):
        """The model's ``forward_cached`` on this session's cache: logits (B, vocab) of the last
        position of ``idx`` (B, T); call it again for a chunked prompt.  A speculative session
        also keeps the prompt in ``history``, for the n-gram draft to search."""
        if self.speculative is not None:
            pos = self.cache.pos
            self.history[:, pos:pos + idx.shape[1]] = idx[:, :max(0, self.history.shape[1] - pos)]
        return self.model.forward_cached(idx, self.cache, **self._model_kw)

    def reset(self):
        """Empty the cache for a new prompt; a captured graph stays valid (same buffers)."""
        self.cache.reset()

    # ------------------------------------------------------------------ one token
    def _body(self):
        """One decode step on device state only: advances start / lens, reads ``self.tokens``,
        writes ``self.logits``."""
        cache = self.cache
        cache.start.copy_(cache.lens)
        cache.lens.add_(1)
        self.model.decode_step(self.tokens, cache, self.logits, **self._model_kw)

    def _capture(self, body, restore):
        """``body`` as a graph.  An eager warm-up on a side stream first (lazy initialisations must
        not happen inside a capture), then the tensors ``restore`` that it advanced or overwrote
        put back, then the capture on the current stream.  A capture launches nothing: the
        caller's first replay is its step."""
        saved = [t.clone() for t in restore]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        for t, s in zip(restore, saved):
            t.copy_(s)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            body()
        self.captures += 1
        return g

    @torch.no_grad()
    def step(self, tokens):
        """Append ``tokens`` (B,) or (B, 1) and return the static logits buffer (B, vocab) of the
        next position.  Raises ``ValueError`` before any launch when the cache is full.  The
        capturing call's own replay does not count in ``replays``."""
        cache = self.cache
        cache.check_room(1)
        self.tokens.copy_(tokens.reshape(self.batch, 1))
        if not (self.graph and self.on_gpu):
            self._body()
        elif self._graph is not None:
            self._graph.replay()
            self.replays += 1
        else:
            self._graph = self._capture(self._body, (cache.lens, cache.start))
            self._graph.replay()
        cache.pos += 1
        return self.logits

    # ------------------------------------------------------------------ sampling loop
    @torch.no_grad()
    def generate(self, idx, n, temperature=1.0, top_k=None):
        """Prefill ``idx`` (B, T) and sample ``n`` tokens (T + n - 1 <= max_len): (B, T + n).
        With the default sampler, sampling stays outside the captured step, on the static logits,
        and the new tokens go into a preallocated output; ``sampler="device"`` is
        :meth:`_generate_device`."""
        if self.speculative is not None:
            return self._generate_speculative(idx, n, temperature, top_k)
        if self.sampler == "device":
            return self._generate_device(idx, n, temperature, top_k)
        B, T = idx.shape
        out = torch.empty(B, T + n, dtype=idx.dtype, device=idx.device)
        out[:, :T] = idx
        logits = self.prefill(idx)
        for i in range(n):
            nxt = generation.sample_logits(logits, temperature, top_k)
            out[:, T + i:T + i + 1] = nxt
            if i + 1 < n:
                logits = self.step(nxt)
        return out

    # ------------------------------------------------------------------ sampling on the device
    def _sample(self, logits):
        """``ops.sample_tokens`` on device state only: the token of every row of ``logits`` at
        position ``cache.lens`` goes into ``self.tokens`` and into ``self.history`` at that column."""
        ops.sample_tokens(logits, params=self.sample_params, seed=self.rng_seed, positions=self.cache.lens,
                          out=self.tokens, history=self.history)

    def _body_sample(self):
        self._body()
        self._sample(self.logits)

    def _step_sample(self):
        """One decode step on ``self.tokens`` and the draw of the next token into it.  With
        ``graph=True`` the pair is one captured linear chain; every replay, the capturing call's
        included, counts in ``replays``."""
        cache = self.cache
        cache.check_room(1)
        if not (self.graph and self.on_gpu):
            self._body_sample()
        else:
            if self._sample_graph is None:
                # the history column the warm-up wrote is the one the first replay writes again
                self._sample_graph = self._capture(self._body_sample, (cache.lens, cache.start, self.tokens))
            self._sample_graph.replay()
            self.replays += 1
        cache.pos += 1

    def _generate_device(self, idx, n, temperature, top_k):
        """:meth:`generate` with every draw on the device.  A fresh 64-bit seed from torch's
        default CPU generator (so ``torch.manual_seed`` governs the tokens) and the sampling
        parameters are written to the device, the prompt is prefilled and the first token drawn
        from its logits; the other n - 1 tokens are n - 1 runs of [step, draw] -- replays of one
        graph with ``graph=True``, with no torch op and no host synchronisation between them.
        Row b's token at sequence position p uses the uniform of Philox counter (p, b, 0, 0); the
        tokens are copied out of ``history`` once at the end."""
        from ..ops.decode import sample_params
        B, T = idx.shape
        p0 = self.cache.pos + T  # the first new token's position (a chunked prompt may precede idx)
        if n < 1:
            return idx.clone()
        self.cache.check_room(T + n - 1)  # before the generator or any session state is touched
        seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64)
        self.rng_seed.copy_(seed)
        sample_params(temperature, top_k, out=self.sample_params)
        logits = self.prefill(idx)
        self._sample(logits)
        for _ in range(n - 1):
            self._step_sample()
        return torch.cat((idx, self.history[:, p0:p0 + n].to(idx.dtype)), dim=1)

    # ------------------------------------------------------------------ speculative decoding
    def _spec_body(self):
        """One verify step on device state only: start <- lens, lens += k + 1, the current token
        and the k guesses into ``spec_tokens``, the forward over them, the draw of the target token
        at every position (the counter of position start + 1 + t), and the accept rule, which
        writes the emitted tokens into ``history`` and the rows' new lengths into ``cache.lens``."""
        cache, k1 = self.cache, self.speculative + 1
        cache.start.copy_(cache.lens)
        cache.lens.add_(k1)
        if self.draft is None:
            ops.spec_draft(self.history, cache.start, self.spec_tokens, self.ngram)
        else:
            cols = cache.start.view(-1, 1).long() + self._draft_cols
            self.spec_tokens.copy_(self.draft.gather(1, cols.clamp(0, self.draft.shape[1] - 1)))
            self.spec_tokens[:, :1] = self.history.gather(1, cols[:, :1].clamp(0, self.history.shape[1] - 1))
        self.model.decode_step(self.spec_tokens, cache, self.spec_logits, **self._model_kw)
        ops.sample_tokens(self.spec_logits, params=self.sample_params, seed=self.rng_seed, positions=cache.start,
                          out=self.spec_target.view(-1), rows_per_seq=k1, position_offset=1)
        ops.spec_accept(self.spec_tokens, self.spec_target, cache.start, cache.lens, self.stop, self.history)

    def _step_speculative(self):
        """One verify step (a replay of its one graph with ``graph=True``; every replay counts in
        ``replays``), then the step's one synchronisation: the rows' lengths come back to the host.
        Returns them."""
        cache = self.cache
        if not (self.graph and self.on_gpu):
            self._spec_body()
        else:
            if self._spec_graph is None:
                # the warm-up's appends land where the first replay's land; the rest is put back
                self._spec_graph = self._capture(self._spec_body, (cache.lens, cache.start, self.spec_tokens,
                                                                   self.spec_target, self.history))
            self._spec_graph.replay()
            self.replays += 1
        lens = cache.lens.tolist()
        self.spec_steps += 1
        return lens

    def _generate_speculative(self, idx, n, temperature, top_k):
        """:meth:`_generate_device` with up to k + 1 tokens per step.  The seed, the sampling
        parameters, the prefill and the first token are that method's; every later token comes
        from verify steps until each row has reached ``stop[b]`` = the column of its n-th token
        (a row that is done emits nothing more).  The tokens are those of the plain loop."""
        from ..ops.decode import sample_params
        B, T = idx.shape
        p0 = self.cache.pos + T
        if n < 1:
            return idx.clone()
        self.cache.check_room(T + n - 1)
        seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64)
        self.rng_seed.copy_(seed)
        sample_params(temperature, top_k, out=self.sample_params)
        logits = self.prefill(idx)
        self._sample(logits)
        last = p0 + n - 1
        self.stop.fill_(last)
        lens = [p0] * B
        while min(lens) < last:
            new = self._step_speculative()
            emitted = sum(new) - sum(lens)
            if emitted <= 0:
                raise RuntimeError(f"speculative step emitted no token (lengths {lens} -> {new})")
            self.spec_emitted += emitted
            lens = new
            self.cache.pos = max(lens)
        return torch.cat((idx, self.history[:, p0:p0 + n].to(idx.dtype)), dim=1)

"""The fused decode step on the CPU: ``ops.linear_decode`` against the composition of the existing
reference ops, :class:`DecodeSession` teacher-forced against the uncached forward, and the
``generate(use_cache="fused" / "graph")`` surface.  On the CPU every path is the fp32 reference
ops, so the bound is the one of tests/test_decode_cpu.py: fp32 eps x the longest reduction
(<= 1,024 terms) = 1e-4."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from tolerance import rel_err

B, PROMPT, STEPS = 2, 19, 9
BOUND = 1e-4
M, N, K = 3, 41, 72

NORMS = [None, "layer", "layer-nobeta", "rms"]
EPIS = ["none", "bias", "bias-gelu", "residual", "bias-residual", "swiglu"]


def _model(name, **kw):
    torch.manual_seed(0)
    m = build_gpt2("gpt2-tiny", **kw) if name == "gpt2-tiny" else build_llama("llama-tiny", **kw)
    return m.eval()


def linear_decode_case(norm, epi, m=M, n=N, k=K, seed=0, device="cpu", dtype=torch.float32):
    """(kwargs of ops.linear_decode, the same function composed from existing reference ops)."""
    g = torch.Generator().manual_seed(seed)

    def r(*s):
        return torch.randn(*s, generator=g).to(dtype).to(device)

    swiglu = epi == "swiglu"
    rows = 2 * n if swiglu else n
    x, w = r(m, k), r(rows, k) * k ** -0.5
    kw = dict(x=x, weight=w)
    if norm is not None:
        kw.update(norm=norm.split("-")[0], norm_weight=1 + 0.1 * r(k), eps=1e-5)
        if norm == "layer":
            kw["norm_bias"] = 0.1 * r(k)
    if "bias" in epi:
        kw["bias"] = r(rows)
    if "gelu" in epi:
        kw["act"] = "gelu"
    if swiglu:
        kw["act"] = "swiglu"
    if "residual" in epi:
        kw["residual"] = r(m, n)

    def composed(kw, lin=F.linear):
        h = kw["x"]
        if kw.get("norm") == "layer":
            h = ref.layer_norm(h, kw["norm_weight"], kw.get("norm_bias"), kw["eps"])
        elif kw.get("norm") == "rms":
            h = ref.rms_norm(h, kw["norm_weight"], kw["eps"])
        y = lin(h, kw["weight"], kw.get("bias"))
        if kw.get("act") == "gelu":
            y = ref.gelu_tanh(y)
        elif kw.get("act") == "swiglu":
            y = ref.swiglu(*y.chunk(2, dim=-1))
        return y if kw.get("residual") is None else y + kw["residual"]

    return kw, composed


def call(kw):
    kw = dict(kw)
    return ops.linear_decode(kw.pop("x"), kw.pop("weight"), kw.pop("bias", None), **kw)


@pytest.mark.parametrize("norm,epi", list(itertools.product(NORMS, EPIS)))
def test_linear_decode_equals_the_composed_reference_ops(norm, epi):
    kw, composed = linear_decode_case(norm, epi)
    y = call(kw)
    want = composed(kw)
    assert y.shape == (M, N) and y.dtype == torch.float32
    assert rel_err(y, want) <= BOUND
    # leading dimensions are kept: (M, 1, K) -> (M, 1, N)
    kw3 = dict(kw, x=kw["x"][:, None], residual=None if kw.get("residual") is None else kw["residual"][:, None])
    assert torch.equal(call(kw3), y[:, None])


def test_linear_decode_surface():
    assert "linear_decode" in ops.__all__ and "linear_decode_eligible" in ops.__all__
    kw, _ = linear_decode_case("rms", "bias")
    assert not ops.linear_decode_eligible(kw["x"], kw["weight"])  # a CPU tensor takes the reference
    out = torch.empty(M, N)
    assert torch.equal(call(dict(kw, out=out)), call(kw)) and torch.equal(out, call(kw))
    with pytest.raises(RuntimeError, match="inference-only"):
        call(dict(kw, x=kw["x"].clone().requires_grad_()))
    with torch.no_grad():
        call(dict(kw, x=kw["x"].clone().requires_grad_()))
    with pytest.raises(AssertionError):
        call(dict(kw, act="relu"))


@pytest.fixture(scope="module", params=["gpt2-tiny", "llama-tiny"])
def teacher(request):
    """(model, tokens, uncached last-position logits of every prefix length), computed once."""
    model = _model(request.param)
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, model.config.vocab_size, (B, PROMPT + STEPS), generator=g)
    with torch.no_grad():
        want = {n: model(toks[:, :n])[0][:, -1] for n in range(PROMPT, PROMPT + STEPS + 1)}
    return model, toks, want


@pytest.mark.parametrize("chunks", [(PROMPT,), (11, 8)], ids=["prefill", "chunked-prefill"])
def test_session_teacher_forced_logits_match_uncached(teacher, chunks):
    model, toks, want = teacher
    eager = DecodeSession(model, B, PROMPT + STEPS)
    graph = model.decode_session(B, PROMPT + STEPS, graph=True)  # nothing to capture on the CPU
    for s in (eager, graph):
        at = 0
        for n in chunks:
            logits = s.prefill(toks[:, at:at + n])
            at += n
        assert s.cache.pos == PROMPT and s.cache.lens.tolist() == [PROMPT] * B
        assert rel_err(logits, want[PROMPT]) <= BOUND
    worst = 0.0
    for step in range(STEPS):
        n = PROMPT + step
        logits = eager.step(toks[:, n:n + 1])
        assert logits.shape == (B, model.config.vocab_size) and logits is eager.logits
        e = rel_err(logits, want[n + 1])
        worst = max(worst, e)
        assert e <= BOUND, f"step {step}: {e:.3e}"
        assert torch.equal(graph.step(toks[:, n]), logits)  # (B,) tokens are taken too
        assert eager.cache.pos == n + 1 and eager.cache.lens.tolist() == [n + 1] * B
        assert eager.cache.start.tolist() == [n] * B
    assert graph.captures == 0 and graph.replays == 0 and graph.cache.pos == PROMPT + STEPS
    print(f"max rel err fused step vs uncached: {worst:.3e}")
    eager.reset()
    assert eager.cache.pos == 0 and eager.cache.lens.tolist() == [0] * B
    assert rel_err(eager.prefill(toks[:, :PROMPT]), want[PROMPT]) <= BOUND


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_fused_and_graph_surface(name):
    model = _model(name)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, model.config.vocab_size, (B, 7), generator=g)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(11)
        out = outs[mode] = model.generate(prompt, 6, temperature=0.9, top_k=20, use_cache=mode)
        assert out.shape == (B, 7 + 6) and out.dtype == prompt.dtype
        assert torch.equal(out[:, :7], prompt)
        assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size
        assert model.generate(prompt, 0, use_cache=mode).shape == (B, 7)
    assert torch.equal(outs["fused"], outs["graph"])
    with pytest.raises(ValueError, match="use_cache"):
        model.generate(prompt, 2, use_cache="paged")


@pytest.mark.parametrize("mode", ["fused", "graph"])
@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_fused_crosses_the_context_limit(name, mode):
    """block 32, prompt 30, 8 new tokens: three come from the session, the rest from the uncached
    sliding-window loop."""
    model = _model(name, **({"block_size": 32} if name == "gpt2-tiny" else {"max_seq_len": 32}))
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, model.config.vocab_size, (B, 30), generator=g)
    out = model.generate(prompt, 8, use_cache=mode)
    assert out.shape == (B, 38) and torch.equal(out[:, :30], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_true_and_false_keep_their_random_stream(name):
    """use_cache=True / False under a fixed seed against hand-rolled loops over ``forward_cached``
    / the plain forward that draw from the same stream."""
    model = _model(name)
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, model.config.vocab_size, (B, 5), generator=g)
    new, temp, top_k = 6, 0.8, 10

    def draw(logits):
        logits = logits.float() / temp
        v, _ = torch.topk(logits, top_k)
        logits[logits < v[:, [-1]]] = -float("inf")
        return torch.multinomial(torch.softmax(logits, -1), 1)

    torch.manual_seed(7)
    got_cached = model.generate(prompt, new, temperature=temp, top_k=top_k, use_cache=True)
    torch.manual_seed(7)
    with torch.no_grad():
        cache = model.new_cache(B, 5 + new - 1)
        idx, logits = prompt, model.forward_cached(prompt, cache)
        for i in range(new):
            nxt = draw(logits)
            idx = torch.cat((idx, nxt), 1)
            if i + 1 < new:
                logits = model.forward_cached(nxt, cache)
    assert torch.equal(got_cached, idx)

    torch.manual_seed(7)
    got_plain = model.generate(prompt, new, temperature=temp, top_k=top_k)
    torch.manual_seed(7)
    with torch.no_grad():
        idx = prompt
        for _ in range(new):
            idx = torch.cat((idx, draw(model(idx)[0][:, -1, :])), 1)
    assert torch.equal(got_plain, idx)


def _draw(logits, temp, top_k):
    """The sampling rule, written out here: the tests below pin ``generate`` against it."""
    logits = logits.float() / temp
    v, _ = torch.topk(logits, top_k)
    logits[logits < v[:, [-1]]] = -float("inf")
    return torch.multinomial(torch.softmax(logits, -1), 1)


def _hand_rolled(model, prompt, new, mode, temp, top_k, limit=None):
    """``new`` tokens after ``prompt``: the first n from ``forward_cached`` (mode True) or a
    :class:`DecodeSession` (``"fused"`` / ``"graph"``), the rest from the plain forward on the
    last ``limit`` tokens.  Without a limit every token is a cached one."""
    T = prompt.size(1)
    n = new if limit is None else min(new, limit - T + 1) if T < limit else 0
    idx = prompt
    with torch.no_grad():
        if n > 0:
            if mode is True:
                cache = model.new_cache(B, T + n - 1)
                first, step = model.forward_cached(prompt, cache), lambda tok: model.forward_cached(tok, cache)
            else:
                sess = model.decode_session(B, T + n - 1, graph=mode == "graph")
                first, step = sess.prefill(prompt), sess.step
            logits = first
            for i in range(n):
                nxt = _draw(logits, temp, top_k)
                idx = torch.cat((idx, nxt), 1)
                if i + 1 < n:
                    logits = step(nxt)
        for _ in range(new - n):
            idx = torch.cat((idx, _draw(model(idx[:, -limit:])[0][:, -1, :], temp, top_k)), 1)
    return idx


@pytest.mark.parametrize("mode", ["fused", "graph"])
@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_fused_and_graph_keep_their_random_stream(name, mode):
    """As the test above for use_cache="fused" / "graph" with the default sampler: a hand-rolled
    loop over ``decode_session(...).prefill`` / ``.step`` under the same seed, token for token."""
    model = _model(name)
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, model.config.vocab_size, (B, 5), generator=g)
    torch.manual_seed(7)
    got = model.generate(prompt, 6, temperature=0.8, top_k=10, use_cache=mode)
    torch.manual_seed(7)
    assert torch.equal(got, _hand_rolled(model, prompt, 6, mode, 0.8, 10))


@pytest.mark.parametrize("plen,new", [(30, 8), (32, 3), (31, 1)],
                         ids=["3-cached-5-window", "window-only", "1-cached"])
@pytest.mark.parametrize("mode", [True, "fused", "graph"])
@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_hands_over_at_the_context_limit(name, mode, plen, new):
    """Context limit 32: ``n = min(new, 32 - T + 1)`` tokens come from the cache or the session (a
    prompt that fills the window has none), the rest from ``model(idx[:, -32:])``; exact under
    the same seed."""
    model = _model(name, **({"block_size": 32} if name == "gpt2-tiny" else {"max_seq_len": 32}))
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, model.config.vocab_size, (B, plen), generator=g)
    torch.manual_seed(7)
    got = model.generate(prompt, new, temperature=0.8, top_k=10, use_cache=mode)
    torch.manual_seed(7)
    want = _hand_rolled(model, prompt, new, mode, 0.8, 10, limit=32)
    assert got.shape == (B, plen + new) and torch.equal(got, want)


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_every_torch_sampler_mode_draws_through_sample_logits(name, monkeypatch):
    """One rule: ``generate`` of the model in its four torch-sampler modes and
    ``DecodeSession.generate`` call ``generation.sample_logits`` once per new token."""
    from orion_amd.models import generation
    calls = []
    rule = generation.sample_logits

    def counting(logits, temperature=1.0, top_k=None):
        calls.append((tuple(logits.shape), temperature, top_k))
        return rule(logits, temperature, top_k)

    monkeypatch.setattr(generation, "sample_logits", counting)
    model = _model(name)
    prompt = torch.zeros(B, 5, dtype=torch.long)
    V = model.config.vocab_size
    for mode in (False, True, "fused", "graph"):
        del calls[:]
        model.generate(prompt, 6, temperature=0.8, top_k=10, use_cache=mode)
        assert calls == [((B, V), 0.8, 10)] * 6, mode
    del calls[:]
    model.decode_session(B, 16).generate(prompt, 4, 0.7, 3)
    assert calls == [((B, V), 0.7, 3)] * 4


@pytest.mark.parametrize("graph", [False, True])
def test_step_raises_before_overflow(graph):
    model = _model("gpt2-tiny")
    s = DecodeSession(model, 1, 4, graph=graph)
    s.prefill(torch.zeros(1, 3, dtype=torch.long))
    s.step(torch.ones(1, 1, dtype=torch.long))
    buf, tok = s.cache.buf.clone(), s.tokens.clone()
    with pytest.raises(ValueError, match="overflow"):
        s.step(torch.full((1, 1), 2, dtype=torch.long))
    assert s.cache.pos == 4 and s.cache.lens.tolist() == [4] and s.cache.start.tolist() == [3]
    assert torch.equal(s.cache.buf, buf) and torch.equal(s.tokens, tok)
    with pytest.raises(ValueError, match="overflow"):
        s.prefill(torch.zeros(1, 1, dtype=torch.long))

"""KV-cache generation on the CPU: ``forward_cached`` against the uncached forward, the
``generate(use_cache=True)`` surface, ``ref.kv_append`` / ``ref.attention_decode`` and
``KVCache``.  On the CPU both paths are the fp32 reference ops and differ only in summation
order, so a logic error (a shifted position, a dropped key) shows at >= 1e-2 while the bound
is fp32 eps x the longest reduction (<= 1,024 terms) = 1e-4."""
import pytest
import torch

from orion_amd import ops
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.kv_cache import KVCache
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from tolerance import rel_err

B, PROMPT, STEPS = 2, 19, 9
BOUND = 1e-4


def _model(name):
    torch.manual_seed(0)
    m = build_gpt2("gpt2-tiny") if name == "gpt2-tiny" else build_llama("llama-tiny")
    return m.eval()


@pytest.fixture(scope="module", params=["gpt2-tiny", "llama-tiny"])
def teacher(request):
    """(model, tokens, uncached last-position logits of every prefix length PROMPT .. PROMPT + STEPS),
    computed once and shared by the two prefill forms."""
    model = _model(request.param)
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, model.config.vocab_size, (B, PROMPT + STEPS), generator=g)
    with torch.no_grad():
        want = {n: model(toks[:, :n])[0][:, -1] for n in range(PROMPT, PROMPT + STEPS + 1)}
    return model, toks, want


@pytest.mark.parametrize("chunks", [(PROMPT,), (11, 8)], ids=["prefill", "chunked-prefill"])
def test_teacher_forced_cached_logits_match_uncached(teacher, chunks):
    """Measured maximum over every step: 4.3e-7 / 4.4e-7 (gpt2-tiny, one / two prefill chunks),
    4.1e-7 / 4.2e-7 (llama-tiny) -- fp32 rounding; a value above 1e-5 deserves a look."""
    model, toks, want = teacher
    cache = model.new_cache(B, PROMPT + STEPS)
    at = 0
    for n in chunks:
        logits = model.forward_cached(toks[:, at:at + n], cache)
        at += n
    assert at == PROMPT and cache.pos == PROMPT and cache.lens.tolist() == [PROMPT] * B
    worst = rel_err(logits, want[PROMPT])
    assert logits.shape == (B, model.config.vocab_size)
    assert worst <= BOUND, f"prefill: {worst:.3e}"
    for step in range(STEPS):
        n = PROMPT + step
        logits = model.forward_cached(toks[:, n:n + 1], cache)
        e = rel_err(logits, want[n + 1])
        worst = max(worst, e)
        assert e <= BOUND, f"step {step}: {e:.3e}"
    assert cache.pos == PROMPT + STEPS
    print(f"max rel err cached vs uncached: {worst:.3e}")


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_with_cache_surface(name):
    model = _model(name)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, model.config.vocab_size, (B, 7), generator=g)
    out = model.generate(prompt, 6, temperature=0.9, top_k=20, use_cache=True)
    assert out.shape == (B, 7 + 6)
    assert torch.equal(out[:, :7], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size
    assert model.generate(prompt, 0, use_cache=True).shape == (B, 7)


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_with_cache_crosses_the_context_limit(name):
    """block_size 32, prompt 30, 8 new tokens: three come from the cache, the rest from the
    uncached sliding-window loop."""
    torch.manual_seed(0)
    model = (build_gpt2("gpt2-tiny", block_size=32) if name == "gpt2-tiny"
             else build_llama("llama-tiny", max_seq_len=32)).eval()
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, model.config.vocab_size, (B, 30), generator=g)
    out = model.generate(prompt, 8, use_cache=True)
    assert out.shape == (B, 38)
    assert torch.equal(out[:, :30], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size


def test_generate_default_is_uncached():
    """use_cache defaults to False: same seed, same tokens as the plain loop."""
    model = _model("gpt2-tiny")
    prompt = torch.zeros(1, 4, dtype=torch.long)
    torch.manual_seed(5)
    a = model.generate(prompt, 5)
    torch.manual_seed(5)
    b = model.generate(prompt, 5, use_cache=False)
    assert torch.equal(a, b)


@pytest.mark.parametrize("with_rope", [False, True])
def test_ref_kv_append_writes_only_its_rows(with_rope):
    Bn, T, Hq, Hkv, D, Tmax = 3, 5, 4, 2, 16, 12
    g = torch.Generator().manual_seed(4)
    k_new, v_new = torch.randn(Bn, T, Hkv, D, generator=g), torch.randn(Bn, T, Hkv, D, generator=g)
    q = torch.randn(Bn, T, Hq, D, generator=g)
    lens = torch.tensor([0, 4, 9], dtype=torch.int32)  # the last row: 9 + 5 > 12, three tokens fit
    kc, vc = torch.full((Bn, Tmax, Hkv, D), 7.0), torch.full((Bn, Tmax, Hkv, D), 7.0)
    cos, sin = ref.rope_tables(Tmax, D)
    q_rot = ops.kv_append(k_new, v_new, kc, vc, lens, **(dict(q=q, cos=cos, sin=sin) if with_rope else {}))
    assert lens.tolist() == [0, 4, 9]
    for b, p0 in enumerate(lens.tolist()):
        n = min(T, Tmax - p0)
        written = torch.zeros(Tmax, dtype=torch.bool)
        written[p0:p0 + n] = True
        assert torch.all(kc[b, ~written] == 7.0) and torch.all(vc[b, ~written] == 7.0)
        assert torch.equal(vc[b, p0:p0 + n], v_new[b, :n])
        want_k = ref.rope(k_new[b:b + 1, :n], cos[p0:], sin[p0:])[0] if with_rope else k_new[b, :n]
        assert torch.equal(kc[b, p0:p0 + n], want_k)
        if with_rope:
            assert torch.equal(q_rot[b, :n], ref.rope(q[b:b + 1, :n], cos[p0:], sin[p0:])[0])
            assert torch.all(q_rot[b, n:] == 0)
    if not with_rope:
        assert q_rot is None


def test_ref_attention_decode_masks_by_length():
    Bn, Hq, Hkv, D, Tmax = 4, 4, 2, 16, 10
    g = torch.Generator().manual_seed(6)
    q = torch.randn(Bn, Hq, D, generator=g)
    kc, vc = torch.randn(Bn, Tmax, Hkv, D, generator=g), torch.randn(Bn, Tmax, Hkv, D, generator=g)
    lens = torch.tensor([0, 1, 6, 99], dtype=torch.int32)
    for b, n in enumerate([0, 1, 6, Tmax]):  # stale positions hold NaN
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    o = ops.attention_decode(q, kc, vc, lens)
    assert torch.isfinite(o).all() and torch.all(o[0] == 0)
    torch.testing.assert_close(o[1], vc[1, 0].repeat_interleave(2, 0))  # one key: its value
    for b, n in [(2, 6), (3, Tmax)]:
        want = ref.attention(q[b:b + 1, None], kc[b:b + 1, :n], vc[b:b + 1, :n], causal=True)[0, 0]
        torch.testing.assert_close(o[b], want, rtol=1e-5, atol=1e-6)


def test_decode_ops_refuse_inputs_that_require_grad():
    from orion_amd.ops.decode import _no_grad
    x = torch.zeros(2, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        _no_grad(x)
    with torch.no_grad():
        _no_grad(x)
    assert "attention_decode" in ops.__all__ and "kv_append" in ops.__all__


def test_kv_cache_raises_before_overflow():
    cache = KVCache(2, 3, 8, 2, 16, dtype=torch.float32)
    assert cache.buf.shape == (2, 2, 3, 8, 2, 16) and cache.lens.dtype == torch.int32
    assert cache.begin(5) == 0 and cache.start.tolist() == [0] * 3 and cache.lens.tolist() == [5] * 3
    with pytest.raises(ValueError, match="overflow"):
        cache.begin(4)
    assert cache.pos == 5 and cache.lens.tolist() == [5] * 3  # untouched by the refused call
    assert cache.begin(3) == 5 and cache.start.tolist() == [5] * 3 and cache.lens.tolist() == [8] * 3
    with pytest.raises(ValueError, match="overflow"):
        cache.begin(1)
    model = _model("gpt2-tiny")
    small = model.new_cache(1, 4)
    with pytest.raises(ValueError, match="overflow"):
        model.forward_cached(torch.zeros(1, 5, dtype=torch.long), small)
    assert torch.all(small.buf == 0)

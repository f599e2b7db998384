"""Speculative decoding without a GPU: the draft and accept references on hand-worked cases, the
sampling reference with several rows per sequence, and the session on the CPU reference path.

The session tests sample greedily (top_k = 1): a CPU matmul's rounding may depend on the number of
rows, and then only an argmax near-tie could differ between a verify step and a plain step.  The
seeds below show none."""
import math

import pytest
import torch

from orion_amd import ops
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from spec_fixtures import K, PATTERNS, accept_case, corrupt, draft_cases, predicted_steps

PROMPT, N = 9, 24
MODELS = {"gpt2-tiny": build_gpt2, "llama-tiny": build_llama}
_models = {}


def _model(name):
    if name not in _models:
        torch.manual_seed(0)
        _models[name] = MODELS[name](name).eval()
    return _models[name]


_plain = {}


def _reference_tokens(name, B):
    """The plain loop's tokens (computed once per model and batch, never modified)."""
    if (name, B) not in _plain:
        m = _model(name)
        idx = torch.randint(0, m.config.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(B))
        torch.manual_seed(5)
        _plain[name, B] = (idx, m.generate(idx, N, 0.8, 1, use_cache="graph", sampler="device"))
    return _plain[name, B]


@pytest.mark.parametrize("name", sorted(draft_cases()))
def test_draft_reference_on_hand_cases(name):
    history, cur, g, want = draft_cases()[name]
    out = torch.full((history.shape[0], K + 1), -1, dtype=torch.int64)
    before = history.clone()
    assert ops.spec_draft(history, cur, out, g) is out
    assert torch.equal(out, want)
    assert torch.equal(history, before)


def test_accept_reference_on_hand_cases():
    tokens, target, start, stop, L, want_e, want_hist = accept_case()
    history = torch.full((tokens.shape[0], L), -1, dtype=torch.int64)
    lens = start + 4  # what the step left there
    assert ref.spec_accept(tokens, target, start, lens, stop, history) == want_e
    assert torch.equal(history, want_hist)
    assert lens.tolist() == [int(s) + e for s, e in zip(start, want_e)]
    history.fill_(-1)
    lens = start + 4
    ops.spec_accept(tokens, target, start, lens, stop, history)  # the op on CPU tensors is the reference
    assert torch.equal(history, want_hist) and lens.tolist() == [int(s) + e for s, e in zip(start, want_e)]


def test_sample_reference_with_rows_per_seq():
    B, R, V = 3, 4, 300
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B * R, V, generator=g).to(torch.bfloat16)
    pos = torch.tensor([5, 0, 17], dtype=torch.int32)
    got = ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, rows_per_seq=R, position_offset=1)
    assert got.shape == (B * R, 1)
    for t in range(R):  # row b R + t is sequence b at position pos[b] + 1 + t
        want = ops.sample_tokens(logits[t::R], 0.8, 40, seed=99, positions=pos + 1 + t)
        assert torch.equal(got[t::R], want), t
    u = ref.philox_uniform(99, pos, R, 1)
    for b in range(B):
        for t in range(R):
            one = torch.zeros(b + 1, dtype=torch.int32)
            one[b] = int(pos[b]) + 1 + t
            assert u[b * R + t] == ref.philox_uniform(99, one)[b]
    # the defaults are the one-row-per-sequence op
    assert torch.equal(ops.sample_tokens(logits[:B], 0.8, 40, seed=99, positions=pos, rows_per_seq=1),
                       ops.sample_tokens(logits[:B], 0.8, 40, seed=99, positions=pos))
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, rows_per_seq=R,
                          history=torch.zeros(B * R, 8, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, 0.8, 40, seed=99, positions=pos, rows_per_seq=5)


def test_attention_decode_multi_reference_is_the_single_query_reference_per_query():
    B, Tq, Hq, Hkv, D, Tmax = 2, 5, 4, 2, 64, 40
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B, Tq, Hq, D, generator=g)
    kc, vc = torch.randn(B, Tmax, Hkv, D, generator=g), torch.randn(B, Tmax, Hkv, D, generator=g)
    for lens in ([5, 2], [23, 45], [40, 7]):
        kv = torch.tensor(lens, dtype=torch.int32)
        o = ops.attention_decode_multi(q, kc, vc, kv)
        for t in range(Tq):
            want = ref.attention_decode(q[:, t], kc, vc, kv - (Tq - 1 - t))
            assert torch.allclose(o[:, t], want, atol=1e-6, rtol=1e-6), (lens, t)
    assert bool((ops.attention_decode_multi(q, kc, vc, torch.tensor([2, 2], dtype=torch.int32))[:, :3] == 0).all())
    with pytest.raises(ValueError):
        ops.attention_decode_multi(q, kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), kv)


@pytest.mark.parametrize("use_cache", ["fused", "graph"])
@pytest.mark.parametrize("B,k", [(1, 1), (1, 7), (2, 3), (2, 7)])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_speculative_tokens_equal_the_plain_loop(name, B, k, use_cache):
    m = _model(name)
    idx, want = _reference_tokens(name, B)
    torch.manual_seed(5)
    got = m.generate(idx, N, 0.8, 1, use_cache=use_cache, sampler="device", speculative=k)
    assert torch.equal(got, want)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_forced_acceptance_patterns(name, pattern):
    B, k = 2, 3
    m = _model(name)
    idx, want = _reference_tokens(name, B)
    draft = corrupt(want, pattern, m.config.vocab_size)
    sess = m.decode_session(B, PROMPT + N - 1, sampler="device", speculative=k, draft=draft)
    torch.manual_seed(5)
    got = sess.generate(idx, N, 0.8, 1)
    assert torch.equal(got, want)
    steps, emitted = predicted_steps(want, draft, PROMPT, N, k)
    assert (sess.spec_steps, sess.spec_emitted) == (steps, emitted)
    assert emitted == B * (N - 1)
    if pattern == "none":
        assert steps == math.ceil((N - 1) / (k + 1))
    if pattern == "all":
        assert steps == N - 1


def test_refusals():
    m = _model("gpt2-tiny")
    idx = torch.zeros(1, 4, dtype=torch.long)
    for kw in (dict(sampler="torch", use_cache="fused"), dict(sampler="device", use_cache=True),
               dict(sampler="device", use_cache="fused", kv="fp8"),
               dict(sampler="device", use_cache="fused", speculative=0),
               dict(sampler="device", use_cache="fused", speculative=16),
               dict(sampler="device", use_cache="fused", draft="model"),
               dict(sampler="device", use_cache="fused", ngram=0)):
        kw.setdefault("speculative", 3)
        with pytest.raises(ValueError):
            m.generate(idx, 4, **kw)
    with pytest.raises(ValueError):
        m.decode_session(3, 16, sampler="device", speculative=5)  # 3 x 6 rows


def test_sample_script_forwards_speculative(monkeypatch, capsys):
    """``sample.py --speculative=K --ngram=G`` reaches ``generate(speculative=K, ngram=G)`` and prints
    the tokens of the run without it."""
    import sample
    from orion_amd.train import ckpt
    model = _model("gpt2-tiny")
    seen = []
    generate = model.generate

    def spy(*args, **kw):
        seen.append(kw)
        return generate(*args, **kw)

    monkeypatch.setattr(model, "generate", spy, raising=False)
    monkeypatch.setattr(ckpt, "load_checkpoint", lambda path: {})
    monkeypatch.setattr(ckpt, "build_model_from_checkpoint", lambda ck: model)
    argv = ["--device=cpu", "--num_samples=1", "--max_new_tokens=12", "--start=ids:1,2,1,2", "--kv_cache=graph",
            "--sampler=device", "--top_k=1"]
    sample.main(argv + ["--speculative=4", "--ngram=2"])
    sample.main(argv)
    assert [(kw["speculative"], kw["ngram"]) for kw in seen] == [(4, 2), (None, 3)]
    a, b = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[1, 2, 1, 2,")]
    assert a == b
    with pytest.raises(ValueError, match="sampler must be 'device'"):
        sample.main(argv[:-2] + ["--speculative=4"])

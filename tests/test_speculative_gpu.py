"""Speculative decoding on the GPU: the tokens equal those of
``generate(use_cache="graph", sampler="device")`` under the same ``torch.manual_seed``, exactly,
for n-gram drafts, forced acceptance patterns, at the context limit and on FP8 weights; the step
is one captured graph; the settings that cannot work are refused before any launch."""
import copy
import math

import pytest
import torch

from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from spec_fixtures import PATTERNS, corrupt, predicted_steps

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPT, N = 9, 24
TEMP, TOP_K = 0.8, 40
BUILD = {"gpt2-tiny": build_gpt2, "llama-tiny": build_llama}  # D 64: MHA, and 4 query heads on 2 KV heads + RoPE
LIMIT_KW = {"gpt2-tiny": "block_size", "llama-tiny": "max_seq_len"}

_models = {}


def _model(name, limit=None):
    if (name, limit) not in _models:
        torch.manual_seed(0)
        m = BUILD[name](name, **({} if limit is None else {LIMIT_KW[name]: limit}))
        m = copy.deepcopy(m).to(DEV).to(torch.bfloat16)
        for bname, buf in m.named_buffers():
            if bname.startswith("rope_"):
                buf.data = buf.data.float()
        _models[name, limit] = m.eval()
    return _models[name, limit]


def _prompt(m, B):
    """A prompt with a repeated stretch, so that the n-gram draft finds matches."""
    g = torch.Generator().manual_seed(B)
    p = torch.randint(0, m.config.vocab_size, (B, PROMPT), generator=g)
    p[:, 5:8] = p[:, 1:4]
    return p.to(DEV)


_plain = {}


def _reference(name, B, n=N, limit=None, **kw):
    """(prompt, the plain loop's tokens), computed once per setting and never modified."""
    key = (name, B, n, limit, tuple(sorted(kw.items())))
    if key not in _plain:
        m = _model(name, limit)
        idx = _prompt(m, B)
        torch.manual_seed(5)
        _plain[key] = (idx, m.generate(idx, n, TEMP, TOP_K, use_cache="graph", sampler="device", **kw))
    return _plain[key]


@pytest.mark.parametrize("use_cache", ["fused", "graph"])
@pytest.mark.parametrize("B,k", [(1, 1), (1, 7), (2, 3), (2, 7)])
@pytest.mark.parametrize("name", sorted(BUILD))
def test_tokens_equal_the_plain_loop(name, B, k, use_cache):
    """(a) n-gram drafts, 24 tokens from a 9-token prompt."""
    m = _model(name)
    idx, want = _reference(name, B)
    torch.manual_seed(5)
    got = m.generate(idx, N, TEMP, TOP_K, use_cache=use_cache, sampler="device", speculative=k)
    assert torch.equal(got, want), (got[:, PROMPT:] != want[:, PROMPT:]).nonzero()[:4].tolist()


@pytest.mark.parametrize("graph", [False, True], ids=["fused", "graph"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(BUILD))
def test_forced_acceptance_patterns(name, pattern, graph):
    """(b) drafts = the reference's own tokens with chosen positions corrupted: the tokens are the
    reference's and the step count is what the accept rule predicts."""
    B, k = 2, 3
    m = _model(name)
    idx, want = _reference(name, B)
    draft = corrupt(want.cpu(), pattern, m.config.vocab_size)
    sess = m.decode_session(B, PROMPT + N - 1, graph=graph, sampler="device", speculative=k, draft=draft.to(DEV))
    torch.manual_seed(5)
    got = sess.generate(idx, N, TEMP, TOP_K)
    assert torch.equal(got, want)
    steps, emitted = predicted_steps(want.cpu(), draft, PROMPT, N, k)
    assert (sess.spec_steps, sess.spec_emitted) == (steps, emitted)
    assert emitted == B * (N - 1)
    if pattern == "none":
        assert steps == math.ceil((N - 1) / (k + 1))
    if pattern == "all":
        assert steps == N - 1
    if graph:  # (e) one captured linear chain, replayed once per step
        assert sess.captures == 1 and sess.replays == sess.spec_steps
    else:
        assert sess.captures == 0 and sess.replays == 0


@pytest.mark.parametrize("name", sorted(BUILD))
def test_generation_up_to_and_past_the_context_limit(name):
    """(c) context 32, k = 7: the verify steps near the limit hold positions past the end of the
    cache; 24 tokens from the session, then 6 from the sliding window, all identical."""
    B, k, n = 2, 7, 30
    m = _model(name, 32)
    idx, want = _reference(name, B, n=n, limit=32)
    assert want.shape == (B, PROMPT + n)
    torch.manual_seed(5)
    got = m.generate(idx, n, TEMP, TOP_K, use_cache="graph", sampler="device", speculative=k)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", sorted(BUILD))
def test_fp8_weights(name):
    """(d) weights="fp8" with speculation equals weights="fp8" without."""
    m = _model(name)
    idx, want = _reference(name, 2, weights="fp8")
    torch.manual_seed(5)
    got = m.generate(idx, N, TEMP, TOP_K, use_cache="graph", sampler="device", weights="fp8", speculative=3)
    assert torch.equal(got, want)


def test_one_graph_and_a_replay_per_step_with_ngram_drafts():
    """(e) with the n-gram draft kernel inside the captured step; a second prompt on the same
    session (reset) replays the same graph."""
    m = _model("llama-tiny")
    idx, want = _reference("llama-tiny", 2)
    sess = m.decode_session(2, PROMPT + N - 1, graph=True, sampler="device", speculative=3, ngram=2)
    for _ in range(2):
        torch.manual_seed(5)
        assert torch.equal(sess.generate(idx, N, TEMP, TOP_K), want)
        assert sess.captures == 1 and sess.replays == sess.spec_steps
        assert sess.cache.pos == PROMPT + N - 1 and sess.cache.lens.tolist() == [PROMPT + N - 1] * 2
        sess.reset()
    assert sess.spec_emitted == 2 * 2 * (N - 1)


def test_refusals():
    """(f) each a ValueError before any launch."""
    m = _model("gpt2-tiny")
    idx = _prompt(m, 1)
    for kw in (dict(sampler="torch", use_cache="graph"), dict(sampler="device", use_cache=True),
               dict(sampler="device", use_cache=False),
               dict(sampler="device", use_cache="graph", kv="fp8"),
               dict(sampler="device", use_cache="graph", speculative=0),
               dict(sampler="device", use_cache="graph", speculative=16),
               dict(sampler="device", use_cache="fused", draft="model"),
               dict(sampler="device", use_cache="fused", draft=torch.zeros(3, 40, dtype=torch.int64))):
        kw.setdefault("speculative", 3)
        with pytest.raises(ValueError):
            m.generate(idx, 4, **kw)
    with pytest.raises(ValueError):
        m.generate(_prompt(m, 3), 4, use_cache="graph", sampler="device", speculative=5)  # 3 x 6 rows
    with pytest.raises(ValueError):
        m.decode_session(2, 16, graph=True, sampler="device", speculative=8)

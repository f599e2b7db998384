"""``sampler="device"`` on the GPU: ``generate(use_cache="graph")`` against ``"fused"`` token for
token, one capture serving other prompts and settings, and every drawn token against the fp64
oracle on the step's own logits and the kernel's Philox uniform."""
import copy

import pytest
import torch

from orion_amd.models.decode_session import DecodeSession
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from sample_fixtures import check_brackets

pytestmark = pytest.mark.gpu
DEV = "cuda"
BM, PROMPT, NEW, TOP_K, MAX_LEN = 2, 37, 12, 50, 64

MODELS = {"gpt2-tiny": lambda: build_gpt2("gpt2-tiny"), "llama-tiny": lambda: build_llama("llama-tiny")}
_SETUPS = {}


def _setup(name):
    """(GPU model, prompt tokens), once per model."""
    if name not in _SETUPS:
        torch.manual_seed(0)
        m = copy.deepcopy(MODELS[name]().eval()).to(DEV).to(torch.bfloat16)
        for bname, buf in m.named_buffers():
            if bname.startswith("rope_"):
                buf.data = buf.data.float()
        g = torch.Generator().manual_seed(1)
        _SETUPS[name] = (m.eval(), torch.randint(0, m.config.vocab_size, (BM, PROMPT), generator=g).to(DEV))
    return _SETUPS[name]


def _check_against_the_oracle(gpu, sess, out, plen, temperature, top_k):
    """An eager default session over the arm's own tokens gives each step's logits; token i of
    every row must sit in the fp64 CDF bracket of u = philox_uniform(seed, position)."""
    replay = DecodeSession(gpu, BM, MAX_LEN, graph=False)
    logits = replay.prefill(out[:, :plen])
    for i in range(out.shape[1] - plen):
        lens = replay.cache.lens.clone()
        assert lens.tolist() == [plen + i] * BM
        u = ref.philox_uniform(sess.rng_seed, lens)
        check_brackets(logits.float(), temperature, top_k, out[:, plen + i:plen + i + 1], u)
        if plen + i + 1 < out.shape[1]:
            logits = replay.step(out[:, plen + i])


@pytest.mark.parametrize("name", list(MODELS))
def test_graph_and_fused_device_sampling(name):
    gpu, prompt = _setup(name)
    V = gpu.config.vocab_size
    torch.manual_seed(3)
    fused = gpu.generate(prompt, NEW, top_k=TOP_K, use_cache="fused", sampler="device")
    torch.manual_seed(3)
    graph = gpu.generate(prompt, NEW, top_k=TOP_K, use_cache="graph", sampler="device")
    assert graph.shape == (BM, PROMPT + NEW) and graph.dtype == prompt.dtype and torch.equal(graph[:, :PROMPT], prompt)
    assert int(graph.min()) >= 0 and int(graph.max()) < V
    assert torch.equal(fused, graph)
    torch.manual_seed(4)
    assert not torch.equal(graph, gpu.generate(prompt, NEW, top_k=TOP_K, use_cache="graph", sampler="device"))

    # one session: counters, the oracle, then another prompt length, temperature and top-k
    sess = gpu.decode_session(BM, MAX_LEN, graph=True, sampler="device")
    eager = gpu.decode_session(BM, MAX_LEN, graph=False, sampler="device")
    torch.manual_seed(3)
    out = sess.generate(prompt, NEW, 1.0, TOP_K)
    assert torch.equal(out, graph)
    assert sess.captures == 1 and sess.replays == NEW - 1 and sess.cache.pos == PROMPT + NEW - 1
    assert torch.equal(sess.history[:, PROMPT:PROMPT + NEW], out[:, PROMPT:]) and torch.equal(sess.tokens, out[:, -1:])
    _check_against_the_oracle(gpu, sess, out, PROMPT, 1.0, TOP_K)
    p2 = 21
    for s in (sess, eager):
        s.reset()
        torch.manual_seed(9)
        s.last = s.generate(prompt[:, :p2], 9, 0.7, 5)
    assert torch.equal(sess.last, eager.last) and sess.last.shape == (BM, p2 + 9)
    assert sess.captures == 1 and sess.replays == NEW - 1 + 8 and eager.captures == 0 and eager.replays == 0
    assert torch.equal(sess.rng_seed, eager.rng_seed)
    _check_against_the_oracle(gpu, sess, sess.last, p2, 0.7, 5)

    # step() keeps its contract and its own graph beside the sampled one
    sess.reset()
    plain = DecodeSession(gpu, BM, MAX_LEN, graph=False)
    sess.prefill(prompt)
    plain.prefill(prompt)
    for n in range(3):
        assert torch.equal(sess.step(out[:, PROMPT + n]), plain.step(out[:, PROMPT + n]))
    assert sess.captures == 2 and sess.replays == NEW - 1 + 8 + 2
    with pytest.raises(ValueError, match="overflow"):
        gpu.decode_session(BM, 40, graph=True, sampler="device").generate(prompt, 6)

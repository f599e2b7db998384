""":class:`DecodeSession` on the GPU: the fused decode step against the CPU fp32 uncached forward
(budget of tests/tolerance.py, the baseline being the stock-op GPU forward as in
tests/test_decode_gpu.py), the captured step bit for bit against the eager one, and the
``generate(use_cache="fused" / "graph")`` modes."""
import copy

import pytest
import torch

from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
BM, PROMPT, STEPS, MAX_LEN = 2, 37, 12, 64

MODELS = {
    "gpt2-tiny": lambda: build_gpt2("gpt2-tiny"),
    "llama-tiny": lambda: build_llama("llama-tiny"),                                  # D 64, GQA 4/2
    "llama-tiny-d128": lambda: build_llama("llama-tiny", dim=512, n_heads=4, n_kv_heads=1),  # D 128, G 4
}


def _gpu_copy(model):
    m = copy.deepcopy(model).to(DEV).to(torch.bfloat16)
    for name, buf in m.named_buffers():
        if name.startswith("rope_"):
            buf.data = buf.data.float()
    return m.eval()


_SETUPS = {}


def _setup(name):
    """(GPU model, tokens, fp32 CPU uncached logits and stock-op GPU logits of every prefix, the
    eager session's logits of every step), computed once per model and left unchanged."""
    if name in _SETUPS:
        return _SETUPS[name]
    torch.manual_seed(0)
    gpu = _gpu_copy(MODELS[name]().eval())
    cpu = copy.deepcopy(gpu).float().cpu()  # the bf16-rounded weights, in fp32
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, cpu.config.vocab_size, (BM, PROMPT + STEPS), generator=g)
    dtoks = toks.to(DEV)
    prefixes = range(PROMPT + 1, PROMPT + STEPS + 1)
    with torch.no_grad():
        want = {n: cpu(toks[:, :n])[0][:, -1] for n in prefixes}
        prev = ops.backend()
        try:
            ops.set_backend("torch")
            base = {n: gpu(dtoks[:, :n])[0][:, -1].cpu() for n in prefixes}
        finally:
            ops.set_backend(prev)
    eager = DecodeSession(gpu, BM, MAX_LEN, graph=False)
    eager.prefill(dtoks[:, :PROMPT])
    steps = [eager.step(dtoks[:, n:n + 1]).clone() for n in range(PROMPT, PROMPT + STEPS)]
    assert eager.cache.pos == PROMPT + STEPS and eager.captures == 0
    _SETUPS[name] = (gpu, dtoks, want, base, steps, eager)
    return _SETUPS[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_fused_step_logits_against_the_uncached_forward(name):
    gpu, dtoks, want, base, steps, eager = _setup(name)
    for i, logits in enumerate(steps):
        n = PROMPT + i + 1
        assert logits.shape == (BM, gpu.config.vocab_size) and logits.dtype == torch.bfloat16
        e, b = within_bf16_budget(f"logits after {n} tokens", logits.cpu(), want[n], base[n])
    print(f"{name}: last step err {e:.3e} baseline {b:.3e}")


@pytest.mark.parametrize("name", list(MODELS))
def test_captured_step_is_bit_equal_to_the_eager_step(name):
    gpu, dtoks, _, _, steps, eager = _setup(name)
    sess = gpu.decode_session(BM, MAX_LEN, graph=True)
    sess.prefill(dtoks[:, :PROMPT])
    assert sess.captures == 0
    for i, n in enumerate(range(PROMPT, PROMPT + STEPS)):
        logits = sess.step(dtoks[:, n:n + 1])
        assert logits is sess.logits
        assert torch.equal(logits, steps[i]), f"step {i}"
    assert sess.captures == 1 and sess.replays == STEPS - 1
    assert sess.cache.lens.tolist() == [PROMPT + STEPS] * BM and sess.cache.pos == PROMPT + STEPS
    # a second prompt of another length on the same session: no new capture, still bit-equal
    other = DecodeSession(gpu, BM, MAX_LEN, graph=False)
    sess.reset()
    p2 = 21
    sess.prefill(dtoks[:, :p2])
    other.prefill(dtoks[:, :p2])
    for n in range(p2, p2 + 3):
        assert torch.equal(sess.step(dtoks[:, n:n + 1]), other.step(dtoks[:, n:n + 1])), f"second prompt, token {n}"
    assert sess.captures == 1 and sess.replays == STEPS - 1 + 3
    assert sess.cache.lens.tolist() == [p2 + 3] * BM


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny-window"])
def test_generate_graph_equals_fused_token_for_token(name):
    """Same seed, same tokens: the two arms draw from bit-equal logits.  llama-tiny with a window
    of 48 and a prompt of 40 also hands over to the uncached loop (9 session tokens, 3 beyond)."""
    torch.manual_seed(0)
    if name == "gpt2-tiny":
        gpu, plen = _gpu_copy(build_gpt2("gpt2-tiny")), 37
    else:
        gpu, plen = _gpu_copy(build_llama("llama-tiny", max_seq_len=48)), 40
    prompt = torch.randint(0, gpu.config.vocab_size, (BM, plen), device=DEV)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(3)
        outs[mode] = gpu.generate(prompt, 12, top_k=50, use_cache=mode)
        assert outs[mode].shape == (BM, plen + 12) and torch.equal(outs[mode][:, :plen], prompt)
        assert int(outs[mode].min()) >= 0 and int(outs[mode].max()) < gpu.config.vocab_size
    assert torch.equal(outs["fused"], outs["graph"])


def test_graph_session_refuses_what_it_cannot_capture():
    gpu = _setup("gpt2-tiny")[0]
    with pytest.raises(ValueError, match="batch 17"):
        DecodeSession(gpu, batch=17, max_len=32, graph=True)
    DecodeSession(gpu, batch=17, max_len=32, graph=False)  # the plain-op composition takes it
    with pytest.raises(ValueError, match="not eligible"):
        DecodeSession(copy.deepcopy(gpu).float(), batch=2, max_len=32, graph=True)
    small = gpu.decode_session(1, 4, graph=True)
    small.prefill(torch.zeros(1, 4, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match="overflow"):
        small.step(torch.zeros(1, 1, dtype=torch.long, device=DEV))
    assert small.captures == 0 and small.cache.pos == 4 and small.cache.lens.tolist() == [4]

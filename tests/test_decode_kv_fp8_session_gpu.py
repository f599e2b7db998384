""":class:`DecodeSession` with an FP8 key/value cache (``kv="fp8"``) on the GPU, on the models and
constants of tests/test_decode_graph_gpu.py.  Quantisation is discontinuous, so two whole runs are
not compared: a step is judged from shared state -- the session's cache after n tokens is copied
into an fp32 CPU model's FP8 cache, whose ``forward_cached`` of the next token is the reference,
and into a stock-op bf16 GPU run, which is the baseline (budget of tests/tolerance.py).  The
captured step is bit-equal to the eager one."""
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
CHECK_AT = (37, 42, 48)  # tokens in the cache before the judged step

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


def _clone_cache(model, src, device):
    """An FP8 cache of ``model`` holding what ``src`` holds: bytes, scales, lens, start, pos."""
    c = model.new_cache(BM, MAX_LEN, kv_dtype="fp8")
    assert c.buf.shape == src.buf.shape and c.scales.shape == src.scales.shape
    c.buf.view(torch.uint8).copy_(src.buf.view(torch.uint8).to(device))
    c.scales.copy_(src.scales.to(device))
    c.lens.copy_(src.lens.to(device))
    c.start.copy_(src.start.to(device))
    c.pos = src.pos
    return c


_SETUPS = {}


def _setup(name):
    """(GPU model, tokens, the eager FP8 session's logits of every step, and per checked n the fp32
    CPU reference and the stock-op bf16 baseline of that step from the session's own cache),
    computed once per model and left unchanged."""
    if name in _SETUPS:
        return _SETUPS[name]
    torch.manual_seed(0)
    gpu = _gpu_copy(MODELS[name]().eval())
    cpu = copy.deepcopy(gpu).float().cpu()  # the bf16-rounded weights, in fp32
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, cpu.config.vocab_size, (BM, PROMPT + STEPS), generator=g)
    dtoks = toks.to(DEV)
    eager = DecodeSession(gpu, BM, MAX_LEN, graph=False, kv="fp8")
    eager.prefill(dtoks[:, :PROMPT])
    steps, want, base = [], {}, {}
    for n in range(PROMPT, PROMPT + STEPS):
        if n in CHECK_AT:
            assert eager.cache.pos == n
            with torch.no_grad():
                want[n] = cpu.forward_cached(toks[:, n:n + 1], _clone_cache(cpu, eager.cache, "cpu"))
                prev = ops.backend()
                try:
                    ops.set_backend("torch")
                    base[n] = gpu.forward_cached(dtoks[:, n:n + 1], _clone_cache(gpu, eager.cache, DEV)).cpu()
                finally:
                    ops.set_backend(prev)
        steps.append(eager.step(dtoks[:, n:n + 1]).clone())
    assert eager.cache.pos == PROMPT + STEPS and eager.captures == 0
    _SETUPS[name] = (gpu, dtoks, steps, want, base)
    return _SETUPS[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_one_step_from_the_sessions_own_cache(name):
    gpu, dtoks, steps, want, base = _setup(name)
    for n in CHECK_AT:
        logits = steps[n - PROMPT]
        assert logits.shape == (BM, gpu.config.vocab_size) and logits.dtype == torch.bfloat16
        assert torch.isfinite(logits).all()
        e, b = within_bf16_budget(f"logits of the step after {n} tokens", logits.cpu(), want[n], base[n])
        print(f"{name} n {n}: err {e:.3e} baseline {b:.3e}")


@pytest.mark.parametrize("name", list(MODELS))
def test_captured_step_is_bit_equal_to_the_eager_step(name):
    gpu, dtoks, steps, _, _ = _setup(name)
    sess = gpu.decode_session(BM, MAX_LEN, graph=True, kv="fp8")
    sess.prefill(dtoks[:, :PROMPT])
    assert sess.captures == 0
    for i, n in enumerate(range(PROMPT, PROMPT + STEPS)):
        logits = sess.step(dtoks[:, n:n + 1])
        assert logits is sess.logits
        assert torch.equal(logits, steps[i]), f"step {i}"
    assert sess.captures == 1 and sess.replays == STEPS - 1
    assert sess.cache.lens.tolist() == [PROMPT + STEPS] * BM and sess.cache.pos == PROMPT + STEPS
    # a second prompt of another length on the same session: no new capture, still bit-equal
    other = DecodeSession(gpu, BM, MAX_LEN, graph=False, kv="fp8")
    sess.reset()
    p2 = 21
    sess.prefill(dtoks[:, :p2])
    other.prefill(dtoks[:, :p2])
    for n in range(p2, p2 + 3):
        assert torch.equal(sess.step(dtoks[:, n:n + 1]), other.step(dtoks[:, n:n + 1])), f"second prompt, token {n}"
    assert sess.captures == 1 and sess.replays == STEPS - 1 + 3


@pytest.mark.parametrize("extra", [{}, {"sampler": "device"}, {"sampler": "device", "weights": "fp8"}],
                         ids=["torch-sampler", "device-sampler", "device-sampler-fp8-weights"])
@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_graph_equals_fused_token_for_token(name, extra):
    gpu = _setup(name)[0]
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, gpu.config.vocab_size, (BM, PROMPT), generator=g).to(DEV)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(3)
        outs[mode] = gpu.generate(prompt, 12, top_k=50, use_cache=mode, kv="fp8", **extra)
        assert outs[mode].shape == (BM, PROMPT + 12) and torch.equal(outs[mode][:, :PROMPT], prompt)
        assert int(outs[mode].min()) >= 0 and int(outs[mode].max()) < gpu.config.vocab_size
    assert torch.equal(outs["fused"], outs["graph"])


def test_generate_with_a_plain_fp8_cache_on_the_gpu():
    gpu = _setup("llama-tiny")[0]
    prompt = torch.randint(0, gpu.config.vocab_size, (BM, 20), device=DEV)
    out = gpu.generate(prompt, 8, top_k=50, use_cache=True, kv="fp8")
    assert out.shape == (BM, 28) and torch.equal(out[:, :20], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < gpu.config.vocab_size


@pytest.mark.parametrize("name", list(MODELS))
def test_cache_bytes_and_unchanged_defaults(name):
    gpu, dtoks, _, _, _ = _setup(name)
    D = gpu.config.head_dim
    plain, kw, q = DecodeSession(gpu, BM, MAX_LEN), DecodeSession(gpu, BM, MAX_LEN, kv="bf16"), \
        DecodeSession(gpu, BM, MAX_LEN, kv="fp8")
    assert plain.cache.buf.dtype == kw.cache.buf.dtype == torch.bfloat16 and plain.cache.scales is None
    assert q.cache_bytes * 2 * D == plain.cache_bytes * (D + 4) and plain.cache_bytes == kw.cache_bytes
    a, b = plain.prefill(dtoks[:, :PROMPT]), kw.prefill(dtoks[:, :PROMPT])
    assert torch.equal(a, b)
    for n in range(PROMPT, PROMPT + 3):
        assert torch.equal(plain.step(dtoks[:, n:n + 1]), kw.step(dtoks[:, n:n + 1]))
    with pytest.raises(ValueError, match="kv must be"):
        DecodeSession(gpu, BM, MAX_LEN, kv="int8")

""":class:`DecodeSession` with ``weights="mxfp4"`` on the GPU: the step's logits against the CPU
fp32 uncached forward of a twin model that holds the session's exactly dequantised weights (budget
of tests/tolerance.py, the baseline being the stock-op GPU bf16 forward of the twin), the captured
step bit for bit against the eager one, the ``generate(weights="mxfp4")`` modes with the device
sampler, speculative decoding and an FP8 cache, and the bf16 session unchanged.  Models and
constants are those of tests/test_decode_fp8_session_gpu.py."""
import copy

import pytest
import torch

import mxfp4_cases as mc
from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from tolerance import FACTOR, FLOOR, rel_err, within_bf16_budget

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
    """(GPU model, tokens, the twin's fp32 CPU logits, the twin's stock-op GPU bf16 logits and the
    unquantised model's fp32 CPU logits of every prefix, the eager mxfp4 session's logits of every
    step, that session, a bf16 session's prefill logits taken before any mxfp4 session existed),
    computed once per model and left unchanged."""
    if name in _SETUPS:
        return _SETUPS[name]
    torch.manual_seed(0)
    gpu = _gpu_copy(MODELS[name]().eval())
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, gpu.config.vocab_size, (BM, PROMPT + STEPS), generator=g)
    dtoks = toks.to(DEV)
    first = DecodeSession(gpu, BM, MAX_LEN).prefill(dtoks[:, :PROMPT]).clone()
    eager = DecodeSession(gpu, BM, MAX_LEN, graph=False, weights="mxfp4")
    twin32 = mc.twin_of(gpu, eager.qweights, torch.float32, "cpu")
    twin16 = mc.twin_of(gpu, eager.qweights, torch.bfloat16)
    plain32 = copy.deepcopy(gpu).float().cpu()
    prefixes = range(PROMPT + 1, PROMPT + STEPS + 1)
    with torch.no_grad():
        want = {n: twin32(toks[:, :n])[0][:, -1] for n in prefixes}
        plain = {n: plain32(toks[:, :n])[0][:, -1] for n in prefixes}
        prev = ops.backend()
        try:
            ops.set_backend("torch")
            base = {n: twin16(dtoks[:, :n])[0][:, -1].cpu() for n in prefixes}
        finally:
            ops.set_backend(prev)
    eager.prefill(dtoks[:, :PROMPT])
    steps = [eager.step(dtoks[:, n:n + 1]).clone() for n in range(PROMPT, PROMPT + STEPS)]
    assert eager.cache.pos == PROMPT + STEPS and eager.captures == 0
    _SETUPS[name] = (gpu, dtoks, want, base, plain, steps, eager, first)
    return _SETUPS[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_mxfp4_step_logits_against_the_twin(name):
    gpu, dtoks, want, base, plain, steps, eager, _ = _setup(name)
    for i, logits in enumerate(steps):
        n = PROMPT + i + 1
        assert logits.shape == (BM, gpu.config.vocab_size) and logits.dtype == torch.bfloat16
        e, b = within_bf16_budget(f"logits after {n} tokens", logits.cpu(), want[n], base[n])
        far = rel_err(logits.cpu(), plain[n])
        assert far > FACTOR * b + FLOOR, f"after {n} tokens: {far:.3e} from the unquantised model, budget " \
                                         f"{FACTOR * b + FLOOR:.3e}"
    print(f"{name}: last step err {e:.3e} baseline {b:.3e}, from the unquantised model {far:.3e}")


@pytest.mark.parametrize("name", list(MODELS))
def test_captured_mxfp4_step_is_bit_equal_to_the_eager_step(name):
    gpu, dtoks, _, _, _, steps, eager, _ = _setup(name)
    sess = gpu.decode_session(BM, MAX_LEN, graph=True, weights="mxfp4")
    sess.prefill(dtoks[:, :PROMPT])
    assert sess.captures == 0
    for i, n in enumerate(range(PROMPT, PROMPT + STEPS)):
        logits = sess.step(dtoks[:, n:n + 1])
        assert logits is sess.logits
        assert torch.equal(logits, steps[i]), f"step {i}"
    assert sess.captures == 1 and sess.replays == STEPS - 1
    assert sess.cache.lens.tolist() == [PROMPT + STEPS] * BM and sess.cache.pos == PROMPT + STEPS
    # a second prompt of another length on the same session: no new capture, still bit-equal
    other = DecodeSession(gpu, BM, MAX_LEN, graph=False, weights="mxfp4")
    sess.reset()
    p2 = 21
    sess.prefill(dtoks[:, :p2])
    other.prefill(dtoks[:, :p2])
    for n in range(p2, p2 + 3):
        assert torch.equal(sess.step(dtoks[:, n:n + 1]), other.step(dtoks[:, n:n + 1])), f"second prompt, token {n}"
    assert sess.captures == 1 and sess.replays == STEPS - 1 + 3


@pytest.mark.parametrize("name,sampler", [("gpt2-tiny", "torch"), ("llama-tiny-window", "torch"),
                                          ("llama-tiny", "device"), ("gpt2-tiny", "device")])
def test_generate_mxfp4_graph_equals_fused_token_for_token(name, sampler):
    """Same seed, same tokens: the two arms draw from bit-equal logits.  llama-tiny with a window
    of 48 and a prompt of 40 also hands over to the uncached loop (9 session tokens, 3 beyond)."""
    torch.manual_seed(0)
    if name == "gpt2-tiny":
        gpu, plen = _gpu_copy(build_gpt2("gpt2-tiny")), 37
    elif name == "llama-tiny":
        gpu, plen = _gpu_copy(build_llama("llama-tiny")), 37
    else:
        gpu, plen = _gpu_copy(build_llama("llama-tiny", max_seq_len=48)), 40
    prompt = torch.randint(0, gpu.config.vocab_size, (BM, plen), device=DEV)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(3)
        outs[mode] = gpu.generate(prompt, 12, top_k=50, use_cache=mode, sampler=sampler, weights="mxfp4")
        assert outs[mode].shape == (BM, plen + 12) and torch.equal(outs[mode][:, :plen], prompt)
        assert int(outs[mode].min()) >= 0 and int(outs[mode].max()) < gpu.config.vocab_size
    assert torch.equal(outs["fused"], outs["graph"])


@pytest.mark.parametrize("mode", ["fused", "graph"])
def test_speculative_mxfp4_emits_the_plain_mxfp4_tokens(mode):
    """``speculative=3`` with a given draft (the plain run's own tokens, half of them spoilt) emits
    the tokens of the non-speculative mxfp4 run under the same seed."""
    gpu, dtoks = _setup("llama-tiny")[:2]
    prompt, new = dtoks[:, :PROMPT], 12
    kw = dict(top_k=50, use_cache=mode, sampler="device", weights="mxfp4")
    torch.manual_seed(5)
    plain = gpu.generate(prompt, new, **kw)
    draft = plain.clone()
    draft[:, PROMPT + 1::2] = (draft[:, PROMPT + 1::2] + 1) % gpu.config.vocab_size  # wrong guesses too
    torch.manual_seed(5)
    spec = gpu.generate(prompt, new, speculative=3, draft=draft, **kw)
    assert torch.equal(spec, plain)


def test_mxfp4_weights_with_an_fp8_cache():
    gpu, dtoks = _setup("llama-tiny")[:2]
    torch.manual_seed(7)
    out = gpu.generate(dtoks[:, :PROMPT], 8, top_k=50, use_cache="graph", sampler="device", weights="mxfp4",
                       kv="fp8")
    assert out.shape == (BM, PROMPT + 8) and torch.equal(out[:, :PROMPT], dtoks[:, :PROMPT])
    assert int(out.min()) >= 0 and int(out.max()) < gpu.config.vocab_size


def test_bf16_sessions_are_unchanged_and_refusals():
    gpu, dtoks = _setup("gpt2-tiny")[:2]
    first = _setup("gpt2-tiny")[-1]
    a = DecodeSession(gpu, BM, MAX_LEN)
    b = DecodeSession(gpu, BM, MAX_LEN, weights="bf16")
    assert a.qweights is None and b.qweights is None
    la = a.prefill(dtoks[:, :PROMPT])
    assert torch.equal(la, first)  # as the session built before any mxfp4 session
    assert torch.equal(la, b.prefill(dtoks[:, :PROMPT]))
    for n in range(PROMPT, PROMPT + 3):
        assert torch.equal(a.step(dtoks[:, n:n + 1]), b.step(dtoks[:, n:n + 1]))
    q = _setup("gpt2-tiny")[-2]
    projections = list(gpu.decode_projections())
    assert q.weight_bytes == sum(p.numel() // 2 + p.numel() // 32 for _, p in projections)
    assert a.weight_bytes == sum(2 * p.numel() for _, p in projections)
    assert all(isinstance(w, ops.Mxfp4Weight) and w.device == p.device
               for w, (_, p) in zip(q.qweights.values(), projections))
    prompt = dtoks[:, :8]
    with pytest.raises(ValueError, match="weights must be"):
        DecodeSession(gpu, BM, MAX_LEN, weights="fp4")
    for mode in (True, False):
        with pytest.raises(ValueError, match="weights='mxfp4'"):
            gpu.generate(prompt, 2, use_cache=mode, weights="mxfp4")
    # down_proj with K = 520: K % 8 == 0 serves the bf16 graph session, K % 32 != 0 refuses the mxfp4 one
    torch.manual_seed(0)
    odd = _gpu_copy(build_llama("llama-tiny", ffn_dim=520))
    DecodeSession(odd, BM, 32, graph=True)
    with pytest.raises(ValueError, match="K % 32"):
        DecodeSession(odd, BM, 32, graph=True, weights="mxfp4")

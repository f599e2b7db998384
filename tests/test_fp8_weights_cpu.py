"""Weight-only FP8 decode on the CPU: the quantisation rule of ``ops.quantize_fp8``,
``ops.linear_decode`` on an ``ops.Fp8Weight`` through the reference path, a
``DecodeSession(weights="fp8")`` against a twin model that holds the dequantised weights, the
``generate(weights="fp8")`` surface, and an emulation of the ideal FP8 kernel on every case of the
GPU sweep (tests/fp8_cases.py) that keeps that sweep's budget honest."""
import itertools

import pytest
import torch

import fp8_cases as fc
from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.ops import reference as ref
from test_decode_fused_cpu import BOUND, EPIS, NORMS, _model, linear_decode_case
from tolerance import FACTOR, FLOOR, rel_err

B, PROMPT, STEPS = 2, 19, 9
E4M3_NAN = 0x7F  # and 0xFF: the only non-finite codes of e4m3fn


def _rows_over_six_decades(n=64, k=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * (10.0 ** torch.linspace(-3, 3, n))[:, None]
    w[::7] *= torch.rand(k, generator=g) ** 8  # some rows with many values far below their maximum
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_quantize_fp8_follows_the_rule(dtype):
    w = _rows_over_six_decades().to(dtype)
    if dtype == torch.float16:
        w = (w.float() / 4).to(dtype)  # inside fp16's range
    w[5] = 0
    qw = ops.quantize_fp8(w)
    assert isinstance(qw, ops.Fp8Weight)
    assert qw.q.dtype == torch.float8_e4m3fn and qw.scale.dtype == torch.float32
    assert qw.shape == w.shape and qw.q.shape == w.shape and qw.scale.shape == (w.shape[0],)
    assert qw.q.is_contiguous() and qw.scale.is_contiguous() and qw.device == w.device
    assert qw.nbytes == w.numel() + 4 * w.shape[0]
    wf = w.float()
    amax = wf.abs().amax(1)
    want_scale = amax / 448
    want_scale[5] = 1.0
    assert torch.equal(qw.scale, want_scale)
    bits = qw.q.view(torch.uint8)
    assert not ((bits & 0x7F) == E4M3_NAN).any()  # no NaN byte
    qf = qw.q.float()
    assert torch.equal(qf.abs().amax(1)[amax > 0], torch.full_like(amax[amax > 0], 448.0))
    where = wf.abs().argmax(1)
    assert torch.equal(qf.gather(1, where[:, None])[:, 0], 448.0 * torch.sign(wf.gather(1, where[:, None])[:, 0]))
    assert torch.equal(qf[5], torch.zeros_like(qf[5]))
    # half a unit in the last place of a 3-bit mantissa, or half the subnormal spacing 2^-9
    deq = qw.dequant(torch.float32)
    assert torch.equal(deq, qf * qw.scale[:, None])
    bound = torch.maximum(wf.abs() * 2.0 ** -4, qw.scale[:, None] * 2.0 ** -10)
    ratio = ((deq - wf).abs() / bound.clamp_min(1e-45)).max().item()
    print(f"{dtype}: worst |dequant - w| / bound {ratio:.3f}")
    assert ((deq - wf).abs() <= bound).all(), ratio
    assert qw.dequant(torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(Exception):
        qw.q = qw.q  # immutable


def test_quantize_fp8_clamps_before_the_cast():
    """A value that rounds above 448 after the division must saturate, never become NaN."""
    w = torch.tensor([[1.0, -1.0, 0.999999, 1e-9], [3e38, -3e38, 1.0, 0.0]])
    qw = ops.quantize_fp8(w)
    assert torch.isfinite(qw.q.float()).all()
    assert qw.q.float()[:, :2].abs().eq(448).all()


@pytest.mark.parametrize("norm,epi", list(itertools.product(NORMS, EPIS)))
def test_linear_decode_on_an_fp8_weight_equals_the_reference_on_the_dequantised(norm, epi):
    kw, _ = linear_decode_case(norm, epi)
    qw = ops.quantize_fp8(kw["weight"])
    assert not ops.linear_decode_eligible(kw["x"], qw)
    got = fc.call(dict(kw, weight=qw))
    kw.pop("weight")
    want = ref.linear_decode(kw.pop("x"), qw.dequant(torch.float32), kw.pop("bias", None), **kw)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert rel_err(got, want) <= BOUND
    assert "Fp8Weight" in ops.__all__ and "quantize_fp8" in ops.__all__


@pytest.fixture(scope="module", params=["gpt2-tiny", "llama-tiny"])
def quantised(request):
    """(model, eager fp8 session, tokens, uncached last-position logits of every prefix length of
    the twin and of the unquantised model), computed once."""
    model = _model(request.param)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    sess = DecodeSession(model, B, PROMPT + STEPS, weights="fp8")
    assert all(torch.equal(p, before[n]) for n, p in model.named_parameters())  # not modified
    names = [n for n, _ in model.decode_projections()]
    assert list(sess.qweights) == names and "lm_head" in names
    assert all(isinstance(q, ops.Fp8Weight) and q.shape == p.shape
               for q, (_, p) in zip(sess.qweights.values(), model.decode_projections()))
    assert sess.weight_bytes == sum(p.numel() + 4 * p.shape[0] for _, p in model.decode_projections())
    twin = fc.twin_of(model, sess.qweights)
    if request.param == "gpt2-tiny":  # the head is quantised, the token table is not
        assert torch.equal(twin.transformer.wte.weight, model.lm_head.weight)
        assert not torch.equal(twin.lm_head.weight, model.lm_head.weight)
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, model.config.vocab_size, (B, PROMPT + STEPS), generator=g)
    with torch.no_grad():
        want = {n: twin(toks[:, :n])[0][:, -1] for n in range(PROMPT, PROMPT + STEPS + 1)}
        plain = {n: model(toks[:, :n])[0][:, -1] for n in range(PROMPT, PROMPT + STEPS + 1)}
    return model, toks, want, plain


@pytest.mark.parametrize("chunks", [(PROMPT,), (11, 8)], ids=["prefill", "chunked-prefill"])
def test_fp8_session_is_the_twin_model_and_not_the_unquantised_one(quantised, chunks):
    model, toks, want, plain = quantised
    sess = model.decode_session(B, PROMPT + STEPS, weights="fp8")
    at = 0
    for n in chunks:
        logits = sess.prefill(toks[:, at:at + n])
        at += n
    assert rel_err(logits, want[PROMPT]) <= BOUND
    assert rel_err(logits, plain[PROMPT]) > BOUND
    for step in range(STEPS):
        n = PROMPT + step
        logits = sess.step(toks[:, n:n + 1])
        e, far = rel_err(logits, want[n + 1]), rel_err(logits, plain[n + 1])
        assert e <= BOUND, f"step {step}: {e:.3e}"
        assert far > BOUND, f"step {step}: {far:.3e} from the unquantised model"
    print(f"last step: {e:.3e} from the twin, {far:.3e} from the unquantised model")
    sess.reset()
    assert rel_err(sess.prefill(toks[:, :PROMPT]), want[PROMPT]) <= BOUND


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_fp8_surface_and_refusals(name):
    model = _model(name)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, model.config.vocab_size, (B, 7), generator=g)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(11)
        out = outs[mode] = model.generate(prompt, 6, temperature=0.9, top_k=20, use_cache=mode, weights="fp8")
        assert out.shape == (B, 13) and torch.equal(out[:, :7], prompt)
        assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size
    assert torch.equal(outs["fused"], outs["graph"])
    for mode in (False, True):
        with pytest.raises(ValueError, match="weights='fp8'"):
            model.generate(prompt, 2, use_cache=mode, weights="fp8")
    with pytest.raises(ValueError, match="weights must be"):
        model.generate(prompt, 2, use_cache="fused", weights="int8")
    with pytest.raises(ValueError, match="weights must be"):
        DecodeSession(model, B, 16, weights="fp4")
    for sess in (DecodeSession(model, B, 16), model.decode_session(B, 16), model.decode_session(B, 16, weights="bf16")):
        assert sess.qweights is None and sess.weights == "bf16"
        assert sess.weight_bytes == sum(p.numel() * p.element_size() for _, p in model.decode_projections())


def test_sample_script_forwards_decode_weights(monkeypatch, capsys):
    """``sample.py --decode_weights=fp8`` reaches ``generate(weights="fp8")``."""
    import sample
    from orion_amd.train import ckpt
    model = _model("gpt2-tiny")
    seen = []
    generate = model.generate

    def spy(*args, **kw):
        seen.append(kw)
        return generate(*args, **kw)

    model.generate = spy
    monkeypatch.setattr(ckpt, "load_checkpoint", lambda path: {})
    monkeypatch.setattr(ckpt, "build_model_from_checkpoint", lambda ck: model)
    argv = ["--device=cpu", "--num_samples=1", "--max_new_tokens=3", "--start=ids:1,2", "--kv_cache=fused"]
    sample.main(argv + ["--decode_weights=fp8"])
    sample.main(argv)
    assert [kw["weights"] for kw in seen] == ["fp8", "bf16"] and seen[0]["use_cache"] == "fused"
    assert capsys.readouterr().out.count("[1, 2,") == 2
    with pytest.raises(ValueError, match="weights='fp8'"):
        sample.main(argv[:-1] + ["--decode_weights=fp8"])


@pytest.mark.parametrize("norm", fc.NORMS)
@pytest.mark.parametrize("n,k", fc.SHAPES)
def test_ideal_kernel_emulation_has_headroom_in_the_gpu_budget(n, k, norm):
    """An ideal FP8 kernel, emulated in fp32 on the cases of the GPU sweep, reaches at most 0.7 x
    that sweep's budget (2 x the bf16 baseline's error + 1e-3): the budget can be met with room
    for the summation order, and a real kernel that misses it is wrong."""
    worst = 0.0
    for m in fc.MS:
        for epi in fc.EPIS:
            kw = fc.make_case(m, n, k, norm, epi, seed=m)
            want = fc.composed(kw, torch.float32)
            e = rel_err(fc.ideal_kernel(kw), want)
            b = rel_err(fc.composed(kw, torch.bfloat16), want)
            worst = max(worst, e / (FACTOR * b + FLOOR))
            assert e <= 0.7 * (FACTOR * b + FLOOR), f"M{m} N{n} K{k} {norm} {epi}: {e:.3e} vs baseline {b:.3e}"
    print(f"N{n} K{k} {norm}: worst ideal err / budget {worst:.2f}")

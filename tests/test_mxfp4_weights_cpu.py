"""Weight-only MXFP4 decode on the CPU: the quantisation rule of ``ops.quantize_mxfp4``,
``ops.linear_decode`` on an ``ops.Mxfp4Weight`` through the reference path, a
``DecodeSession(weights="mxfp4")`` against a twin model that holds the dequantised weights, the
``generate(weights="mxfp4")`` surface, and an emulation of the ideal MXFP4 kernel on every case of
the GPU sweep (tests/mxfp4_cases.py) that keeps that sweep's budget honest."""
import itertools

import pytest
import torch

import mxfp4_cases as mc
from orion_amd import ops
from orion_amd.models.decode_session import DecodeSession
from orion_amd.ops import reference as ref
from test_decode_fused_cpu import BOUND, EPIS, NORMS, _model, linear_decode_case
from tolerance import FACTOR, FLOOR, rel_err

B, PROMPT, STEPS = 2, 19, 9
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _rows_over_six_decades(n=64, k=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * (10.0 ** torch.linspace(-3, 3, n))[:, None]
    w[::7] *= torch.rand(k, generator=g) ** 8  # some blocks with most values far below their maximum
    return w


def _codes(qw):
    """The (N, K) e2m1 codes of an Mxfp4Weight, even k from the low nibble."""
    return torch.stack((qw.q & 15, qw.q >> 4), dim=-1).view(qw.q.shape[0], -1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_quantize_mxfp4_follows_the_rule(dtype):
    w = _rows_over_six_decades().to(dtype)
    if dtype == torch.float16:
        w = (w.float() / 4).to(dtype)  # inside fp16's range
    w[5] = 0
    N, K = w.shape
    qw = ops.quantize_mxfp4(w)
    assert isinstance(qw, ops.Mxfp4Weight)
    assert qw.q.dtype == torch.uint8 and qw.scale.dtype == torch.uint8
    assert qw.shape == w.shape and qw.q.shape == (N, K // 2) and qw.scale.shape == (N, K // 32)
    assert qw.q.is_contiguous() and qw.scale.is_contiguous() and qw.device == w.device
    assert qw.nbytes == N * K // 2 + N * K // 32
    wf = w.float().view(N, K // 32, 32)
    amax = wf.abs().amax(-1)
    want = 127 + torch.floor(torch.log2(amax.double())).long() - 2  # fp64 log2 of an fp32: floor is exact here
    want[amax == 0] = 127
    assert torch.equal(qw.scale.long(), want)
    assert int(qw.scale.min()) >= 2 and int(qw.scale.max()) <= 252
    mags = GRID[(_codes(qw) & 7).long()].view(N, K // 32, 32)
    top = mags.amax(-1)
    assert ((top == 4) | (top == 6))[amax > 0].all()  # the largest element lands in [4, 8) / 2^e
    assert (top[amax == 0] == 0).all() and torch.equal(qw.q[5], torch.zeros_like(qw.q[5]))
    deq = qw.dequant(torch.float32)
    e = (qw.scale.float() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(deq.abs(), mags.view(N, K) * torch.exp2(e))
    assert torch.equal(torch.signbit(deq), torch.signbit(w.float()))
    # half a step of a 1-bit mantissa, half the subnormal step 2^e / 2, the saturation of (6, 8) -> 6
    bound = torch.maximum(w.float().abs(), torch.exp2(e)) * 2.0 ** -2
    ratio = ((deq - w.float()).abs() / bound).max().item()
    print(f"{dtype}: worst |dequant - w| / bound {ratio:.3f}")
    assert ((deq - w.float()).abs() <= bound).all(), ratio
    bf = qw.dequant(torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf.float(), deq)  # exact in bf16 too
    with pytest.raises(Exception):
        qw.q = qw.q  # immutable


def test_quantize_mxfp4_ties_go_to_the_even_code():
    w = torch.zeros(2, 32)
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[0, :7], w[0, 7] = mids, 4.0  # amax 4: e = 0
    w[1, :7], w[1, 7] = -mids * 2.0 ** -9, 2.0 ** -7  # the same at e = -9, negative
    qw = ops.quantize_mxfp4(w)
    assert qw.scale.flatten().tolist() == [127, 118]
    codes = _codes(qw)
    assert codes[0, :8].tolist() == [0, 2, 2, 4, 4, 6, 6, 6]  # 0, 1, 1, 2, 2, 4, 4 and the 4 itself
    assert codes[1, :8].tolist() == [8, 10, 10, 12, 12, 14, 14, 6]
    assert qw.dequant()[0, :8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]


def test_quantize_mxfp4_stays_finite_at_the_ends_of_fp32():
    w = torch.zeros(3, 64)
    w[0, :3] = torch.tensor([3e38, -3e38, 1.0])
    w[1, :2] = torch.tensor([1e-45, -1e-45])
    w[2, 32:35] = torch.tensor([1e-45, 3e38, -1e30])
    qw = ops.quantize_mxfp4(w)
    assert int(qw.scale.min()) >= 2 and int(qw.scale.max()) <= 252
    for dtype in (torch.float32, torch.bfloat16):
        d = qw.dequant(dtype)
        assert torch.isfinite(d).all()
        assert d[0, 0] == 6 * 2.0 ** 125 and d[0, 1] == -6 * 2.0 ** 125  # saturated, not NaN or inf
    assert torch.equal(qw.dequant(torch.bfloat16).float(), qw.dequant(torch.float32))


def test_mxfp4_weight_rejects_wrong_dtypes_and_shapes():
    q, s = torch.zeros(4, 32, dtype=torch.uint8), torch.full((4, 2), 127, dtype=torch.uint8)
    w = ops.Mxfp4Weight(q, s)
    assert w.shape == (4, 64) and w.nbytes == 4 * 32 + 4 * 2 and w.device == q.device
    assert torch.equal(w.dequant(), torch.zeros(4, 64))
    for bad_q, bad_s in ((q.to(torch.int8), s), (q, s.float()), (q, s[:, :1].contiguous()), (q, s[:3]),
                         (q[:, :24].contiguous(), s), (q.t().contiguous().t(), s), (q, s.t().contiguous().t()),
                         (q[0], s[0])):
        with pytest.raises(AssertionError):
            ops.Mxfp4Weight(bad_q, bad_s)
    with pytest.raises(AssertionError, match="K % 32"):
        ops.quantize_mxfp4(torch.randn(4, 48))


@pytest.mark.parametrize("norm,epi", list(itertools.product(NORMS, EPIS)))
def test_linear_decode_on_an_mxfp4_weight_equals_the_reference_on_the_dequantised(norm, epi):
    kw, _ = linear_decode_case(norm, epi, k=96)
    qw = ops.quantize_mxfp4(kw["weight"])
    assert not ops.linear_decode_eligible(kw["x"], qw)
    got = mc.call(dict(kw, weight=qw))
    kw.pop("weight")
    want = ref.linear_decode(kw.pop("x"), qw.dequant(torch.float32), kw.pop("bias", None), **kw)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert rel_err(got, want) <= BOUND
    assert "Mxfp4Weight" in ops.__all__ and "quantize_mxfp4" in ops.__all__


@pytest.fixture(scope="module", params=["gpt2-tiny", "llama-tiny"])
def quantised(request):
    """(model, tokens, uncached last-position logits of every prefix length of the twin and of the
    unquantised model), computed once."""
    model = _model(request.param)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    sess = DecodeSession(model, B, PROMPT + STEPS, weights="mxfp4")
    assert all(torch.equal(p, before[n]) for n, p in model.named_parameters())  # not modified
    names = [n for n, _ in model.decode_projections()]
    assert list(sess.qweights) == names and "lm_head" in names and sess.weights == "mxfp4"
    assert all(isinstance(q, ops.Mxfp4Weight) and q.shape == p.shape
               for q, (_, p) in zip(sess.qweights.values(), model.decode_projections()))
    assert sess.weight_bytes == sum(p.numel() // 2 + p.numel() // 32 for _, p in model.decode_projections())
    twin = mc.twin_of(model, sess.qweights)
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
def test_mxfp4_session_is_the_twin_model_and_not_the_unquantised_one(quantised, chunks):
    model, toks, want, plain = quantised
    sess = model.decode_session(B, PROMPT + STEPS, weights="mxfp4")
    at = 0
    for n in chunks:
        logits = sess.prefill(toks[:, at:at + n])
        at += n
    assert rel_err(logits, want[PROMPT]) <= BOUND
    assert rel_err(logits, plain[PROMPT]) > BOUND
    for step in range(STEPS):
        n = PROMPT + step
        logits = sess.step(toks[:, n:n + 1])
        for row in range(B):  # every logit row
            e, far = rel_err(logits[row], want[n + 1][row]), rel_err(logits[row], plain[n + 1][row])
            assert e <= BOUND, f"step {step} row {row}: {e:.3e}"
            assert far > BOUND, f"step {step} row {row}: {far:.3e} from the unquantised model"
    print(f"last step: {e:.3e} from the twin, {far:.3e} from the unquantised model")
    sess.reset()
    assert rel_err(sess.prefill(toks[:, :PROMPT]), want[PROMPT]) <= BOUND


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
def test_generate_mxfp4_surface_and_refusals(name):
    model = _model(name)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, model.config.vocab_size, (B, 7), generator=g)
    outs = {}
    for mode in ("fused", "graph"):
        torch.manual_seed(11)
        out = outs[mode] = model.generate(prompt, 6, temperature=0.9, top_k=20, use_cache=mode, weights="mxfp4")
        assert out.shape == (B, 13) and torch.equal(out[:, :7], prompt)
        assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size
    assert torch.equal(outs["fused"], outs["graph"])
    for mode in (False, True):
        with pytest.raises(ValueError, match="weights='mxfp4'"):
            model.generate(prompt, 2, use_cache=mode, weights="mxfp4")
    with pytest.raises(ValueError, match="weights must be 'bf16', 'fp8' or 'mxfp4'"):
        model.generate(prompt, 2, use_cache="fused", weights="fp4")
    with pytest.raises(ValueError, match="weights must be 'bf16', 'fp8' or 'mxfp4'"):
        DecodeSession(model, B, 16, weights="nvfp4")


def test_mxfp4_session_refuses_a_projection_whose_k_is_no_multiple_of_32():
    """down_proj with K = 520: the format has one scale per 32 along K."""
    odd = _model("llama-tiny", ffn_dim=520)
    for graph in (True, False):
        with pytest.raises(ValueError, match="K % 32"):
            DecodeSession(odd, B, 16, graph=graph, weights="mxfp4")
    DecodeSession(odd, B, 16, graph=True)  # the bf16 session is served


def test_sample_script_forwards_decode_weights_mxfp4(monkeypatch, capsys):
    """``sample.py --decode_weights=mxfp4`` reaches ``generate(weights="mxfp4")``."""
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
    sample.main(argv + ["--decode_weights=mxfp4"])
    assert [kw["weights"] for kw in seen] == ["mxfp4"] and seen[0]["use_cache"] == "fused"
    assert capsys.readouterr().out.count("[1, 2,") == 1
    with pytest.raises(ValueError, match="weights='mxfp4'"):
        sample.main(argv[:-1] + ["--decode_weights=mxfp4"])


@pytest.mark.parametrize("norm", mc.NORMS)
@pytest.mark.parametrize("n,k", mc.SHAPES)
def test_ideal_kernel_emulation_has_headroom_in_the_gpu_budget(n, k, norm):
    """An ideal MXFP4 kernel, emulated in fp32 on the cases of the GPU sweep, reaches at most
    0.7 x that sweep's budget (2 x the bf16 baseline's error + 1e-3): the budget can be met with
    room for the summation order, and a real kernel that misses it is wrong."""
    worst = 0.0
    for m in mc.MS:
        for epi in mc.EPIS:
            kw = mc.make_case(m, n, k, norm, epi, seed=m)
            want = mc.composed(kw, torch.float32)
            e = rel_err(mc.ideal_kernel(kw), want)
            b = rel_err(mc.composed(kw, torch.bfloat16), want)
            worst = max(worst, e / (FACTOR * b + FLOOR))
            assert e <= 0.7 * (FACTOR * b + FLOOR), f"M{m} N{n} K{k} {norm} {epi}: {e:.3e} vs baseline {b:.3e}"
    print(f"N{n} K{k} {norm}: worst ideal err / budget {worst:.2f}")

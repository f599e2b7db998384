"""The FP8 skinny decode linear of csrc/linear_decode_fp8.hip on the GPU: every prologue x
epilogue over the edge shapes, against the fp32 composition on the exactly dequantised weight
with the budget of tests/tolerance.py (err(HIP vs fp32) <= 2 x err(stock bf16 PyTorch on the
bf16-rounded dequantised weight vs fp32) + 1e-3), and an all-integer case that must come out bit
for bit.  The cases are drawn on the CPU by tests/fp8_cases.py, whose header states the shapes:
(16, 16), (41, 80), (48, 1104), (130, 256), then N = 48 at K = 64, 128, 256, 512, 2048, 2304,
4096 and those +- 16 (chunks of 64 and rounds of 256 with a prologue; chunks of 128 and rounds
of 512 without; chunks of 256 and rounds of 2048 in the 8-wave form that plain projections take
from K = 2048)."""
import os
import subprocess
import sys

import pytest
import torch

import fp8_cases as fc
from orion_amd import ops
from orion_amd.ops._ext import C
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")


def check(name, kw, got=None):
    got = fc.call(kw) if got is None else got
    want = fc.composed(kw, torch.float32)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    return within_bf16_budget(name, got, want, fc.composed(kw, torch.bfloat16))


@pytest.mark.parametrize("norm", fc.NORMS)
@pytest.mark.parametrize("n,k", fc.SHAPES)
def test_linear_decode_fp8_sweep(n, k, norm):
    worst = 0.0
    for m in fc.MS:
        for epi in fc.EPIS:
            kw = fc.make_case(m, n, k, norm, epi, seed=m, device=DEV)
            assert ops.linear_decode_eligible(kw["x"], kw["weight"])
            e, b = check(f"M{m} N{n} K{k} {norm} {epi}", kw)
            worst = max(worst, e / (2 * b + 1e-3))
    print(f"N{n} K{k} {norm}: worst err / budget {worst:.2f}")


@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("k", [16, 64, 80, 256])
def test_integer_case_is_bit_exact(k, m):
    """Pins the byte and half-word order of the FP8 -> bf16 conversion and the k mapping of the
    A and B fragments: any k paired with a wrong weight changes an integer sum."""
    kw = fc.make_integer_case(m, 41, k, seed=k + m, device=DEV)
    assert ops.linear_decode_eligible(kw["x"], kw["weight"])
    want = fc.composed(kw, torch.float32).to(torch.bfloat16)
    got = fc.call(kw)
    assert torch.equal(got, want), f"{(got.float() - want.float()).abs().max().item()} off"
    # the quantised values are not symmetric in k: a reversed or swapped order would not pass
    flipped = dict(kw, weight=ops.Fp8Weight(kw["weight"].q.flip(1).contiguous(), kw["weight"].scale))
    assert not torch.equal(fc.composed(flipped, torch.float32).to(torch.bfloat16), want)


@pytest.mark.parametrize("f", [24, 40])
@pytest.mark.parametrize("norm", [None, "rms"])
def test_swiglu_packed_gate_up(f, norm):
    """Packed [gate; up] weight of 2F rows -> (M, F); F = 24 and 40 end inside a 16-column tile,
    and row F + n has a scale of its own."""
    for m in (1, 5, 16):
        kw = fc.make_case(m, f, 272, norm, "swiglu", seed=f + m, device=DEV)
        assert kw["weight"].shape == (2 * f, 272)
        y = fc.call(kw)
        assert y.shape == (m, f)
        check(f"swiglu F{f} M{m}", kw, y)


@pytest.mark.parametrize("norm", [None, "layer", "rms"])
def test_strided_and_padded_inputs(norm):
    """Rows beyond M, and the gaps between strided rows, hold NaN: none of it may be read."""
    m, n, k = 5, 41, 144
    kw = fc.make_case(m, n, k, norm, "bias-residual", seed=3, device=DEV)
    want = fc.call(kw)
    check("contiguous", kw, want)
    nan = float("nan")
    buf = torch.full((16, k), nan, device=DEV, dtype=torch.bfloat16)
    buf[:m] = kw["x"]
    rbuf = torch.full((16, n + 7), nan, device=DEV, dtype=torch.bfloat16)  # row stride 48
    rbuf[:m, :n] = kw["residual"]
    wide = torch.full((m, 2 * k), nan, device=DEV, dtype=torch.bfloat16)
    wide[:, :k] = kw["x"]
    h = torch.full((m, 3, k), nan, device=DEV, dtype=torch.bfloat16)  # the model's h[:, -1, :]
    h[:, -1] = kw["x"]
    for name, xs in (("padded", buf[:m]), ("row stride 2K", wide[:, :k]), ("h[:, -1, :]", h[:, -1, :])):
        assert ops.linear_decode_eligible(xs, kw["weight"]), name
        got = fc.call(dict(kw, x=xs, residual=rbuf[:m, :n]))
        assert torch.isfinite(got).all(), name
        assert torch.equal(got, want), name
    assert not h[:, -1, :].is_contiguous() and not rbuf[:m, :n].is_contiguous()


@pytest.mark.parametrize("epi", fc.EPIS)
def test_linear_decode_fp8_is_deterministic(epi):
    kw = fc.make_case(16, 130, 1104, "layer", epi, seed=5, device=DEV)
    assert torch.equal(fc.call(kw), fc.call(kw))


def test_refusals_and_the_ineligible_path():
    raw = C().linear_decode_fp8
    kw = fc.make_case(16, 41, 80, None, "residual", seed=6, device=DEV)
    x, w, r = kw["x"], kw["weight"], kw["residual"]
    q, s = w.q, w.scale
    x17 = torch.cat((x, x[:1]))
    with pytest.raises(RuntimeError, match="M <= 16"):
        raw(x17, q, s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        raw(x[:, :72].contiguous(), q[:, :72].contiguous(), s, None, 0, None, None, 1e-5, 0, None, None)
    assert not ops.linear_decode_eligible(x[:, :72].contiguous(), ops.Fp8Weight(q[:, :72].contiguous(), s))
    for other in (torch.float8_e5m2, torch.float8_e4m3fnuz):
        with pytest.raises(RuntimeError, match="Float8_e4m3fn"):
            raw(x, q.view(other), s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="bfloat16"):
        raw(x.float(), q, s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s.to(torch.bfloat16), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s[:-1].contiguous(), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, torch.cat((s, s))[::2], None, 0, None, None, 1e-5, 0, None, None)
    before = r.clone()
    with pytest.raises(RuntimeError, match="aliases the output"):
        raw(x, q, s, None, 0, None, None, 1e-5, 0, r, r)
    assert torch.equal(r, before)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.linear_decode(x.clone().requires_grad_(), w)
    # 17 rows: the plain ops composed on the dequantised weight, never a wrong result
    for norm, epi in (("layer", "bias-gelu"), ("rms", "swiglu"), (None, "bias-residual")):
        kw = fc.make_case(16, 48, 256, norm, epi, seed=7, device=DEV)
        kw["x"] = torch.cat((kw["x"], kw["x"][:1]))
        if "residual" in kw:
            kw["residual"] = torch.cat((kw["residual"], kw["residual"][:1]))
        assert not ops.linear_decode_eligible(kw["x"], kw["weight"])
        check(f"M 17 {norm} {epi}", kw)
    out = torch.empty(16, 41, device=DEV, dtype=torch.bfloat16)
    kw = fc.make_case(16, 41, 80, "rms", "bias", seed=9, device=DEV)
    assert torch.equal(fc.call(dict(kw, out=out)), fc.call(kw)) and torch.equal(out, fc.call(kw))


DEBUG_SCRIPT = r"""
import torch
from orion_amd.ops._ext import C, load_ext, EXT_PATH
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
load_ext(required=True)
op = C().linear_decode_fp8
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
for m in (1, 5, 16):
    for n, k in %r:
        x, res = r(16, k)[:m], r(m, n)
        for norm in (0, 1, 2):
            nw, nb = (r(k) if norm else None), (r(k) if norm == 1 else None)
            for act in (0, 1, 2):
                rows = 2 * n if act == 2 else n
                q = r(rows, k).float().to(torch.float8_e4m3fn)
                s = torch.rand(rows, device="cuda", generator=g) + 0.5
                y = op(x, q, s, r(rows), norm, nw, nb, 1e-5, act, res, None)
        assert y.shape == (m, n)
torch.cuda.synchronize()
assert torch.isfinite(y).all()
print("debug build ok")
""" % (fc.SMALL_SHAPES,)


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_linear_decode_fp8_passes_its_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

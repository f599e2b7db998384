"""The MXFP4 skinny decode linear of csrc/linear_decode_mxfp4.hip on the GPU: all 256 code bytes
decoded value for value, an all-integer case that must come out bit for bit, and every prologue x
epilogue over the edge shapes against the fp32 composition on the exactly dequantised weight with
the budget of tests/tolerance.py (err(HIP vs fp32) <= 2 x err(stock bf16 PyTorch on the dequantised
weight vs fp32) + 1e-3).  The cases are drawn on the CPU by tests/mxfp4_cases.py, whose header
states the shapes: (16, 32), (41, 96), (48, 1120), (130, 256), then N = 48 at K = 128, 256, 512,
2048, 2304, 4096 and those +- 32 (chunks of 128 and rounds of 512 in the 4-wave form; chunks of
256 and rounds of 2048 in the 8-wave form that plain projections take from K = 2048)."""
import os
import subprocess
import sys

import pytest
import torch

import mxfp4_cases as mc
from orion_amd import ops
from orion_amd.ops._ext import C
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def check(name, kw, got=None):
    got = mc.call(kw) if got is None else got
    want = mc.composed(kw, torch.float32)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    return within_bf16_budget(name, got, want, mc.composed(kw, torch.bfloat16))


def test_all_256_code_bytes():
    """Row n of the weight is byte n repeated, x row 0 selects the even k (low nibbles) and row 1
    the odd k (high nibbles): y[0, n] = 16 lo(n) 2^(s - 127) and y[1, n] = 16 hi(n) 2^(s - 127),
    every one a bf16 value, so equality is exact.  Pins the decoding of every code, the nibble
    order and the byte order within a word.  (A zero's sign is the accumulator's and is not
    compared: 16 x -0 summed from +0 is +0.)"""
    n, k = 256, 32
    q = torch.arange(n, dtype=torch.uint8).view(n, 1).repeat(1, k // 2)
    s = (120 + torch.arange(n) % 16).to(torch.uint8).view(n, 1)
    x = torch.zeros(2, k)
    x[0, 0::2] = 1
    x[1, 1::2] = 1
    w = ops.Mxfp4Weight(q.to(DEV), s.to(DEV))
    assert ops.linear_decode_eligible(x.to(DEV).to(torch.bfloat16), w)
    got = ops.linear_decode(x.to(DEV).to(torch.bfloat16), w).float().cpu()

    def val(code):
        return (-1.0 if code & 8 else 1.0) * E2M1[code & 7]

    want = torch.tensor([[16 * val(b & 15) * 2.0 ** (int(s[b]) - 127) for b in range(n)],
                         [16 * val(b >> 4) * 2.0 ** (int(s[b]) - 127) for b in range(n)]])
    assert torch.equal(want.to(torch.bfloat16).float(), want)  # representable
    bad = (got != want).nonzero().tolist()
    assert not bad, f"(row, byte) {bad[:8]}: got {[got[i, j].item() for i, j in bad[:8]]}, " \
                    f"want {[want[i, j].item() for i, j in bad[:8]]}"


@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("k", [32, 64, 96, 256])
def test_integer_case_is_bit_exact(k, m):
    """Pins the k mapping of the A and B fragments and the pairing of a block with its scale: any
    k paired with a wrong weight or a wrong scale changes an exact sum."""
    kw = mc.make_integer_case(m, 41, k, seed=k + m, device=DEV)
    assert ops.linear_decode_eligible(kw["x"], kw["weight"])
    want = mc.composed(kw, torch.float32).to(torch.bfloat16)
    got = mc.call(kw)
    assert torch.equal(got, want), f"{(got.float() - want.float()).abs().max().item()} off"
    # the codes are not symmetric in k, and the scales differ between the blocks of a row: a
    # reversed order, or a scale paired with another block, would not pass
    w = kw["weight"]
    flipped = dict(kw, weight=ops.Mxfp4Weight(w.q.flip(1).contiguous(), w.scale))
    assert not torch.equal(mc.composed(flipped, torch.float32).to(torch.bfloat16), want)
    if k > 32:
        rolled = dict(kw, weight=ops.Mxfp4Weight(w.q, w.scale.roll(1, dims=1).contiguous()))
        assert not torch.equal(mc.composed(rolled, torch.float32).to(torch.bfloat16), want)


@pytest.mark.parametrize("norm", mc.NORMS)
@pytest.mark.parametrize("n,k", mc.SHAPES)
def test_linear_decode_mxfp4_sweep(n, k, norm):
    worst = 0.0
    for m in mc.MS:
        for epi in mc.EPIS:
            kw = mc.make_case(m, n, k, norm, epi, seed=m, device=DEV)
            assert ops.linear_decode_eligible(kw["x"], kw["weight"])
            e, b = check(f"M{m} N{n} K{k} {norm} {epi}", kw)
            worst = max(worst, e / (2 * b + 1e-3))
    print(f"N{n} K{k} {norm}: worst err / budget {worst:.2f}")


@pytest.mark.parametrize("f", [24, 40])
@pytest.mark.parametrize("norm", [None, "rms"])
def test_swiglu_packed_gate_up(f, norm):
    """Packed [gate; up] weight of 2F rows -> (M, F); F = 24 and 40 end inside a 16-column tile,
    and row F + n has codes and scales of its own."""
    for m in (1, 5, 16):
        kw = mc.make_case(m, f, 288, norm, "swiglu", seed=f + m, device=DEV)
        assert kw["weight"].shape == (2 * f, 288)
        y = mc.call(kw)
        assert y.shape == (m, f)
        check(f"swiglu F{f} M{m}", kw, y)


@pytest.mark.parametrize("norm", [None, "layer", "rms"])
def test_strided_and_padded_inputs(norm):
    """Rows beyond M, and the gaps between strided rows, hold NaN: none of it may be read."""
    m, n, k = 5, 41, 160
    kw = mc.make_case(m, n, k, norm, "bias-residual", seed=3, device=DEV)
    want = mc.call(kw)
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
        got = mc.call(dict(kw, x=xs, residual=rbuf[:m, :n]))
        assert torch.isfinite(got).all(), name
        assert torch.equal(got, want), name
    assert not h[:, -1, :].is_contiguous() and not rbuf[:m, :n].is_contiguous()


@pytest.mark.parametrize("epi", mc.EPIS)
def test_linear_decode_mxfp4_is_deterministic(epi):
    kw = mc.make_case(16, 130, 1120, "layer", epi, seed=5, device=DEV)
    assert torch.equal(mc.call(kw), mc.call(kw))


def test_refusals_and_the_ineligible_path():
    raw = C().linear_decode_mxfp4
    kw = mc.make_case(16, 41, 96, None, "residual", seed=6, device=DEV)
    x, w, r = kw["x"], kw["weight"], kw["residual"]
    q, s = w.q, w.scale
    x17 = torch.cat((x, x[:1]))
    with pytest.raises(RuntimeError, match="M <= 16"):
        raw(x17, q, s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        raw(x[:, :80].contiguous(), q[:, :40].contiguous(), s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="uint8"):
        raw(x, q.view(torch.int8), s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="uint8"):
        raw(x, q.view(torch.float8_e4m3fn), s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="bfloat16"):
        raw(x.float(), q, s, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s.view(torch.int8), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s.float(), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s[:, :2].contiguous(), None, 0, None, None, 1e-5, 0, None, None)  # wrong shape
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, s[:-1].contiguous(), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="w_scale"):
        raw(x, q, torch.cat((s, s), dim=1)[:, ::2], None, 0, None, None, 1e-5, 0, None, None)  # not contiguous
    before = r.clone()
    with pytest.raises(RuntimeError, match="aliases the output"):
        raw(x, q, s, None, 0, None, None, 1e-5, 0, r, r)
    assert torch.equal(r, before)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.linear_decode(x.clone().requires_grad_(), w)
    # 17 rows: the plain ops composed on the dequantised weight, never a wrong result
    for norm, epi in (("layer", "bias-gelu"), ("rms", "swiglu"), (None, "bias-residual")):
        kw = mc.make_case(16, 48, 256, norm, epi, seed=7, device=DEV)
        kw["x"] = torch.cat((kw["x"], kw["x"][:1]))
        if "residual" in kw:
            kw["residual"] = torch.cat((kw["residual"], kw["residual"][:1]))
        assert not ops.linear_decode_eligible(kw["x"], kw["weight"])
        check(f"M 17 {norm} {epi}", kw)
    out = torch.empty(16, 41, device=DEV, dtype=torch.bfloat16)
    kw = mc.make_case(16, 41, 96, "rms", "bias", seed=9, device=DEV)
    assert torch.equal(mc.call(dict(kw, out=out)), mc.call(kw)) and torch.equal(out, mc.call(kw))


DEBUG_SCRIPT = r"""
import torch
from orion_amd.ops._ext import C, load_ext, EXT_PATH
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
load_ext(required=True)
op = C().linear_decode_mxfp4
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
u8 = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device="cuda", generator=g).to(torch.uint8)
for m in (1, 5, 16):
    for n, k in %r:
        x, res = r(16, k)[:m], r(m, n)
        for norm in (0, 1, 2):
            nw, nb = (r(k) if norm else None), (r(k) if norm == 1 else None)
            for act in (0, 1, 2):
                rows = 2 * n if act == 2 else n
                y = op(x, u8(0, 255, rows, k // 2), u8(120, 126, rows, k // 32), r(rows), norm, nw, nb, 1e-5, act,
                       res, None)
        assert y.shape == (m, n)
torch.cuda.synchronize()
assert torch.isfinite(y).all()
print("debug build ok")
""" % (mc.SMALL_SHAPES,)


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_linear_decode_mxfp4_passes_its_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

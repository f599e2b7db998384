"""The skinny decode linear of csrc/linear_decode.hip on the GPU: every prologue x epilogue over
the edge shapes, against the fp32 reference on fp32 copies of the bf16 inputs with the budget of
tests/tolerance.py (err(HIP vs fp32) <= 2 x err(stock bf16 PyTorch vs fp32) + 1e-3; the baseline
is the same composition on stock bf16 torch ops)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from orion_amd import ops
from orion_amd.ops._ext import C
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")

MS = [1, 2, 5, 8, 16]
# a K shorter than one round of the wave split; an odd N with a masked last tile; a K with a
# remainder after several rounds; more than one full tile plus a tail.  Then the kernel's own
# boundaries +- 8: a wave takes chunks of 128 elements and the four waves a round of 512; a plain
# projection (no prologue, no activation) with K >= 2048 takes chunks of 256 and rounds of 2048.
# The boundary shapes have N = 48, three tiles: the budget compares two relative errors, and on
# the 16 values of an M = 1, N = 16 output an ideal fused kernel emulated with stock fp32 ops on
# the CPU (normalised x rounded to bf16, fp32 accumulation, one rounding at the store) reaches
# 0.92 - 1.15 x the budget in 1 of 400 random draws, which thousands of cases would hit; at 48
# values the worst of 400 draws is 0.66 x.
SHAPES = [(16, 32), (41, 72), (48, 1096), (130, 256),
          (48, 120), (48, 128), (48, 136), (48, 504), (48, 512), (48, 520),
          (48, 2040), (48, 2048), (48, 2056), (48, 2296), (48, 2304), (48, 2312), (48, 4088), (48, 4096), (48, 4104)]
NORMS = [None, "layer", "layer-nobeta", "rms"]
EPIS = ["none", "bias", "gelu", "bias-gelu", "residual", "bias-residual", "swiglu", "bias-swiglu"]


def make_case(m, n, k, norm, epi, seed=0):
    """bf16 keyword arguments of ops.linear_decode for one case."""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def r(*s):
        return torch.randn(*s, device=DEV, generator=g)

    rows = 2 * n if "swiglu" in epi else n
    kw = dict(x=r(m, k), weight=r(rows, k) * k ** -0.5)
    if norm is not None:
        kw.update(norm=norm.split("-")[0], norm_weight=1 + 0.1 * r(k), eps=1e-5)
        if norm == "layer":
            kw["norm_bias"] = 0.1 * r(k)
    if "bias" in epi:
        kw["bias"] = r(rows)
    if "gelu" in epi:
        kw["act"] = "gelu"
    if "swiglu" in epi:
        kw["act"] = "swiglu"
    if "residual" in epi:
        kw["residual"] = r(m, n)
    return {a: v.to(torch.bfloat16) if torch.is_tensor(v) else v for a, v in kw.items()}


def composed(kw, dtype):
    """The unfused composition on stock torch ops in ``dtype``: fp32 is the reference, bf16 (every
    op rounding its output, as the unfused path does) the baseline."""
    def t(name):
        v = kw.get(name)
        return None if v is None else v.to(dtype)

    h = t("x")
    K = h.shape[-1]
    if kw.get("norm") == "layer":
        h = F.layer_norm(h, (K,), t("norm_weight"), t("norm_bias"), kw["eps"])
    elif kw.get("norm") == "rms":
        hf = h.float()
        h = (hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + kw["eps"])).to(dtype) * t("norm_weight")
    y = F.linear(h, t("weight"), t("bias"))
    if kw.get("act") == "gelu":
        y = F.gelu(y, approximate="tanh")
    elif kw.get("act") == "swiglu":
        gate, up = y.chunk(2, dim=-1)
        y = F.silu(gate) * up
    return y if kw.get("residual") is None else y + t("residual")


def call(kw):
    kw = dict(kw)
    return ops.linear_decode(kw.pop("x"), kw.pop("weight"), kw.pop("bias", None), **kw)


def check(name, kw, got=None):
    got = call(kw) if got is None else got
    want = composed(kw, torch.float32)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    return within_bf16_budget(name, got, want, composed(kw, torch.bfloat16))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_linear_decode_sweep(n, k, norm):
    worst = 0.0
    for m in MS:
        for epi in EPIS:
            kw = make_case(m, n, k, norm, epi, seed=m)
            assert ops.linear_decode_eligible(kw["x"], kw["weight"])
            e, b = check(f"M{m} N{n} K{k} {norm} {epi}", kw)
            worst = max(worst, e / (2 * b + 1e-3))
    print(f"N{n} K{k} {norm}: worst err / budget {worst:.2f}")


@pytest.mark.parametrize("f", [24, 40])
@pytest.mark.parametrize("norm", [None, "rms"])
def test_swiglu_packed_gate_up(f, norm):
    """Packed [gate; up] weight of 2F rows -> (M, F); F = 24 and 40 end inside a 16-column tile."""
    for m in (1, 5, 16):
        kw = make_case(m, f, 264, norm, "swiglu", seed=f + m)
        assert kw["weight"].shape == (2 * f, 264)
        y = call(kw)
        assert y.shape == (m, f)
        check(f"swiglu F{f} M{m}", kw, y)


@pytest.mark.parametrize("norm", [None, "layer", "rms"])
def test_strided_and_padded_inputs(norm):
    """Rows beyond M, and the gaps between strided rows, hold NaN: none of it may be read."""
    m, n, k = 5, 41, 136
    kw = make_case(m, n, k, norm, "bias-residual", seed=3)
    want = call(kw)
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
        got = call(dict(kw, x=xs, residual=rbuf[:m, :n]))
        assert torch.isfinite(got).all(), name
        assert torch.equal(got, want), name
    assert not h[:, -1, :].is_contiguous() and not rbuf[:m, :n].is_contiguous()


@pytest.mark.parametrize("epi", EPIS)
def test_linear_decode_is_deterministic(epi):
    kw = make_case(16, 130, 1096, "layer", epi, seed=5)
    assert torch.equal(call(kw), call(kw))


def test_refusals_and_the_ineligible_path():
    raw = C().linear_decode
    kw = make_case(16, 41, 72, None, "residual", seed=6)
    x, w, r = kw["x"], kw["weight"], kw["residual"]
    x17 = torch.cat((x, x[:1]))
    with pytest.raises(RuntimeError, match="M <= 16"):
        raw(x17, w, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="bfloat16"):
        raw(x.float(), w, None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        raw(x[:, :60].contiguous(), w[:, :60].contiguous(), None, 0, None, None, 1e-5, 0, None, None)
    with pytest.raises(RuntimeError, match="misaligned"):
        raw(torch.zeros(4, 81, device=DEV, dtype=torch.bfloat16)[:, :72], w, None, 0, None, None, 1e-5, 0, None, None)
    before = r.clone()
    with pytest.raises(RuntimeError, match="aliases the output"):
        raw(x, w, None, 0, None, None, 1e-5, 0, r, r)
    assert torch.equal(r, before)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.linear_decode(x.clone().requires_grad_(), w)
    # 17 rows: the plain ops composed, never a wrong result
    for norm, epi in (("layer", "bias-gelu"), ("rms", "swiglu"), (None, "bias-residual")):
        kw = make_case(16, 48, 256, norm, epi, seed=7)
        kw["x"] = torch.cat((kw["x"], kw["x"][:1]))
        if "residual" in kw:
            kw["residual"] = torch.cat((kw["residual"], kw["residual"][:1]))
        assert not ops.linear_decode_eligible(kw["x"], kw["weight"])
        check(f"M 17 {norm} {epi}", kw)
    out = torch.empty(16, 41, device=DEV, dtype=torch.bfloat16)
    kw = make_case(16, 41, 72, "rms", "bias", seed=9)
    assert torch.equal(call(dict(kw, out=out)), call(kw)) and torch.equal(out, call(kw))


DEBUG_SCRIPT = r"""
import torch
from orion_amd.ops._ext import C, load_ext, EXT_PATH
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
load_ext(required=True)
op = C().linear_decode
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
for m in (1, 5, 16):
    for n, k in ((16, 32), (41, 72), (48, 1096), (130, 256), (16, 120), (24, 520), (16, 2040), (24, 2056), (16, 4104)):
        x, res = r(16, k)[:m], r(m, n)
        for norm in (0, 1, 2):
            nw, nb = (r(k) if norm else None), (r(k) if norm == 1 else None)
            for act in (0, 1, 2):
                w = r(2 * n if act == 2 else n, k)
                y = op(x, w, r(w.shape[0]), norm, nw, nb, 1e-5, act, res, None)
        assert y.shape == (m, n)
torch.cuda.synchronize()
assert torch.isfinite(y).all()
print("debug build ok")
"""


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_linear_decode_passes_its_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

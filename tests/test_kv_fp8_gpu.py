"""The FP8 key/value cache kernels of csrc/attn_decode.hip on the GPU: single-query attention
over e4m3 bytes with per-(token, head) scales and the quantising append.  Attention is held to the
budget of tests/tolerance.py against the fp32 reference on the exactly dequantised cache (the
baseline: SDPA in bf16 on that cache rounded to bf16), so only the kernel's own arithmetic is
judged: the quantisation error is in the reference too.  Inputs come from tests/kv_fp8_cases.py."""
import os
import subprocess
import sys

import pytest
import torch

import kv_fp8_cases as kc
from orion_amd import ops
from orion_amd.ops import reference as ref
from orion_amd.ops.decode import attention_decode_fp8_tile, attention_decode_torch
from tolerance import FACTOR, FLOOR, rel_err, within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")

HEADS = [(4, 4), (8, 2), (16, 2), (12, 1)]  # G = 1, 4, 8 and 12 (the 8-row group loops)


def _shape(D):
    """(Tmax, lengths) of the sweep: two key tiles and a part of a third; one key, one short of a
    tile, one past it, and 20 short of Tmax."""
    tile = attention_decode_fp8_tile(D)
    tmax = 2 * tile + 64
    return tmax, [1, tile - 1, tile + 1, tmax - 20]


def _call(c, splits=0, **over):
    a = dict(c, **over)
    return ops.attention_decode(a["q"], a["kc"], a["vc"], a["lens"], splits=splits, k_scale=a["ks"], v_scale=a["vs"])


_CASES = {}


def _case(D, Hq, Hkv):
    """Inputs, fp32 reference and SDPA-bf16 baseline of one sweep shape, computed once."""
    key = (D, Hq, Hkv)
    if key not in _CASES:
        tmax, lens = _shape(D)
        c = kc.decode_case(D, Hq, Hkv, lens, tmax, device=DEV)
        k32, v32 = kc.dequantized(c)
        want = ref.attention_decode(c["q"].float(), k32, v32, c["lens"])
        base = attention_decode_torch(c["q"], k32.to(torch.bfloat16), v32.to(torch.bfloat16), c["lens"])
        _CASES[key] = (c, want, base)
    return _CASES[key]


def test_the_sweep_shapes_fit_their_bound():
    assert attention_decode_fp8_tile(64) == 128 and attention_decode_fp8_tile(128) == 64
    assert _shape(64) == (320, [1, 127, 129, 300]) and _shape(128) == (192, [1, 63, 65, 172])


@pytest.mark.parametrize("splits", [0, 1, 3, 8])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_sweep(D, Hq, Hkv, splits):
    """Ragged lengths with 0x7F bytes and NaN scales beyond them; 8 splits leave rows with empty splits."""
    c, want, base = _case(D, Hq, Hkv)
    o = _call(c, splits)
    assert o.shape == (4, Hq, D) and o.dtype == torch.bfloat16
    assert torch.isfinite(o).all()
    e, b = rel_err(o, want), rel_err(base, want)
    print(f"D{D} H{Hq}/{Hkv} splits {splits}: err {e:.3e} baseline {b:.3e}")
    within_bf16_budget("o", o, want, base)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
def test_one_hot_selection_is_bit_exact(D, splits):
    """Pins the byte order of the conversions and the lane-to-column mapping: the output is one
    row of the dequantised v, exactly."""
    c, j = kc.one_hot_case(D, device=DEV)
    want = kc.one_hot_expected(c, j)
    o = _call(c, splits)
    assert torch.equal(o, want), f"{(o.float() - want.float()).abs().max().item()} off"
    # neither the keys nor the values are symmetric in d: a reversed byte order would not pass
    flipped_v = dict(c, vc=c["vc"].flip(-1).contiguous())
    assert not torch.equal(kc.one_hot_expected(flipped_v, j), want)
    assert not torch.equal(kc.one_hot_expected(c, (D - 1) - j), want)  # the keys' order reversed
    for g in (4, 8):  # reversed inside each word / each lane's 8 bytes
        jr = (j // g) * g + (g - 1 - j % g)
        assert not torch.equal(kc.one_hot_expected(c, jr), want)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 1), (16, 1)])  # 1 row, one full pass of 8, two passes
@pytest.mark.parametrize("D", [64, 128])
def test_unit_scale_fp8_cache_equals_the_bf16_kernel(D, Hq, Hkv, splits):
    """The two cache types run one kernel body: e4m3 values are bf16 values, so on the widened cache
    the bf16 kernel sees the same K and V, and (d * 1) * scale and fma(p * 1, v, acc) are its own
    operations."""
    tmax, tile = 384, attention_decode_fp8_tile(D)
    g = torch.Generator().manual_seed(D + Hq)
    q = torch.randn(2, Hq, D, generator=g).to(torch.bfloat16).to(DEV)
    k8 = torch.randn(2, tmax, Hkv, D, generator=g).to(torch.float8_e4m3fn).to(DEV)
    v8 = torch.randn(2, tmax, Hkv, D, generator=g).to(torch.float8_e4m3fn).to(DEV)
    assert torch.equal(k8.to(torch.bfloat16).float(), k8.float())  # the widening is exact
    lens = torch.tensor([tile + 3, 37], dtype=torch.int32, device=DEV)
    one = torch.ones(2, Hkv, tmax, device=DEV)
    want = ops.attention_decode(q, k8.to(torch.bfloat16), v8.to(torch.bfloat16), lens, splits=splits)
    got = ops.attention_decode(q, k8, v8, lens, splits=splits, k_scale=one, v_scale=one)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, want), f"{(got.float() - want.float()).abs().max().item()} off"


@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 4), (128, 8, 2)])
def test_decode_strided_inputs(D, Hq, Hkv):
    """k / v bytes and scales as views into one cache buffer each, q a view of a packed projection."""
    c, want, base = _case(D, Hq, Hkv)
    B, tmax = c["q"].shape[0], c["kc"].shape[1]
    kv = torch.stack((c["kc"], c["vc"]), dim=2)       # (B, Tmax, 2, Hkv, D)
    sc = torch.stack((c["ks"], c["vs"]), dim=1)       # (B, 2, Hkv, Tmax)
    wide = torch.full((B, 2, Hkv, tmax + 24), float("nan"), device=DEV)
    wide[..., :tmax] = sc                             # a row stride that is not Tmax
    packed = torch.randn(B, 1, Hq + 2 * Hkv, D, device=DEV).to(torch.bfloat16)
    packed[:, 0, :Hq] = c["q"]
    s = dict(q=packed[:, 0, :Hq], kc=kv[:, :, 0], vc=kv[:, :, 1], ks=wide[:, 0, :, :tmax], vs=wide[:, 1, :, :tmax])
    assert not s["kc"].is_contiguous() and not s["ks"].is_contiguous() and s["q"].stride(0) != Hq * D
    for splits in (1, 3):
        o = _call(c, splits, **s)
        within_bf16_budget("o strided", o, want, base)
        assert torch.equal(o, _call(c, splits))


@pytest.mark.parametrize("splits", [0, 1, 3])
def test_decode_length_edges(splits):
    D, Hq, Hkv = 64, 8, 2
    tmax = _shape(D)[0]
    c = kc.decode_case(D, Hq, Hkv, [tmax] * 3, tmax, seed=2, device=DEV)
    zero = torch.zeros(3, dtype=torch.int32, device=DEV)
    assert torch.all(_call(c, splits, lens=zero) == 0), "length 0 must give zeros"
    over = torch.tensor([tmax + 1, tmax + 1000, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    full = _call(c, splits)
    assert torch.equal(_call(c, splits, lens=over), full)
    assert torch.equal(_call(c, splits), full), "two calls are bit-equal"


def test_decode_refuses_bad_inputs():
    c, _, _ = _case(64, 4, 4)
    with pytest.raises((RuntimeError, ValueError)):  # bytes of another type
        ops.attention_decode(c["q"], c["kc"].view(torch.float8_e5m2), c["vc"].view(torch.float8_e5m2), c["lens"],
                             k_scale=c["ks"], v_scale=c["vs"])
    with pytest.raises(RuntimeError):  # scales of another type
        _call(c, ks=c["ks"].double())
    with pytest.raises(ValueError):
        ops.attention_decode(c["q"], c["kc"], c["vc"], c["lens"])
    with pytest.raises(ValueError):
        ops.attention_decode(c["q"], c["kc"], c["vc"], c["lens"], k_scale=c["ks"])
    with pytest.raises(RuntimeError):  # D 32
        _call(c, q=c["q"][..., :32], kc=c["kc"][..., :32], vc=c["vc"][..., :32])
    with pytest.raises(RuntimeError):
        _call(c, lens=c["lens"].cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        _call(c, q=c["q"].clone().requires_grad_())
    with pytest.raises(ValueError):  # a bf16 cache with scales
        ops.attention_decode(c["q"], c["kc"].to(torch.bfloat16), c["vc"].to(torch.bfloat16), c["lens"],
                             k_scale=c["ks"], v_scale=c["vs"])


@pytest.mark.parametrize("with_rope", [False, True], ids=["copy", "rope"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5])
def test_kv_append(T, D, with_rope):
    """Strided k / v / q views of a packed projection, ragged lengths, one row running past Tmax;
    sentinel bytes and scales wherever nothing is appended."""
    tmax = 24
    a = kc.append_case(T, D, tmax=tmax, device=DEV)
    cos, sin = ref.rope_tables(tmax + 8, D, device=DEV)
    kw = dict(q=a["q"], cos=cos, sin=sin) if with_rope else {}
    q_rot = ops.kv_append(a["k_new"], a["v_new"], a["kc"], a["vc"], a["lens"], k_scale=a["ks"], v_scale=a["vs"], **kw)
    assert a["lens"].tolist() == a["lens_h"]
    for b, p0 in enumerate(a["lens_h"]):
        n = max(0, min(T, tmax - p0))
        outside = torch.ones(tmax, dtype=torch.bool, device=DEV)
        outside[p0:p0 + n] = False
        for cache, sc in ((a["kc"], a["ks"]), (a["vc"], a["vs"])):
            assert torch.all(kc.as_bytes(cache)[b, outside] == kc.SENT_BYTE)
            assert torch.all(sc[b][:, outside] == kc.SENT_SCALE)
        if n == 0:
            continue
        wq, ws = ops.quantize_kv_fp8(a["v_new"][b, :n])
        assert torch.equal(kc.as_bytes(a["vc"])[b, p0:p0 + n], kc.as_bytes(wq)), "v bytes"
        assert torch.equal(a["vs"][b][:, p0:p0 + n], ws.t()), "v scales"
        got_b, got_s = a["kc"][b, p0:p0 + n], a["ks"][b][:, p0:p0 + n]
        if not with_rope:
            wq, ws = ops.quantize_kv_fp8(a["k_new"][b, :n])
            assert torch.equal(kc.as_bytes(got_b), kc.as_bytes(wq)), "k bytes"
            assert torch.equal(got_s, ws.t()), "k scales"
            continue
        # the rotation's FMA contraction may differ from torch's: no bit equality, but every row is
        # at full scale and as close to the fp32 rotated k as the reference quantisation of it is
        assert torch.all(got_b.float().abs().amax(-1) == 448.0)
        k32 = ref.rope(a["k_new"][b:b + 1, :n].float(), cos[p0:], sin[p0:])[0]
        wq, ws = ops.quantize_kv_fp8(k32)
        e = rel_err(got_b.float() * got_s.t()[..., None], k32)
        r = rel_err(wq.float() * ws[..., None], k32)
        print(f"T{T} D{D} row {b}: k err {e:.3e} reference quantisation {r:.3e}")
        assert e <= FACTOR * r + FLOOR
    if with_rope:
        plain = torch.zeros(3, tmax, 2, D, dtype=torch.bfloat16, device=DEV)
        want_q = ops.kv_append(a["k_new"], a["v_new"], plain, plain.clone(), a["lens"], q=a["q"], cos=cos, sin=sin)
        assert q_rot.shape == want_q.shape and q_rot.is_contiguous()
        assert torch.equal(q_rot, want_q), "the rotated q is the bf16 append's"
    else:
        assert q_rot is None


def test_append_refuses_bad_inputs():
    a = kc.append_case(1, 64, device=DEV)
    with pytest.raises(ValueError):
        ops.kv_append(a["k_new"], a["v_new"], a["kc"], a["vc"], a["lens"])
    with pytest.raises(RuntimeError):  # scales (B, Tmax, Hkv) passed as a transposed view: tokens not innermost
        ops.kv_append(a["k_new"], a["v_new"], a["kc"], a["vc"], a["lens"],
                      k_scale=a["ks"].transpose(1, 2).contiguous().transpose(1, 2), v_scale=a["vs"])
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.kv_append(a["k_new"].clone().requires_grad_(), a["v_new"], a["kc"], a["vc"], a["lens"],
                      k_scale=a["ks"], v_scale=a["vs"])


DEBUG_SCRIPT = r"""
import math, sys, torch
sys.path.insert(0, "tests")
import kv_fp8_cases as kc
from orion_amd.ops._ext import C, load_ext, EXT_PATH
from orion_amd.ops.reference import rope_tables
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
load_ext(required=True)
ops = C()
a = kc.append_case(5, 128, Hq=12, Hkv=1, device="cuda")
cos, sin = rope_tables(32, 128, device="cuda")
ops.kv_append_fp8(a["k_new"], a["v_new"], a["kc"], a["vc"], a["ks"], a["vs"], a["lens"], a["q"], cos, sin)
ops.kv_append_fp8(a["k_new"], a["v_new"], a["kc"], a["vc"], a["ks"], a["vs"], a["lens"], None, None, None)
c = kc.decode_case(64, 4, 4, [1, 127, 129, 300], 320, device="cuda")  # the sweep's D 64 case
for splits in (0, 1, 3):
    o = ops.attn_decode_fp8(c["q"], c["kc"], c["vc"], c["ks"], c["vs"], c["lens"], 1 / math.sqrt(64), splits)
torch.cuda.synchronize()
assert torch.isfinite(o).all()
print("debug build ok")
"""


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_fp8_cache_kernels_pass_their_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

"""Multi-query decode attention (csrc/attn_decode.hip) on the GPU: bit-equality with the
single-query kernel per query, the bf16 budget against the fp32 reference, NaN beyond the
lengths, determinism and the refusal of an FP8 cache.

The key tile is 128 keys at D = 64 and 64 at D = 128; with Tmax = 384, splits = 3 cuts at 128 and
256 for both, and splits = 0 plans one tile per split.  Each case runs three pairs of lengths:
the cache empty before the step beside kv_lens = 2 (< Tq: the early queries have no keys), the
window of Tq bounds straddling the first tile boundary beside one straddling the split boundary at
256, and kv_lens just beyond Tmax (clamped, the last bounds saturate) beside an ordinary length."""
import pytest
import torch

from orion_amd import ops
from orion_amd.ops import reference as ref
from orion_amd.ops.decode import attention_decode_multi_torch
from tolerance import within_bf16_budget, within_bf16_budget_slices

pytestmark = pytest.mark.gpu
DEV = "cuda"
TMAX = 384
HEADS = [(2, 2), (4, 2), (8, 1), (16, 1)]  # rows per KV head at Tq = 1: 1, 2, 8 (a full pass), 16 (two)
TQS = [1, 2, 5, 8, 16]


def _lens(D, Tq):
    tile, half = (128 if D == 64 else 64), (Tq + 1) // 2
    return [[Tq, 2], [tile + half, 256 + half], [TMAX + 2, 37]]


_INPUTS = {}


def _inputs(D, Hq, Hkv, Tq):
    """q and NaN-free caches of one shape, made once and never modified."""
    key = (D, Hq, Hkv, Tq)
    if key not in _INPUTS:
        g = torch.Generator(device=DEV).manual_seed(D + Hq + 3 * Tq)
        q = torch.randn(2, Tq, Hq, D, device=DEV, generator=g).to(torch.bfloat16)
        kc = torch.randn(2, TMAX, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
        vc = torch.randn(2, TMAX, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
        _INPUTS[key] = (q, kc, vc)
    return _INPUTS[key]


_REFS = {}


def _reference(D, Hq, Hkv, Tq, lens):
    """(fp32 reference, SDPA-bf16 baseline) of one shape and pair of lengths, computed once."""
    key = (D, Hq, Hkv, Tq, tuple(lens))
    if key not in _REFS:
        q, kc, vc = _inputs(D, Hq, Hkv, Tq)
        kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
        _REFS[key] = (ref.attention_decode_multi(q.float(), kc.float(), vc.float(), kv),
                      attention_decode_multi_torch(q, kc, vc, kv))
    return _REFS[key]


@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("Tq", TQS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_multi_query_sweep(D, Hq, Hkv, Tq, splits):
    q, kc, vc = _inputs(D, Hq, Hkv, Tq)
    for lens in _lens(D, Tq):
        kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
        o = ops.attention_decode_multi(q, kc, vc, kv, splits=splits)
        assert o.shape == (2, Tq, Hq, D) and o.dtype == torch.bfloat16
        assert torch.isfinite(o).all()
        # (i) every query is the single-query kernel on its own length, bit for bit
        for t in range(Tq):
            one = ops.attention_decode(q[:, t], kc, vc, kv - (Tq - 1 - t), splits=splits)
            assert torch.equal(o[:, t], one), (lens, t, (o[:, t].float() - one.float()).abs().max().item())
        # (ii) the bf16 budget, whole and per (b, t, head)
        want, base = _reference(D, Hq, Hkv, Tq, lens)
        e, b = within_bf16_budget("o", o, want, base)
        es, bs = within_bf16_budget_slices("o per (b, t, head)", o.reshape(-1, D), want.reshape(-1, D),
                                           base.reshape(-1, D))
        print(f"D{D} H{Hq}/{Hkv} Tq{Tq} splits {splits} lens {lens}: err {e:.3e} (baseline {b:.3e}), "
              f"worst slice {es:.3e} (baseline {bs:.3e})")
        # queries without keys are zeros
        for bi, n in enumerate(lens):
            for t, lim in enumerate(ref.decode_multi_bounds(n, Tq, TMAX)):
                if lim == 0:
                    assert bool((o[bi, t] == 0).all()), (lens, bi, t)
        # (iii) NaN at every position >= kv_lens[b] changes no bit; (iv) nor does a second run
        kn, vn = kc.clone(), vc.clone()
        for bi, n in enumerate(lens):
            kn[bi, n:] = float("nan")
            vn[bi, n:] = float("nan")
        assert torch.equal(ops.attention_decode_multi(q, kn, vn, kv, splits=splits), o), lens
        assert torch.equal(ops.attention_decode_multi(q, kc, vc, kv, splits=splits), o), lens


def test_multi_query_strided_q_and_cache_views():
    """q a view of a packed projection (B, Tq, 3, H, D), k / v views into one buffer: what the
    models' decode steps pass."""
    D, H, Tq = 64, 2, 4
    _, kc, vc = _inputs(D, H, H, Tq)
    g = torch.Generator(device=DEV).manual_seed(9)
    qkv = torch.randn(2, Tq, 3, H, D, device=DEV, generator=g).to(torch.bfloat16)
    kv2 = torch.stack((kc, vc), dim=2)
    kv = torch.tensor([130, 9], dtype=torch.int32, device=DEV)
    o = ops.attention_decode_multi(qkv[:, :, 0], kv2[:, :, 0], kv2[:, :, 1], kv)
    assert torch.equal(o, ops.attention_decode_multi(qkv[:, :, 0].contiguous(), kc, vc, kv))


def test_multi_query_refusals():
    q, kc, vc = _inputs(64, 2, 2, 2)
    kv = torch.tensor([5, 5], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):  # (v) an FP8 cache
        ops.attention_decode_multi(q, kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), kv)
    with pytest.raises(ValueError):
        ops.attention_decode_multi(q.repeat(1, 9, 1, 1)[:, :17], kc, vc, kv)  # Tq = 17
    with pytest.raises(RuntimeError):
        ops.attention_decode_multi(q, kc, vc, kv.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.attention_decode_multi(q.clone().requires_grad_(), kc, vc, kv)

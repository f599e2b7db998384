"""Inputs of the FP8 key/value cache tests (tests/test_kv_fp8_cpu.py, tests/test_kv_fp8_gpu.py),
drawn on the CPU so that both devices see the same numbers; ``device`` moves them."""
from __future__ import annotations

import torch

from orion_amd.ops.fp8 import dequantize_kv_fp8, quantize_kv_fp8

NAN_BYTE = 0x7F  # e4m3fn NaN
ONE_BYTE = 0x38  # e4m3fn 1.0
SENT_BYTE, SENT_SCALE = 0x55, -3.0  # what the append tests fill a cache with


def as_bytes(t):
    """A float8 tensor's bytes as uint8 (comparisons and fills work on those on every device)."""
    return t.view(torch.uint8)


def quantized_cache(x):
    """x (B, T, H, D) float -> bytes (B, T, H, D) float8_e4m3fn and scales (B, H, T) fp32, contiguous."""
    q, s = quantize_kv_fp8(x)
    return q.contiguous(), s.transpose(1, 2).contiguous()


def decode_case(D, Hq, Hkv, lens, tmax, seed=0, device="cpu"):
    """bf16 q (B, Hq, D), a quantised random cache whose positions at or beyond each row's length
    hold NaN bytes and NaN scales, and int32 lengths: dict of q, kc, vc, ks, vs, lens."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    q = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
    kc, ks = quantized_cache(torch.randn(B, tmax, Hkv, D, generator=g))
    vc, vs = quantized_cache(torch.randn(B, tmax, Hkv, D, generator=g))
    for b, n in enumerate(lens):
        n = max(0, min(int(n), tmax))
        as_bytes(kc)[b, n:] = NAN_BYTE
        as_bytes(vc)[b, n:] = NAN_BYTE
        ks[b, :, n:] = float("nan")
        vs[b, :, n:] = float("nan")
    case = dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, lens=torch.tensor(lens, dtype=torch.int32))
    return {k: v.to(device) for k, v in case.items()}


def dequantized(case, dtype=torch.float32):
    """(k, v) of a case as plain tensors: exact in fp32, rounded once in bf16."""
    return dequantize_kv_fp8(case["kc"], case["ks"], dtype), dequantize_kv_fp8(case["vc"], case["vs"], dtype)


def one_hot_case(D, B=2, Hq=4, Hkv=2, device="cpu"):
    """Keys k[t] = e_t (t < D, scale 1), queries 2048 e_j with a j per (row, head) that covers both
    halves of D and both ends of a lane's 8-element slice, values small integers that are not
    symmetric in (t, d) with power-of-two scales.  The softmax weight of key j is exactly 1 in
    fp32 (the others are 2^(-2048 log2(e) / sqrt(D)) <= 2^-261 of it), so the output is row j of
    the dequantised v, bit for bit.  Returns the case and j (B, Hq)."""
    js = [0, 7, 8, D // 2 - 1, D // 2, D // 2 + 7, D - 8, D - 1]
    assert B * Hq == len(js)
    j = torch.tensor(js).view(B, Hq)
    q = torch.zeros(B, Hq, D)
    q.scatter_(2, j[..., None], 2048.0)
    kc = torch.zeros(B, D, Hkv, D, dtype=torch.uint8)
    t = torch.arange(D)
    kc[:, t, :, t] = ONE_BYTE
    d = torch.arange(D)
    vals = ((3 * t[:, None] + 5 * d[None, :]) % 15 - 7).float()  # (T, D), integers in [-7, 7]
    v = vals[None, :, None, :].expand(B, D, Hkv, D).clone()
    v[:, :, 1:] = -v[:, :, 1:].flip(-1)  # the second KV head holds other numbers
    vs = (2.0 ** ((t % 5) - 2).float())[None, None, :].expand(B, Hkv, D).contiguous()
    vc = v.to(torch.float8_e4m3fn)
    assert torch.equal(vc.float(), v), "the integers are e4m3 values"
    case = dict(q=q.to(torch.bfloat16), kc=kc.view(torch.float8_e4m3fn), vc=vc, ks=torch.ones(B, Hkv, D), vs=vs,
                lens=torch.full((B,), D, dtype=torch.int32))
    return {k: x.to(device) for k, x in case.items()}, j.to(device)


def one_hot_expected(case, j):
    """Row j[b, h] of the dequantised v of head h's KV head, as bf16 (B, Hq, D): exact."""
    _, v = dequantized(case)
    B, Hq = j.shape
    rep = Hq // v.shape[2]
    rows = [[v[b, j[b, h], h // rep] for h in range(Hq)] for b in range(B)]
    return torch.stack([torch.stack(r) for r in rows]).to(torch.bfloat16)


def append_case(T, D, B=3, Hq=4, Hkv=2, tmax=24, device="cpu"):
    """A packed bf16 projection (B, T, Hq + 2 Hkv, D) whose q / k / v are strided views, lengths
    [0, 7, tmax - T + 2] (the last row runs past tmax), and a cache filled with sentinels: bytes
    0x55 and scales -3."""
    g = torch.Generator().manual_seed(T * 1000 + D)
    packed = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16).to(device)
    kv = torch.full((B, tmax, 2, Hkv, D), SENT_BYTE, dtype=torch.uint8, device=device).view(torch.float8_e4m3fn)
    sc = torch.full((B, 2, Hkv, tmax), SENT_SCALE, device=device)
    lens_h = [0, 7, tmax - T + 2]
    return dict(q=packed[:, :, :Hq], k_new=packed[:, :, Hq:Hq + Hkv], v_new=packed[:, :, Hq + Hkv:],
                kc=kv[:, :, 0], vc=kv[:, :, 1], ks=sc[:, 0], vs=sc[:, 1], lens_h=lens_h,
                lens=torch.tensor(lens_h, dtype=torch.int32, device=device))


"""Weight-only FP8 for the decode step: OCP ``e4m3fn`` bytes (gfx950's format, not MI300's
``fnuz``) with one fp32 scale per weight row.  Quantisation runs once per session on stock torch
ops; the hot path is csrc/linear_decode_fp8.hip, which turns the bytes back into bf16 in
registers and applies the row scale once, in its fp32 epilogue.

The key/value cache uses the same bytes with one fp32 scale per (token, KV head) row of ``D``
values: :func:`quantize_kv_fp8` is the one definition of that rule, followed by the cache append
of csrc/attn_decode.hip and by ``ops.reference.kv_append``."""
from __future__ import annotations

from dataclasses import dataclass

import torch

E4M3_MAX = 448.0  # the largest finite e4m3fn value


@dataclass(frozen=True)
class Fp8Weight:
    """An (N, K) weight as ``q`` (N, K) ``float8_e4m3fn`` and ``scale`` (N,) fp32:
    W[n, k] = scale[n] q[n, k]."""
    q: torch.Tensor
    scale: torch.Tensor

    def __post_init__(self):
        q, s = self.q, self.scale
        assert q.dtype == torch.float8_e4m3fn and q.dim() == 2, (q.dtype, tuple(q.shape))
        assert s.dtype == torch.float32 and s.shape == (q.shape[0],) and s.device == q.device, \
            (s.dtype, tuple(s.shape), s.device)

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def nbytes(self):
        """Bytes held: one per element and four per row."""
        return self.q.numel() * self.q.element_size() + self.scale.numel() * self.scale.element_size()

    def dequant(self, dtype=torch.float32):
        """``q.to(fp32) * scale[:, None]`` cast to ``dtype``: exact in fp32 (a 4-bit significand
        times a 24-bit one), one rounding in bf16."""
        return (self.q.to(torch.float32) * self.scale[:, None]).to(dtype)


@torch.no_grad()
def quantize_fp8(weight) -> Fp8Weight:
    """Per-row e4m3 quantisation of an (N, K) float weight on its device: scale[n] =
    amax(|W[n, :]|) / 448 (1.0 for an all-zero row) and q[n, k] = fp8(clamp(W[n, k] / scale[n],
    -448, 448)).  The clamp comes before the cast: torch's cast saturates nothing, a value well
    beyond 448 becomes NaN."""
    assert weight.dim() == 2 and weight.is_floating_point(), (tuple(weight.shape), weight.dtype)
    w = weight.detach().to(torch.float32)
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (w / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return Fp8Weight(q.contiguous(), scale.contiguous())


@torch.no_grad()
def quantize_kv_fp8(x):
    """The key/value cache's quantisation of head rows ``x`` (..., D), on any device: per row, in
    fp32, a = max |x|, scale = a / 448 (1.0 for an all-zero row; a correctly rounded division) and
    byte = e4m3fn(clamp(x / scale, -448, 448)) rounded to nearest even, the clamp before the cast as
    in :func:`quantize_fp8`.  Returns the bytes (``float8_e4m3fn``, the shape of ``x``) and the
    scales (fp32, ``x.shape[:-1]``); value = scale * byte."""
    assert x.is_floating_point() and x.dim() >= 1, (tuple(x.shape), x.dtype)
    xf = x.detach().to(torch.float32)
    amax = xf.abs().amax(dim=-1)
    # a tensor divisor: by a Python scalar torch's GPU kernels multiply by its rounded reciprocal
    scale = torch.where(amax > 0, amax / torch.full_like(amax, E4M3_MAX), torch.ones_like(amax))
    q = (xf / scale.unsqueeze(-1)).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, scale


def dequantize_kv_fp8(q, scale, dtype=torch.float32):
    """``q.float() * scale`` for cache bytes ``q`` (..., T, H, D) and scales (..., H, T), cast once to
    ``dtype``: exact in fp32."""
    return (q.to(torch.float32) * scale.transpose(-1, -2).unsqueeze(-1)).to(dtype)

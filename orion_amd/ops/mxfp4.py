"""Weight-only MXFP4 for the decode step: the OCP microscaling 4-bit format, gfx950's native one.
An (N, K) weight is ``e2m1`` codes (sign, two exponent bits, one mantissa bit: magnitudes 0, 0.5,
1, 1.5, 2, 3, 4, 6), two per byte, with one ``e8m0`` power-of-two scale per block of 32 along K:
4.25 bits per weight.  Quantisation runs once per session on stock torch ops; the hot path is
csrc/linear_decode_mxfp4.hip, which turns the codes into bf16 in registers, the block scale
applied exactly by the conversion itself."""
from __future__ import annotations

from dataclasses import dataclass

import torch

BLOCK = 32  # elements of K per scale
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitude by code & 7; code & 8 is the sign
E2M1_MAX = 6.0
SCALE_EXP_MIN, SCALE_EXP_MAX = -125, 125  # the quantiser's clamp: scale bytes in [2, 252]


@dataclass(frozen=True)
class Mxfp4Weight:
    """A logical (N, K) weight as ``q`` (N, K / 2) uint8 and ``scale`` (N, K / 32) uint8, both
    contiguous: W[n, k] = 2^(scale[n, k // 32] - 127) e2m1(code[n, k]), the code of an even k in
    the low nibble of byte k // 2 and that of the odd k after it in the high nibble (the order
    of ``torch.float4_e2m1fn_x2``)."""
    q: torch.Tensor
    scale: torch.Tensor

    def __post_init__(self):
        q, s = self.q, self.scale
        assert q.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] % (BLOCK // 2) == 0 and q.shape[1] > 0 \
            and q.is_contiguous(), (q.dtype, tuple(q.shape))
        assert s.dtype == torch.uint8 and s.shape == (q.shape[0], q.shape[1] // (BLOCK // 2)) \
            and s.device == q.device and s.is_contiguous(), (s.dtype, tuple(s.shape), s.device)

    @property
    def shape(self):
        return torch.Size((self.q.shape[0], self.q.shape[1] * 2))

    @property
    def device(self):
        return self.q.device

    @property
    def nbytes(self):
        """Bytes held: N K / 2 of codes and N K / 32 of scales."""
        return self.q.numel() + self.scale.numel()

    def dequant(self, dtype=torch.float32):
        """The weight itself, cast to ``dtype``: exact in fp32, and in bf16 for scale bytes in
        [2, 252] (a 2-bit significand times a power of two that keeps it normal)."""
        q = self.q
        lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=q.device)
        codes = torch.stack((q & 15, q >> 4), dim=-1).view(q.shape[0], -1)  # ascending k
        s = torch.ldexp(torch.ones((), dtype=torch.float32, device=q.device), self.scale.to(torch.int32) - 127)
        return (lut[codes.long()] * s.repeat_interleave(BLOCK, dim=1)).to(dtype)


@torch.no_grad()
def quantize_mxfp4(weight) -> Mxfp4Weight:
    """OCP MXFP4 quantisation of an (N, K) float weight, K % 32 == 0, on its device, in fp32.  Per
    block of 32 along K: e = floor(log2(amax)) - 2 (from ``torch.frexp``, exact) clamped to
    [-125, 125], 0 for an all-zero block; the scale byte is e + 127 and the element
    clamp(|w| / 2^e, max=6) rounded to the nearest e2m1 value, ties to the even code, the sign
    kept.  The clamp of e makes every element times its scale a normal bf16 (0.5 x 2^-125 and
    6 x 2^125 are); scale byte 255 (the e8m0 NaN) is never produced.  The kernel's result for
    scale bytes outside [2, 252] (a given ``Mxfp4Weight`` may hold them) is unspecified."""
    assert weight.dim() == 2 and weight.is_floating_point(), (tuple(weight.shape), weight.dtype)
    N, K = weight.shape
    assert K > 0 and K % BLOCK == 0, f"quantize_mxfp4: K % 32 == 0 (one scale per 32 along K), got K = {K}"
    w = weight.detach().to(torch.float32).reshape(N, K // BLOCK, BLOCK)
    amax = w.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)  # amax = m 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, (ex - 3).clamp(SCALE_EXP_MIN, SCALE_EXP_MAX), torch.zeros_like(ex))
    a = torch.ldexp(w.abs(), -e.unsqueeze(-1)).clamp_(max=E2M1_MAX)
    # steps of 0.5 below 2, of 1 below 4, of 2 up to 6; torch.round goes to the even integer,
    # which on each stretch is the even code
    code = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, torch.round(a / 2) + 4))
    code = code.to(torch.uint8) | (torch.signbit(w).to(torch.uint8) << 3)
    code = code.view(N, K // 2, 2)
    q = code[..., 0] | (code[..., 1] << 4)
    return Mxfp4Weight(q.contiguous(), (e + 127).to(torch.uint8).contiguous())

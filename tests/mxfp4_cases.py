"""Cases of the MXFP4 skinny-linear tests, drawn with a CPU generator so that the GPU tests
(tests/test_linear_decode_mxfp4_gpu.py, which move them to the device) and the CPU tests
(tests/test_mxfp4_weights_cpu.py, which emulate the ideal kernel on them) see identical inputs.

Shapes: a K of one 32-element block; an odd N with a masked last tile and a K that is no multiple
of a 128-element lane-group block; a K with a remainder after several rounds; more than one full
tile plus a tail.  Then the kernel's own boundaries +- 32 at N = 48 (three tiles: the header of
tests/test_linear_decode_gpu.py says why not 16).  csrc/linear_decode_mxfp4.hip has two forms:
4 waves that take chunks of 128 elements, a round of 512 (every form with a prologue or an
activation, and plain projections with K < 2048); and, for a plain projection (no prologue, no
activation) with K >= 2048, 8 waves that take chunks of 256, a round of 2048.  So the chunk and
round sizes 128, 256, 512 and 2048, and in the wide form one round plus one chunk (2304) and two
rounds (4096)."""
import torch
import torch.nn.functional as F

from fp8_cases import EPIS, MS, NORMS, call, twin_of  # noqa: F401  (shared with the FP8 tests)
from orion_amd import ops

SHAPES = [(16, 32), (41, 96), (48, 1120), (130, 256)] + \
    [(48, k + d) for k in (128, 256, 512, 2048, 2304, 4096) for d in (-32, 0, 32)]
SMALL_SHAPES = [(16, 32), (41, 96), (48, 1120), (130, 256), (16, 160), (24, 288), (24, 544), (16, 2016),
                (24, 2080), (16, 4128)]


def make_case(m, n, k, norm, epi, seed=0, device="cpu"):
    """Keyword arguments of ops.linear_decode for one case: bf16 tensors and an ``ops.Mxfp4Weight``
    (the quantised random weight).  Drawn on the CPU whatever ``device`` is."""
    g = torch.Generator().manual_seed(seed)

    def r(*s):
        return torch.randn(*s, generator=g)

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
    kw = {a: v.to(torch.bfloat16) if torch.is_tensor(v) else v for a, v in kw.items()}
    kw["weight"] = ops.quantize_mxfp4(kw["weight"])
    return to_device(kw, device)


def make_integer_case(m, n, k, seed=0, device="cpu"):
    """No norm, no activation: x integers in [-8, 8], every code byte drawn uniformly (so per
    element), scale bytes in 124..129 drawn per block, integer bias and residual.  Every product
    is a multiple of 2^-4 of at most 8 x 6 x 4 = 192, and every partial sum over K <= 256 a multiple
    of 2^-4 below 2^16: exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=g)

    q = ints(0, 255, n, k // 2).to(torch.uint8)
    scale = ints(124, 129, n, k // 32).to(torch.uint8)
    kw = dict(x=ints(-8, 8, m, k).to(torch.bfloat16), weight=ops.Mxfp4Weight(q, scale),
              bias=ints(-8, 8, n).to(torch.bfloat16), residual=ints(-8, 8, m, n).to(torch.bfloat16))
    return to_device(kw, device)


def to_device(kw, device):
    def mv(v):
        if isinstance(v, ops.Mxfp4Weight):
            return ops.Mxfp4Weight(v.q.to(device), v.scale.to(device))
        return v.to(device) if torch.is_tensor(v) else v
    return {a: mv(v) for a, v in kw.items()}


def composed(kw, dtype):
    """The unfused composition on stock torch ops in ``dtype`` on the dequantised weight: fp32
    (exact dequantisation) is the reference, bf16 (every op's output rounded; the dequantised
    weight is exact in bf16 too) the baseline."""
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
    y = F.linear(h, kw["weight"].dequant(dtype), t("bias"))
    if kw.get("act") == "gelu":
        y = F.gelu(y, approximate="tanh")
    elif kw.get("act") == "swiglu":
        gate, up = y.chunk(2, dim=-1)
        y = F.silu(gate) * up
    return y if kw.get("residual") is None else y + t("residual")


def ideal_kernel(kw):
    """What an ideal fused kernel gives, on fp32 CPU ops: the normalised x rounded to bf16, the
    exact weight (code times block scale), fp32 sums, the epilogue in fp32, one rounding at the
    store."""
    f = torch.float32
    x = kw["x"].to(f)
    K = x.shape[-1]
    if kw.get("norm") == "layer":
        b = kw.get("norm_bias")
        x = F.layer_norm(x, (K,), kw["norm_weight"].to(f), None if b is None else b.to(f), kw["eps"])
    elif kw.get("norm") == "rms":
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + kw["eps"]) * kw["norm_weight"].to(f)
    x = x.to(torch.bfloat16).to(f)
    y = x @ kw["weight"].dequant(f).t()
    if kw.get("bias") is not None:
        y = y + kw["bias"].to(f)
    if kw.get("act") == "gelu":
        y = F.gelu(y, approximate="tanh")
    elif kw.get("act") == "swiglu":
        gate, up = y.chunk(2, dim=-1)
        y = F.silu(gate) * up
    if kw.get("residual") is not None:
        y = y + kw["residual"].to(f)
    return y.to(torch.bfloat16)

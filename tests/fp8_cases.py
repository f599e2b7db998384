"""Cases of the FP8 skinny-linear tests, drawn with a CPU generator so that the GPU tests
(tests/test_linear_decode_fp8_gpu.py, which move them to the device) and the CPU tests
(tests/test_fp8_weights_cpu.py, which emulate the ideal kernel on them) see identical inputs.

Shapes: a K of one 16-element fragment; an odd N with a masked last tile and a K that is no
multiple of a 64-element block; a K with a remainder after several rounds; more than one full
tile plus a tail.  Then the kernel's own boundaries +- 16 at N = 48 (three tiles: the header of
tests/test_linear_decode_gpu.py says why not 16).  csrc/linear_decode_fp8.hip has three forms:
with a prologue, 4 waves that take chunks of 64 elements, a round of 256; without one, 4 waves
that take chunks of 128, a round of 512; and, for a plain projection (no prologue, no
activation) with K >= 2048, 8 waves that take chunks of 256, a round of 2048.  So the chunk and
round sizes 64, 128, 256, 512 and 2048, and in the wide form one round plus one chunk (2304)
and two rounds (4096)."""
import copy

import torch
import torch.nn.functional as F

from orion_amd import ops

MS = [1, 2, 5, 8, 16]
SHAPES = [(16, 16), (41, 80), (48, 1104), (130, 256)] + \
    [(48, k + d) for k in (64, 128, 256, 512, 2048, 2304, 4096) for d in (-16, 0, 16)]
NORMS = [None, "layer", "layer-nobeta", "rms"]
EPIS = ["none", "bias", "gelu", "bias-gelu", "residual", "bias-residual", "swiglu", "bias-swiglu"]
SMALL_SHAPES = [(16, 16), (41, 80), (48, 1104), (130, 256), (16, 48), (16, 112), (24, 272), (24, 528), (16, 2032),
                (24, 2064), (16, 4112)]


def make_case(m, n, k, norm, epi, seed=0, device="cpu"):
    """Keyword arguments of ops.linear_decode for one case: bf16 tensors and an ``ops.Fp8Weight``
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
    kw["weight"] = ops.quantize_fp8(kw["weight"])
    return to_device(kw, device)


def make_integer_case(m, n, k, seed=0, device="cpu"):
    """No norm, no activation, every value a small integer: x and q in [-8, 8] (q drawn per
    element, every one an e4m3 value), scales powers of two, integer bias and residual.  Every
    partial sum is an integer below 2^24 times a power of two, exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=g).float()

    q = ints(-8, 8, n, k).to(torch.float8_e4m3fn)
    scale = 2.0 ** ints(-3, 2, n)
    kw = dict(x=ints(-8, 8, m, k).to(torch.bfloat16), weight=ops.Fp8Weight(q, scale),
              bias=ints(-8, 8, n).to(torch.bfloat16), residual=ints(-8, 8, m, n).to(torch.bfloat16))
    return to_device(kw, device)


def to_device(kw, device):
    def mv(v):
        if isinstance(v, ops.Fp8Weight):
            return ops.Fp8Weight(v.q.to(device), v.scale.to(device))
        return v.to(device) if torch.is_tensor(v) else v
    return {a: mv(v) for a, v in kw.items()}


def composed(kw, dtype):
    """The unfused composition on stock torch ops in ``dtype`` on the dequantised weight: fp32
    (exact dequantisation) is the reference, bf16 (the weight and every op's output rounded) the
    baseline."""
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
    exact q, fp32 sums, the row scale, the epilogue in fp32, one rounding at the store."""
    f = torch.float32
    x = kw["x"].to(f)
    K = x.shape[-1]
    if kw.get("norm") == "layer":
        b = kw.get("norm_bias")
        x = F.layer_norm(x, (K,), kw["norm_weight"].to(f), None if b is None else b.to(f), kw["eps"])
    elif kw.get("norm") == "rms":
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + kw["eps"]) * kw["norm_weight"].to(f)
    x = x.to(torch.bfloat16).to(f)
    w = kw["weight"]
    y = (x @ w.q.to(f).t()) * w.scale
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


def call(kw):
    kw = dict(kw)
    return ops.linear_decode(kw.pop("x"), kw.pop("weight"), kw.pop("bias", None), **kw)


def twin_of(model, qweights, dtype=torch.float32, device=None):
    """A deep copy of ``model`` in ``dtype`` whose projection weights are the dequantised entries
    of a session's ``qweights`` (exact in fp32, rounded once in bf16).  GPT-2's head gets a
    parameter of its own, so the token embedding keeps the unquantised table, as the session
    does.  Buffers (the fp32 RoPE tables) keep their dtype."""
    twin = copy.deepcopy(model)
    for prm in twin.parameters():
        prm.data = prm.data.to(dtype)
    for name, qw in qweights.items():
        try:
            mod = twin.get_submodule(name)
        except AttributeError:
            mod = twin.get_submodule("transformer." + name)
        mod.weight = torch.nn.Parameter(qw.dequant(torch.float32).to(dtype), requires_grad=False)
    return (twin if device is None else twin.to(device)).eval()

"""LayerNorm / RMSNorm autograd wrappers over the HIP kernels (csrc/layernorm.hip,
csrc/rmsnorm_rope.hip).  Weights may be fp32 (eval/inference) or bf16 (arena);
kernels always see bf16 and gradients are returned in the weight's dtype."""
from __future__ import annotations

import torch

from ._ext import C
from .grad_sink import claim_bf16, finish, out_view


def as_bf16(t):
    return t if t is None or t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


def layer_norm_backward(dy, x, mean, rstd, w, b, rb=None, dres=None):
    """(dx, dw, db, drb) of y = LayerNorm(x) from dy (None: y was not used), with the gradient
    ``dres`` of a second consumer of x folded into dx (None: there was none) and, for a branch
    bias ``rb`` that was added into x, drb = colsum(dx).  The three small gradients go straight
    into their gradient-arena slices where they can (ops/grad_sink.py; None is returned for
    those), else they are returned in their parameter's dtype; db / drb are None without b / rb."""
    if dy is None:
        dy = torch.zeros_like(x)
    dres = None if dres is None else dres.contiguous()
    sw, sb, srb = claim_bf16(w, b, rb)
    dx, dw, db, drb = C().layernorm_bwd(dy.contiguous(), x, as_bf16(w), mean, rstd, b is not None,
                                        dres, rb is not None, out_view(sw), out_view(sb),
                                        out_view(srb))
    return (dx, finish(dw, sw, w.dtype), None if b is None else finish(db, sb, b.dtype),
            None if rb is None else finish(drb, srb, rb.dtype))


def rms_norm_backward(dy, x, rstd, w, dres=None):
    """(dx, dw) of y = RMSNorm(x); dy, dres and the arena as for ``layer_norm_backward``."""
    if dy is None:
        dy = torch.zeros_like(x)
    dres = None if dres is None else dres.contiguous()
    (sw,) = claim_bf16(w)
    dx, dw = C().rmsnorm_bwd(dy.contiguous(), x, as_bf16(w), rstd, dres, out_view(sw))
    return dx, finish(dw, sw, w.dtype)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        xb = as_bf16(x)
        y, mean, rstd = C().layernorm_fwd(xb, as_bf16(w), as_bf16(b), float(eps))
        ctx.save_for_backward(xb, w, mean, rstd)
        ctx.x_dtype = x.dtype
        ctx.params = (w, b)
        return y.view(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xb, _, mean, rstd = ctx.saved_tensors
        dx, dw, db, _ = layer_norm_backward(as_bf16(dy.contiguous()), xb, mean, rstd, *ctx.params)
        return dx.view(xb.shape).to(ctx.x_dtype), dw, db, None


def layer_norm_hip(x, weight, bias, eps=1e-5):
    return _LayerNorm.apply(x, weight, bias, eps)


class _AddLayerNorm(torch.autograd.Function):
    """(s, y) = (x + (r + rb), LayerNorm(s)).  ``rb`` is the bias of the branch's output
    projection (added here instead of in the GEMM epilogue).  Backward folds the
    residual-stream gradient ds into the LayerNorm input gradient and produces the
    branch-bias gradient colsum(ds_total) in the same kernel."""

    @staticmethod
    def forward(ctx, x, r, w, b, rb, eps):
        s, y, mean, rstd = C().add_layernorm_fwd(x, r, as_bf16(w), as_bf16(b), float(eps), as_bf16(rb))
        # an unused output (the last block's residual sum) arrives as None, not as a
        # materialised zero tensor (a 100 MB fill + read per step on GPT-2)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(s, w, mean, rstd)
        ctx.params = (w, b, rb)
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, ds, dy):
        s, _, mean, rstd = ctx.saved_tensors
        dx, dw, db, drb = layer_norm_backward(dy, s, mean, rstd, *ctx.params, dres=ds)
        dx = dx.view(s.shape)
        return dx, dx, dw, db, drb, None


def add_layer_norm_hip(x, r, weight, bias, eps=1e-5, r_bias=None):
    return _AddLayerNorm.apply(x, r, weight, bias, r_bias, eps)


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        xb = as_bf16(x)
        y, rstd = C().rmsnorm_fwd(xb, as_bf16(w), float(eps))
        ctx.save_for_backward(xb, w, rstd)
        ctx.x_dtype = x.dtype
        ctx.weight = w
        return y.view(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xb, _, rstd = ctx.saved_tensors
        dx, dw = rms_norm_backward(as_bf16(dy.contiguous()), xb, rstd, ctx.weight)
        return dx.view(xb.shape).to(ctx.x_dtype), dw, None


def rms_norm_hip(x, weight, eps=1e-5):
    return _RMSNorm.apply(x, weight, eps)


class _AddRMSNorm(torch.autograd.Function):
    """(s, y) = (x + r, RMSNorm(x + r)) with the residual gradient folded into backward."""

    @staticmethod
    def forward(ctx, x, r, w, eps):
        s, y, rstd = C().add_rmsnorm_fwd(x, r, as_bf16(w), float(eps))
        ctx.set_materialize_grads(False)  # see _AddLayerNorm
        ctx.save_for_backward(s, w, rstd)
        ctx.weight = w
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, ds, dy):
        s, _, rstd = ctx.saved_tensors
        dx, dw = rms_norm_backward(dy, s, rstd, ctx.weight, dres=ds)
        dx = dx.view(s.shape)
        return dx, dx, dw, None


def add_rms_norm_hip(x, r, weight, eps=1e-5):
    return _AddRMSNorm.apply(x, r, weight, eps)

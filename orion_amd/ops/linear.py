"""The linear layer's autograd node over the GEMMs of ops/gemm.py, and the order of a linear
layer's two backward GEMMs for every node that ends in one."""
from __future__ import annotations

import torch

from . import gemm  # WGRAD_FIRST is read at call time
from .gemm import bias_grad, linear_dgrad, linear_fwd, weight_grad
from .grad_sink import sink_of


def grads_in_order(dgrad, wgrad, need_dx, need_dw, wgrad_first):
    """(dx, dW) of one linear layer from the two callables, each run only if needed: the input
    gradient before the weight gradient, or after it with ``wgrad_first`` (ops/gemm.py,
    WGRAD_FIRST: dX is then written right before the next backward kernel reads it)."""
    dx = dgrad() if need_dx and not wgrad_first else None
    dw = wgrad() if need_dw else None
    if need_dx and wgrad_first:
        dx = dgrad()
    return dx, dw


def linear_input_weight_grads(dy2, x, w, sink, need_dx, need_dw):
    """dx = dy W and dW = dy^T x of y = x W^T (dy2: (rows, N)), in the configured order
    (ops.gemm.WGRAD_FIRST); dW goes straight into the gradient arena through ``sink`` when
    there is one (then None is returned for it)."""
    return grads_in_order(lambda: linear_dgrad(dy2, w).view(x.shape),
                          lambda: weight_grad(dy2, x.reshape(-1, x.shape[-1]), sink),
                          need_dx, need_dw, gemm.WGRAD_FIRST)


class _Linear(torch.autograd.Function):
    """y = x W^T + b on hipBLASLt (or csrc/gemm.hip: ops/gemm.py); backward computes the
    bias gradient with the deterministic two-stage column-sum kernel instead of a generic
    reduction."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.sink = sink_of(w)  # dW straight into the gradient arena (ops/grad_sink.py)
        ctx.bias = b
        return linear_fwd(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        db = None
        want_db = ctx.bias is not None and ctx.needs_input_grad[2]
        if want_db and gemm.WGRAD_FIRST:  # dY was just written by the previous kernel: sum it now
            db = bias_grad(dy2, ctx.bias)
        dx, dw = linear_input_weight_grads(dy2, x, w, ctx.sink, ctx.needs_input_grad[0],
                                           ctx.needs_input_grad[1])
        if want_db and not gemm.WGRAD_FIRST:
            db = bias_grad(dy2, ctx.bias)
        return dx, dw, db


def linear_hip(x, weight, bias=None):
    return _Linear.apply(x, weight, bias)

"""The producer side of the gradient-sink protocol (ops/grad_sink.py: claim_bf16, out_view,
finish) and the one weight-gradient rule built on it (ops/gemm.py: weight_grad), on CPU
tensors with the GEMMs replaced by recorders: what is called with which ``accumulate`` flag,
what is returned to autograd, and when the arena's listeners hear of the parameter."""
import pytest
import torch

from orion_amd.ops import gemm
from orion_amd.ops.grad_sink import GradSink, claim_bf16, finish, out_view


def _sunk(dtype=torch.bfloat16, shape=(6, 4)):
    """(param, sink, heard): a parameter with a sink on a param-shaped arena slice; ``heard``
    lists the parameters reported to the arena's listener."""
    p = torch.zeros(shape, dtype=dtype, requires_grad=True)
    heard = []
    sink = GradSink(p, torch.zeros(shape), [heard.append])
    p._orion_sink = sink
    return p, sink, heard


@pytest.fixture
def gemms(monkeypatch):
    """ops.gemm.wgrad / wgrad_into replaced by recorders; wgrad returns a marker tensor."""
    calls, marker = [], torch.full((6, 4), 3.0)
    monkeypatch.setattr(gemm, "wgrad", lambda *a: calls.append(("wgrad",) + a) or marker)
    monkeypatch.setattr(gemm, "wgrad_into", lambda *a: calls.append(("wgrad_into",) + a))
    return calls, marker


def test_weight_grad_without_sink_returns_wgrad(gemms):
    calls, marker = gemms
    dy, x, scale = torch.ones(8, 6), torch.ones(8, 4), torch.tensor([0.5])
    assert gemm.weight_grad(dy, x, None) is marker
    assert gemm.weight_grad(dy, x, None, scale) is marker
    assert [c[0] for c in calls] == ["wgrad", "wgrad"]
    assert calls[0][1] is dy and calls[0][2] is x and calls[0][3] is None
    assert calls[1][3] is scale


def test_weight_grad_through_sink_overwrites_then_accumulates(gemms):
    calls, _ = gemms
    p, sink, heard = _sunk()
    dy, x, scale = torch.ones(8, 6), torch.ones(8, 4), torch.tensor([0.5])
    assert gemm.weight_grad(dy, x, sink) is None
    assert len(calls) == 1 and heard == [p]  # the listener fired once
    name, a_dy, a_x, a_out, a_acc, a_scale = calls[0]
    assert name == "wgrad_into" and a_dy is dy and a_x is x and a_out is sink.view
    assert a_acc is False and a_scale is None
    assert gemm.weight_grad(dy, x, sink, scale) is None  # second micro-batch of the step
    assert calls[1][4] is True and calls[1][5] is scale and heard == [p, p]
    sink.reset()
    assert gemm.weight_grad(dy, x, sink, scale) is None
    assert calls[2][4] is False and calls[2][5] is scale
    assert [c[0] for c in calls] == ["wgrad_into"] * 3


def test_claim_bf16_only_fresh_bf16_sinks():
    p, sink, _ = _sunk()
    p32, _, _ = _sunk(torch.float32)
    plain = torch.zeros(4, dtype=torch.bfloat16)
    assert claim_bf16(None, p32, plain, p) == (None, None, None, sink)
    assert claim_bf16(p) == (None,)  # second claim of the step: AccumulateGrad's turn
    sink.reset()
    assert claim_bf16(p) == (sink,)
    assert out_view(sink) is sink.view and out_view(None) is None


def test_finish_notifies_the_sink_or_returns_the_gradient():
    p, sink, heard = _sunk()
    assert finish(sink.view, sink, torch.bfloat16) is None  # never the slice itself
    assert heard == [p]
    g = torch.ones(4, dtype=torch.bfloat16)
    out = finish(g, None, torch.float32)
    assert out.dtype == torch.float32 and torch.equal(out, g.float())
    assert finish(g, None) is g
    assert finish(None, None, torch.float32) is None
    assert heard == [p]

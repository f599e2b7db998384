"""The per-slice error budget of tests/tolerance.py, on the CPU: it passes an ideal kernel
(fp32 math, one rounding) and rejects one wrong row among 33001, or one wrong element of a
column sum, which the whole-tensor budget need not."""
import pytest
import torch

from tolerance import rel_err, slice_errs, within_bf16_budget, within_bf16_budget_slices

F = torch.nn.functional
ROWS, C = 33001, 128


@pytest.fixture(scope="module")
def ln():
    """fp32 reference, stock bf16 baseline and the ideal bf16 result of one LayerNorm
    forward / backward (y, dw); read-only."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(ROWS, C, generator=g).bfloat16()
    w = (1 + 0.1 * torch.randn(C, generator=g)).bfloat16()
    b = (0.1 * torch.randn(C, generator=g)).bfloat16()
    dy = torch.randn(ROWS, C, generator=g).bfloat16()
    wr = w.float().requires_grad_()
    yr = F.layer_norm(x.float(), (C,), wr, b.float(), 1e-5)
    yr.backward(dy.float())
    yb = F.layer_norm(x, (C,), w, b, 1e-5)
    return {"y": yr.detach(), "y_base": yb, "y_ideal": yr.detach().bfloat16(),
            "dw": wr.grad, "dw_ideal": wr.grad.bfloat16()}


def test_ideal_result_passes_both_budgets(ln):
    e, b = within_bf16_budget("y", ln["y_ideal"], ln["y"], ln["y_base"])
    es, bs = within_bf16_budget_slices("y", ln["y_ideal"], ln["y"], ln["y_base"], dim=0)
    print(f"global {e:.3e} / {b:.3e}; worst row {es:.3e} / {bs:.3e}")
    assert es >= e and bs >= b  # the worst row is no better than the average one
    within_bf16_budget_slices("dw", ln["dw_ideal"], ln["dw"], ln["dw_ideal"])


def test_slice_errors_are_per_slice_rms_over_global_rms(ln):
    y, got = ln["y"], ln["y_ideal"]
    e = slice_errs(got, y, 0)
    assert e.shape == (ROWS,)
    want = (got.float() - y).double().pow(2).mean(1).sqrt() / y.double().pow(2).mean().sqrt()
    assert torch.allclose(e, want, rtol=1e-9, atol=0)
    # along the other dim, and the mean of the squares is the whole tensor's relative error
    ec = slice_errs(got, y, 1)
    assert ec.shape == (C,)
    assert abs(ec.pow(2).mean().sqrt().item() - rel_err(got, y)) < 1e-6
    assert slice_errs(ln["dw_ideal"], ln["dw"]).shape == (C,)


def test_zeroed_last_row_fails_the_slice_budget_and_is_named(ln):
    bad = ln["y_ideal"].clone()
    bad[-1] = 0
    with pytest.raises(AssertionError, match=r"slice 33000 along dim 0"):
        within_bf16_budget_slices("y", bad, ln["y"], ln["y_base"], dim=0)
    # the whole-tensor error of that result is within a budget this suite uses for LayerNorm
    # (dx of stock bf16: 2 x 2.5e-3 + 1e-3), which is why the per-row budget exists
    assert rel_err(bad, ln["y"]) < 2 * 2.5e-3 + 1e-3


def test_nan_row_fails_the_slice_budget(ln):
    bad = ln["y_ideal"].clone()
    bad[17, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"slice 17 along dim 0"):
        within_bf16_budget_slices("y", bad, ln["y"], ln["y_base"], dim=0)


def test_zeroed_element_of_a_column_sum_fails_the_slice_budget(ln):
    dw = ln["dw"]
    i = int(dw.abs().argmax())
    bad = ln["dw_ideal"].clone()
    bad[i] = 0
    with pytest.raises(AssertionError, match=rf"slice {i} along dim 0"):
        within_bf16_budget_slices("dw", bad, dw, ln["dw_ideal"])

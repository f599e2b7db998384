"""The row loops of the LayerNorm, RMSNorm, column-sum and RoPE kernels (csrc/layernorm.hip,
csrc/rmsnorm_rope.hip, csrc/activations.hip) against fp32 autograd of the plain PyTorch
composition, at row counts where a wave or workgroup visits several rows and at every width
variant, checked per row.

Budgets (tests/tolerance.py).  Activation-shaped outputs (y, s, dx) on their (rows, C) view:
the whole-tensor budget and the per-row one, both against stock PyTorch bf16.  Column sums
(dw, db, the branch-bias gradient): a bf16 output against the one-rounding result
``ref32.to(bf16)`` (whole tensor and per element), an fp32 output to rel err < 1e-4 (fp32
accumulated, fp32 stored).  The branch-bias gradient is by definition the column sum of the
kernel's own ROUNDED dx (what stock PyTorch's bias gradient of a bf16 dx is too), so its fp32
form is held to 1e-4 against ``dx_kernel.float().sum(0)``; against the fp32 reference, where
the rows' roundings leave ~1e-3 whatever the kernel does, it gets the bf16 budget with the
column sum of the one-rounding dx as the baseline.

Every figure is printed before it is asserted (``pytest -s``), lines starting ``[norm-rows]``;
``stock`` lines are the error of stock bf16 dw / db against fp32, for the record only.
"""
import os
import subprocess
import sys

import pytest
import torch

from orion_amd import ops
from orion_amd.ops import reference as ref
from orion_amd.ops._ext import C as ext
from tolerance import rel_err, torch_bf16, within_bf16_budget, within_bf16_budget_slices

F = torch.nn.functional

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
FP32_SUM_BOUND = 1e-4  # test_wgrad_into_fp32's bound for fp32-accumulated, fp32-stored sums
SENTINEL = -777.0
PAD = 5  # an odd offset: the arena slices are not 16-byte aligned


@pytest.fixture(scope="module", autouse=True)
def _ext():
    ops.set_backend("hip")
    assert ops.load_ext(required=True)
    yield


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def grid(*shape, scale=1.0):
    """Multiples of 1/16 within [-4, 4]: a sum of three of them is exact in bf16."""
    return ((torch.randn(*shape, device=DEV) * scale * 16).round().clamp(-64, 64) / 16).to(torch.bfloat16)


def norm_weight(C):
    return (1 + 0.1 * torch.randn(C, device=DEV)).to(torch.bfloat16)


def report(tag, **figs):
    print(f"[norm-rows] {tag} " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))


def check_act(tag, name, got, ref32, base):
    """An activation-shaped output: whole-tensor and per-row budgets on the (rows, C) view."""
    C = got.shape[-1]
    g, r, b = (t.reshape(-1, C) for t in (got, ref32, base))
    e, eb = within_bf16_budget(name, g, r, b)
    s, sb = within_bf16_budget_slices(name, g, r, b, dim=0)
    report(f"{tag} {name}", err=e, base=eb, worst_row=s, base_worst_row=sb)


def check_sum(tag, name, got, ref32):
    """A column-sum output against the fp32 reference: fp32 to 1e-4, bf16 within the budget
    of the one-rounding result (whole tensor and per element)."""
    assert got.shape == ref32.shape, (name, got.shape, ref32.shape)
    if got.dtype == torch.float32:
        e = rel_err(got, ref32)
        report(f"{tag} {name} fp32", err=e)
        assert e < FP32_SUM_BOUND, f"{name}: fp32 column sum rel err {e:.3e} >= {FP32_SUM_BOUND:.0e}"
        return
    base = ref32.to(got.dtype)
    e, eb = within_bf16_budget(name, got, ref32, base)
    s, sb = within_bf16_budget_slices(name, got, ref32, base)
    report(f"{tag} {name} bf16", err=e, base=eb, worst_el=s, base_worst_el=sb)


def check_dx_colsum(tag, name, got, dx_kernel, dx_ref32):
    """The branch-bias gradient (see the module docstring): the column sum of the kernel's own
    rounded dx, and within the bf16 budget of the fp32 reference's column sum."""
    C = got.shape[-1]
    own = dx_kernel.reshape(-1, C).double().sum(0).float()
    ref_sum = dx_ref32.reshape(-1, C).double().sum(0).float()
    if got.dtype == torch.float32:
        e = rel_err(got, own)
        report(f"{tag} {name} fp32 vs own dx", err=e, vs_ref32=rel_err(got, ref_sum))
        assert e < FP32_SUM_BOUND, f"{name}: rel err {e:.3e} vs the column sum of the kernel's dx"
        base = dx_ref32.reshape(-1, C).bfloat16().double().sum(0).float()
        within_bf16_budget(name, got, ref_sum, base)
        within_bf16_budget_slices(name, got, ref_sum, base)
        return
    within_bf16_budget(f"{name} vs own dx", got, own, own.to(got.dtype))
    within_bf16_budget_slices(f"{name} vs own dx", got, own, own.to(got.dtype))
    check_sum(tag, name, got, ref_sum)


class Guarded:
    """C-element views at an odd offset inside one sentinel-filled buffer; ``intact()`` is
    whether every element outside the views still holds the sentinel."""

    def __init__(self, C, dtype, n):
        self.C, self.n = C, n
        self.buf = torch.full((n * (C + PAD) + PAD,), SENTINEL, dtype=dtype, device=DEV)

    def view(self, i):
        o = PAD + i * (self.C + PAD)
        return self.buf[o:o + self.C]

    def intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for i in range(self.n):
            o = PAD + i * (self.C + PAD)
            mask[o:o + self.C] = False
        return bool((self.buf[mask] == SENTINEL).all())


# --------------------------------------------------------------------------- LayerNorm
def ln_torch(dtype, C, x, r, rb, w, b, dy, ds):
    """s = x [+ (r [+ rb])], y = LayerNorm(s) and the gradients of <y, dy> [+ <s, ds>] with
    stock PyTorch in ``dtype``: fp32 is the reference, bf16 the budgets' baseline."""
    xx, rr, rbb, ww, bb = (None if t is None else t.detach().to(dtype).requires_grad_()
                           for t in (x, r, rb, w, b))
    s = xx.view_as(xx) if rr is None else xx + (rr if rbb is None else rr + rbb)
    y = F.layer_norm(s, (C,), ww, bb, EPS)
    outs, gouts = [y], [dy.to(dtype)]
    if ds is not None:
        outs.append(s)
        gouts.append(ds.to(dtype))
    torch.autograd.backward(outs, gouts)
    g = {"s": s.detach(), "y": y.detach(), "dx": xx.grad, "dw": ww.grad}
    g["db"] = None if bb is None else bb.grad
    g["drb"] = None if rbb is None else rbb.grad
    return g


# rows 1 / 5 / 9: wave 0 of the backward gets 1 / 2 / 3 rows, the other waves none or one;
# 4099: 65 backward workgroups, the last with 3 rows; 16385 / 32771 / 49154: 2 / 3 / 4 rows per
# wave of ln_fwd1_kernel (4096 workgroups), both exits of its pipelined loop, and more
# backward rows than one resident round.  C: 128 <8,1> 16 active lanes; 520 <8,2> with one
# lane in the second iteration (the clamped load); 2048 <8,4>, the widest; 256 backward
# <4,1,EXACT>; 260 the 4-wide non-exact path.
LN_CASES = ([(rows, C) for C in (128, 520, 2048, 256, 260) for rows in (1, 5, 9, 4099)]
            + [(16385, 128), (32771, 128), (49154, 128), (32771, 520), (32771, 260)])
NO_BIAS_ROWS = (5, 32771)  # these run with bias=None


def ln_inputs(rows, C, exact_sum=False):
    """``exact_sum``: x, r and rb on a grid that makes s = x + (r + rb) exact in bf16.  The op
    normalises the bf16 s it returns while the fp32 reference normalises the unrounded sum;
    one rounding of s moves a column sum over few rows by as much as the one rounding of the
    result that its budget allows, so the add forms are given sums that need no rounding."""
    torch.manual_seed(rows * 4099 + C)
    b = None if rows in NO_BIAS_ROWS else bf(C, scale=0.1)
    rnd = grid if exact_sum else bf
    return dict(x=rnd(rows, C), r=rnd(rows, C), rb=rnd(C, scale=0.5), w=norm_weight(C), b=b,
                dy=bf(rows, C), ds=bf(rows, C))


@pytest.mark.parametrize("mode", ["plain", "add", "add_rbias"])
@pytest.mark.parametrize("rows,C", LN_CASES)
def test_layernorm_rows(rows, C, mode):
    """ops.layer_norm (ln_fwd1_kernel) and ops.add_layer_norm without / with r_bias
    (ln_fwd_kernel), forward and backward (ln_bwd_kernel with dres and the branch-bias
    column sum in the add forms), bf16 gradients."""
    t = ln_inputs(rows, C, exact_sum=mode != "plain")
    tag = f"ln {mode} {rows}x{C}"
    x, w, b = t["x"].requires_grad_(), t["w"].requires_grad_(), t["b"]
    if b is not None:
        b.requires_grad_()
    r = rb = ds = None
    if mode == "plain":
        y = ops.layer_norm(x, w, b)
        y.backward(t["dy"])
    else:
        r, ds = t["r"].requires_grad_(), t["ds"]
        rb = t["rb"].requires_grad_() if mode == "add_rbias" else None
        s, y = ops.add_layer_norm(x, r, w, b, r_bias=rb)
        torch.autograd.backward((s, y), (ds, t["dy"]))
    r32 = ln_torch(torch.float32, C, x, r, rb, w, b, t["dy"], ds)
    b16 = ln_torch(torch.bfloat16, C, x, r, rb, w, b, t["dy"], ds)
    check_act(tag, "y", y.detach(), r32["y"], b16["y"])
    check_act(tag, "dx", x.grad, r32["dx"], b16["dx"])
    if mode != "plain":
        check_act(tag, "s", s.detach(), r32["s"], b16["s"])
        assert torch.equal(s.detach().float(), r32["s"])  # exact sums (ln_inputs)
        assert torch.equal(r.grad, x.grad)
    assert w.grad.dtype == torch.bfloat16
    check_sum(tag, "dw", w.grad, r32["dw"])
    stock = {"dw": rel_err(b16["dw"], r32["dw"])}
    if b is not None:
        check_sum(tag, "db", b.grad, r32["db"])
        stock["db"] = rel_err(b16["db"], r32["db"])
    if rb is not None:
        check_dx_colsum(tag, "drb", rb.grad, x.grad, r32["dx"])
    report(f"{tag} stock", **stock)


@pytest.mark.parametrize("rows,C", LN_CASES)
def test_layernorm_bwd_fp32_arena_rows(rows, C):
    """C().layernorm_bwd with dres, the branch-bias column sum and fp32 dw_out / db_out /
    dxs_out slices inside a sentinel-filled buffer."""
    t = ln_inputs(rows, C)
    tag = f"ln arena {rows}x{C}"
    x, w, b, dy, ds = t["x"], t["w"], t["b"], t["dy"], t["ds"]
    y, mean, rstd = ext().layernorm_fwd(x, w, b, EPS)
    g = Guarded(C, torch.float32, 3)
    dx = ext().layernorm_bwd(dy, x, w, mean, rstd, b is not None, ds, True, g.view(0),
                             None if b is None else g.view(1), g.view(2))[0]
    r32 = ln_torch(torch.float32, C, x, None, None, w, b, dy, ds)
    b16 = ln_torch(torch.bfloat16, C, x, None, None, w, b, dy, ds)
    check_act(tag, "y", y, r32["y"], b16["y"])
    check_act(tag, "dx", dx, r32["dx"], b16["dx"])
    check_sum(tag, "dw", g.view(0), r32["dw"])
    if b is not None:
        check_sum(tag, "db", g.view(1), r32["db"])
    else:
        assert bool((g.view(1) == SENTINEL).all())
    check_dx_colsum(tag, "dxs", g.view(2), dx, r32["dx"])
    assert g.intact()


def test_layernorm_first_unsupported_width_raises():
    """C = 2056 is 8-wide with 5 iterations: refused by check_launch, forward and backward."""
    C = 2056
    x, w, b = bf(9, C), norm_weight(C), bf(C, scale=0.1)
    with pytest.raises(RuntimeError, match="layernorm_fwd"):
        ops.layer_norm(x, w, b)
    with pytest.raises(RuntimeError, match="add_layernorm_fwd"):
        ops.add_layer_norm(x, bf(9, C), w, b)
    stat = torch.zeros(9, device=DEV)
    with pytest.raises(RuntimeError, match="layernorm_bwd"):
        ext().layernorm_bwd(bf(9, C), x, w, stat, stat + 1, True, None, False, None, None, None)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- RMSNorm
def rms_torch(dtype, C, x, r, w, dy, ds):
    xx, rr, ww = (None if t is None else t.detach().to(dtype).requires_grad_() for t in (x, r, w))
    s = xx.view_as(xx) if rr is None else xx + rr
    if dtype == torch.float32:
        y = s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + EPS) * ww
    else:
        y = F.rms_norm(s, (C,), ww, EPS)
    outs, gouts = [y], [dy.to(dtype)]
    if ds is not None:
        outs.append(s)
        gouts.append(ds.to(dtype))
    torch.autograd.backward(outs, gouts)
    return {"s": s.detach(), "y": y.detach(), "dx": xx.grad, "dw": ww.grad}


# 4101 rows: the forward's 4096 workgroups plus 5, and in the backward (1024 workgroups) five
# workgroups with 5 rows, the rest with 4: dw accumulates over rows in registers and the LDS
# reduction scratch is reused between rows.  C = 264: IT = 1 with 33 active threads; 2056:
# IT = 2, the second iteration with one active thread; 16384: IT = 8, the widest.
RMS_CASES = [(4101, 264), (4101, 2056), (1, 264), (3, 264), (7, 16384)]


def rms_inputs(rows, C, exact_sum=False):
    torch.manual_seed(rows * 4101 + C)
    rnd = grid if exact_sum else bf  # as in ln_inputs
    return dict(x=rnd(rows, C), r=rnd(rows, C), w=norm_weight(C), dy=bf(rows, C), ds=bf(rows, C))


@pytest.mark.parametrize("mode", ["plain", "add"])
@pytest.mark.parametrize("rows,C", RMS_CASES)
def test_rmsnorm_rows(rows, C, mode):
    """ops.rms_norm and ops.add_rms_norm (s returned, dres into the backward), bf16 dw."""
    t = rms_inputs(rows, C, exact_sum=mode == "add")
    tag = f"rms {mode} {rows}x{C}"
    x, w = t["x"].requires_grad_(), t["w"].requires_grad_()
    r = ds = None
    if mode == "plain":
        y = ops.rms_norm(x, w)
        y.backward(t["dy"])
    else:
        r, ds = t["r"].requires_grad_(), t["ds"]
        s, y = ops.add_rms_norm(x, r, w)
        torch.autograd.backward((s, y), (ds, t["dy"]))
    r32 = rms_torch(torch.float32, C, x, r, w, t["dy"], ds)
    b16 = rms_torch(torch.bfloat16, C, x, r, w, t["dy"], ds)
    check_act(tag, "y", y.detach(), r32["y"], b16["y"])
    check_act(tag, "dx", x.grad, r32["dx"], b16["dx"])
    if mode == "add":
        check_act(tag, "s", s.detach(), r32["s"], b16["s"])
        assert torch.equal(s.detach().float(), r32["s"])  # exact sums (rms_inputs)
        assert torch.equal(r.grad, x.grad)
    assert w.grad.dtype == torch.bfloat16
    check_sum(tag, "dw", w.grad, r32["dw"])
    report(f"{tag} stock", dw=rel_err(b16["dw"], r32["dw"]))


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,C", RMS_CASES)
def test_rmsnorm_bwd_arena_rows(rows, C, gdt):
    """C().rmsnorm_bwd with dres and dw_out an offset view inside a sentinel-filled buffer."""
    t = rms_inputs(rows, C)
    tag = f"rms arena {rows}x{C}"
    x, w, dy, ds = t["x"], t["w"], t["dy"], t["ds"]
    y, rstd = ext().rmsnorm_fwd(x, w, EPS)
    g = Guarded(C, gdt, 1)
    dx, dw = ext().rmsnorm_bwd(dy, x, w, rstd, ds, g.view(0))
    assert dw.data_ptr() == g.view(0).data_ptr()
    r32 = rms_torch(torch.float32, C, x, None, w, dy, ds)
    b16 = rms_torch(torch.bfloat16, C, x, None, w, dy, ds)
    check_act(tag, "y", y, r32["y"], b16["y"])
    check_act(tag, "dx", dx, r32["dx"], b16["dx"])
    check_sum(tag, "dw", g.view(0), r32["dw"])
    assert g.intact()


def test_rmsnorm_first_unsupported_width_raises():
    """C = 16392 would need IT = 9: refused by check_launch, forward and backward."""
    C = 16392
    x, w = bf(3, C), norm_weight(C)
    with pytest.raises(RuntimeError, match="rmsnorm_fwd"):
        ops.rms_norm(x, w)
    with pytest.raises(RuntimeError, match="add_rmsnorm_fwd"):
        ops.add_rms_norm(x, bf(3, C), w)
    with pytest.raises(RuntimeError, match="rmsnorm_bwd"):
        ext().rmsnorm_bwd(bf(3, C), x, w, torch.ones(3, device=DEV), None, None)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- switches
# ORION_COLSUM=2 (two-stage column sums) and ORION_LN_FWD1=0 (the per-row forward without a
# residual) are read once per process: each setting runs in a child on the same inputs.
# LayerNorm rows 5 / 130 / 4099 give 1 / 3 / 65 rows of partials, so the two-stage fold's 16
# splits are mostly empty, then 3 of 16 empty.
SWITCH_LN = [(rows, C) for rows in (5, 130, 4099) for C in (520, 768)]
SWITCH_RMS = (4101, 264)

CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[2])
from orion_amd.ops._ext import C, load_ext
load_ext(required=True)
out = {}
def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(torch.bfloat16)
for rows, Cc in %(ln)r:
    torch.manual_seed(rows + Cc)
    x, dy, ds = bf(rows, Cc), bf(rows, Cc), bf(rows, Cc)
    w, b = (1 + 0.1 * torch.randn(Cc, device="cuda")).to(torch.bfloat16), bf(Cc, scale=0.1)
    y, mean, rstd = C().layernorm_fwd(x, w, b, 1e-5)
    dx, dw, db, dxs = C().layernorm_bwd(dy, x, w, mean, rstd, True, ds, True, None, None, None)
    f32 = [torch.full((Cc,), -777.0, device="cuda") for _ in range(3)]
    dx2 = C().layernorm_bwd(dy, x, w, mean, rstd, True, ds, True, *f32)[0]
    out[f"ln{rows}x{Cc}"] = dict(x=x, dy=dy, ds=ds, w=w, b=b, y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db,
                                 dxs=dxs, dx2=dx2, dw32=f32[0], db32=f32[1], dxs32=f32[2])
rows, Cc = %(rms)r
torch.manual_seed(rows + Cc)
x, dy, ds = bf(rows, Cc), bf(rows, Cc), bf(rows, Cc)
w = (1 + 0.1 * torch.randn(Cc, device="cuda")).to(torch.bfloat16)
y, rstd = C().rmsnorm_fwd(x, w, 1e-5)
dx, dw = C().rmsnorm_bwd(dy, x, w, rstd, ds, None)
dw32 = torch.full((Cc,), -777.0, device="cuda")
dx2 = C().rmsnorm_bwd(dy, x, w, rstd, ds, dw32)[0]
out["rms"] = dict(x=x, dy=dy, ds=ds, w=w, y=y, rstd=rstd, dx=dx, dw=dw, dx2=dx2, dw32=dw32)
torch.cuda.synchronize()
torch.save({k: {n: t.cpu() for n, t in v.items()} for k, v in out.items()}, sys.argv[1])
""" % {"ln": SWITCH_LN, "rms": SWITCH_RMS}


def _child(tmp_path, tag, env_extra):
    out = tmp_path / f"{tag}.pt"
    env = {k: v for k, v in os.environ.items() if k not in ("ORION_COLSUM", "ORION_LN_FWD1", "ORION_LN_FWD1_BLOCKS")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), ROOT], env=env, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=True)


def test_colsum_two_stage_and_per_row_forward_switches(tmp_path):
    sw = _child(tmp_path, "switched", {"ORION_COLSUM": "2", "ORION_LN_FWD1": "0"})
    df = _child(tmp_path, "default", {})
    for key, d in df.items():  # the switches change the kernel and the fold order, not a row's math
        for n in ("x", "dy", "ds", "w", "y", "rstd", "dx", "dx2") + (("mean",) if "mean" in d else ()):
            assert torch.equal(sw[key][n], d[n]), (key, n)
    for rows, C in SWITCH_LN:
        d = {n: t.to(DEV) for n, t in sw[f"ln{rows}x{C}"].items()}
        tag = f"switches ln {rows}x{C}"
        r32 = ln_torch(torch.float32, C, d["x"], None, None, d["w"], d["b"], d["dy"], d["ds"])
        b16 = ln_torch(torch.bfloat16, C, d["x"], None, None, d["w"], d["b"], d["dy"], d["ds"])
        check_act(tag, "y", d["y"], r32["y"], b16["y"])
        check_act(tag, "dx", d["dx"], r32["dx"], b16["dx"])
        for n in ("dw", "db"):
            assert d[n].dtype == torch.bfloat16
            check_sum(tag, n, d[n], r32[n])
            check_sum(tag, n, d[n + "32"], r32[n])
        check_dx_colsum(tag, "dxs", d["dxs"], d["dx"], r32["dx"])
        check_dx_colsum(tag, "dxs", d["dxs32"], d["dx"], r32["dx"])
    d = {n: t.to(DEV) for n, t in sw["rms"].items()}
    tag = "switches rms %dx%d" % SWITCH_RMS
    r32 = rms_torch(torch.float32, SWITCH_RMS[1], d["x"], None, d["w"], d["dy"], d["ds"])
    b16 = rms_torch(torch.bfloat16, SWITCH_RMS[1], d["x"], None, d["w"], d["dy"], d["ds"])
    check_act(tag, "y", d["y"], r32["y"], b16["y"])
    check_act(tag, "dx", d["dx"], r32["dx"], b16["dx"])
    check_sum(tag, "dw", d["dw"], r32["dw"])
    check_sum(tag, "dw", d["dw32"], r32["dw"])


# --------------------------------------------------------------------------- RoPE
def _rope_bf16(x, cos, sin):
    """RoPE with stock PyTorch bf16 arithmetic (the tolerance baseline)."""
    d2 = x.shape[-1] // 2
    c = cos[: x.shape[1]].view(1, x.shape[1], 1, d2).to(x.dtype)
    s_ = sin[: x.shape[1]].view(1, x.shape[1], 1, d2).to(x.dtype)
    x1, x2 = x[..., :d2], x[..., d2:]
    return torch.cat([x1 * c - x2 * s_, x1 * s_ + x2 * c], dim=-1)


# (2, 2052, 33, 128): 1,083,456 groups of 16 elements against the 4096 x 256 = 1,048,576 threads
# of the capped grid, so 34,880 threads take a second group; (1, 5, 3, 64): D = 64, one
# partial workgroup.
@pytest.mark.parametrize("B,T,H,D,pos0", [(2, 2052, 33, 128, 7), (1, 5, 3, 64, 3)])
def test_rope_rows(B, T, H, D, pos0):
    torch.manual_seed(0)
    tag = f"rope {B}x{T}x{H}x{D}"
    qkv = bf(B, T, 3, H, D).requires_grad_()
    cos, sin = ref.rope_tables(T + pos0, D, device=DEV)
    y = ops.rope(qkv[:, :, 0], cos, sin, pos0)
    dy = bf(B, T, H, D)
    y.backward(dy)
    qr = qkv.detach()[:, :, 0].float().requires_grad_()
    yr = ref.rope(qr, cos[pos0:], sin[pos0:])
    yr.backward(dy.float())
    yb, gb = torch_bf16(lambda x_: _rope_bf16(x_, cos[pos0:], sin[pos0:]),
                        (qkv.detach()[:, :, 0].clone().requires_grad_(),), dy)
    check_act(tag, "y", y.detach(), yr.detach(), yb.detach())
    check_act(tag, "dq", qkv.grad[:, :, 0], qr.grad, gb[0])
    assert qkv.grad[:, :, 1:].abs().max().item() == 0


@pytest.mark.parametrize("B,T,H,D,pos0", [(2, 37, 5, 128, 2), (1, 5, 3, 64, 3)])
def test_rope_inplace_round_trip(B, T, H, D, pos0):
    """C().rope_ forward then inverse on the strided q|k view of a packed projection restores
    it to two bf16 roundings (the budget of the same round trip in stock bf16), and leaves v."""
    torch.manual_seed(1)
    tag = f"rope_ {B}x{T}x{H}x{D}"
    qkv = bf(B, T, 3 * H, D)
    orig = qkv.clone()
    cos, sin = ref.rope_tables(T + pos0 + 1, D, device=DEV)
    qk = qkv[:, :, :2 * H]
    assert not qk.is_contiguous()
    x32 = orig[:, :, :2 * H].float()
    fwd32 = ref.rope(x32, cos[pos0:], sin[pos0:])
    fwd16 = _rope_bf16(orig[:, :, :2 * H], cos[pos0:], sin[pos0:])
    ext().rope_(qk, cos, sin, pos0, 1.0)
    check_act(tag, "fwd", qk, fwd32, fwd16)
    assert torch.equal(qkv[:, :, 2 * H:], orig[:, :, 2 * H:])
    ext().rope_(qk, cos, sin, pos0, -1.0)
    back16 = _rope_bf16(fwd16, cos[pos0:], -sin[pos0:])
    check_act(tag, "round trip", qk, x32, back16)
    assert torch.equal(qkv[:, :, 2 * H:], orig[:, :, 2 * H:])


# --------------------------------------------------------------------------- column sums
# (4099, 520): 65 row blocks, the last with 3 rows, and a ragged column block (65 lanes' worth
# of 8 columns: the second block has one valid lane); (3, 8): fewer rows than waves, one lane.
SUM_CASES = [(4099, 520), (3, 8)]


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,C", SUM_CASES)
def test_colsum_rows(rows, C, gdt):
    torch.manual_seed(rows + C)
    m = bf(rows, C)
    want = m.double().sum(0).float()
    tag = f"colsum {rows}x{C}"
    if gdt == torch.bfloat16:
        got = ext().colsum(m, None)
        assert got.dtype == torch.bfloat16
        check_sum(tag, "sum", got, want)
        return
    g = Guarded(C, torch.float32, 1)
    got = ext().colsum(m, g.view(0))
    assert got.data_ptr() == g.view(0).data_ptr()
    check_sum(tag, "sum", g.view(0), want)
    assert g.intact()


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,C", SUM_CASES)
def test_bias_gelu_bwd_rows(rows, C, gdt):
    torch.manual_seed(rows + C + 1)
    x, b, dy = bf(rows, C), bf(C, scale=0.1), bf(rows, C)
    tag = f"bias_gelu_bwd {rows}x{C}"
    xr, br = (t.float().requires_grad_() for t in (x, b))
    F.gelu(xr + br, approximate="tanh").backward(dy.float())
    _, gb = torch_bf16(lambda x_, b_: F.gelu(x_ + b_, approximate="tanh"),
                       (x.clone().requires_grad_(), b.clone().requires_grad_()), dy)
    if gdt == torch.bfloat16:
        dx, db = ext().bias_gelu_bwd(dy, x, b, None)
        assert db.dtype == torch.bfloat16
    else:
        g = Guarded(C, torch.float32, 1)
        dx = ext().bias_gelu_bwd(dy, x, b, g.view(0))[0]
        db = g.view(0)
        assert g.intact()
    check_act(tag, "dx", dx, xr.grad, gb[0])
    check_sum(tag, "db", db, br.grad)
    report(f"{tag} stock", db=rel_err(gb[1], br.grad))

"""Attention backward forms on the GPU vs the fp32 PyTorch reference (ops/reference.py):
the fused kernel (fp32-atomic dQ, csrc/attention.hip: the fallback for operands beyond 2 GB,
forced here by flag 8) and the split kernels (dK/dV + dQ, no
atomics, csrc/attn_bwd_split.hip), determinism of the split form, the long-context
Llama-7B attention shape (T = 4096, GQA 32/8, D = 128) and Tk != T (bottom-right causal)."""
import math

import pytest
import torch

from orion_amd.ops import reference as ref
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"

FUSED, SPLIT = 8, 4  # attn_bwd flags (csrc/bindings.cpp): 8 = the >2 GB fallback, forced


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _C():
    from orion_amd.ops._ext import C, load_ext
    load_ext(required=True)
    return C()


def _run(q, k, v, do, causal, flags):
    C = _C()
    scale = 1.0 / math.sqrt(q.shape[-1])
    o, lse = C.attn_fwd(q, k, v, causal, scale)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    C.attn_bwd(do, q, k, v, o, lse, causal, scale, dq, dk, dv, flags)
    return o, dq, dk, dv


def _ref(q, k, v, do, causal):
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    o = ref.attention(qr, kr, vr, causal).float()
    o.backward(do.float())
    return o, qr.grad, kr.grad, vr.grad


def _sdpa_bf16(q, k, v, do, causal):
    """The tolerance baseline: F.scaled_dot_product_attention on the bf16 (B, T, H, D)
    inputs (GQA by repeat; Tk > T causal as bottom-right, like the kernels), bf16 grads."""
    Tq, Tk = q.shape[1], k.shape[1]
    qb, kb, vb = (t.detach().clone().requires_grad_() for t in (q, k, v))
    rep = q.shape[2] // k.shape[2]
    kk, vv = (kb.repeat_interleave(rep, 2), vb.repeat_interleave(rep, 2)) if rep > 1 else (kb, vb)
    mask = None
    if causal and Tk != Tq:
        mask = torch.ones(Tq, Tk, dtype=torch.bool, device=q.device).tril(Tk - Tq)
    o = torch.nn.functional.scaled_dot_product_attention(
        qb.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2), attn_mask=mask,
        is_causal=causal and Tk == Tq).transpose(1, 2)
    o.backward(do)
    return o, qb.grad, kb.grad, vb.grad


def _check(got, want, base):
    for name, a, b, c in zip(("o", "dq", "dk", "dv"), got, want, base):
        within_bf16_budget(name, a, b, c)


def _inputs(B, T, Tk, Hq, Hkv, D, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mk = lambda *s: torch.randn(*s, device=DEV, dtype=torch.bfloat16, generator=g)
    return mk(B, T, Hq, D), mk(B, Tk, Hkv, D), mk(B, Tk, Hkv, D), mk(B, T, Hq, D)


@pytest.mark.parametrize("form", [FUSED, SPLIT])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_backward_forms_match_reference(form, D, causal):
    q, k, v, do = _inputs(2, 320, 320, 4, 2, D)
    got = _run(q, k, v, do, causal, form)
    want = _ref(q, k, v, do, causal)
    _check(got, want, _sdpa_bf16(q, k, v, do, causal))


@pytest.mark.parametrize("D", [64, 128])
def test_split_backward_is_deterministic(D):
    q, k, v, do = _inputs(2, 512, 512, 8, 2, D, seed=3)
    a = _run(q, k, v, do, True, SPLIT)
    b = _run(q, k, v, do, True, SPLIT)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


def test_deterministic_switch_routes_ops_to_split(monkeypatch):
    from orion_amd import ops
    from orion_amd.ops import flash_attn
    monkeypatch.setenv("ORION_DETERMINISTIC", "1")
    assert flash_attn._bwd_flags() == SPLIT
    q, k, v, do = _inputs(1, 256, 256, 4, 4, 64, seed=5)
    grads = []
    for _ in range(2):
        qq, kk, vv = (t.clone().requires_grad_() for t in (q, k, v))
        ops.attention(qq, kk, vv, causal=True).backward(do)
        grads.append((qq.grad, kk.grad, vv.grad))
    for x, y in zip(*grads):
        assert torch.equal(x, y)


@pytest.mark.parametrize("form", [FUSED, SPLIT])
def test_long_context_llama7b_attention_shape(form):
    """BASELINE config 4's attention: T = 4096, 32 query heads on 8 KV heads, D = 128."""
    q, k, v, do = _inputs(1, 4096, 4096, 32, 8, 128, seed=1)
    got = _run(q, k, v, do, True, form)
    want = _ref(q, k, v, do, True)
    _check(got, want, _sdpa_bf16(q, k, v, do, True))


@pytest.mark.parametrize("form", [FUSED, SPLIT])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_cross_length_tk_ne_t(form, D, causal):
    """Tk > T (a query block at the end of a longer key sequence, causal bottom-right)."""
    q, k, v, do = _inputs(2, 192, 328, 4, 2, D, seed=2)
    got = _run(q, k, v, do, causal, form)
    want = _ref(q, k, v, do, causal)
    _check(got, want, _sdpa_bf16(q, k, v, do, causal))


def test_deterministic_training_steps_are_bitwise_reproducible(monkeypatch):
    """ORION_DETERMINISTIC=1 (ops/determinism.py): two fresh runs of three full training
    steps (GPT-2 shape, 2 layers: split attention backward, in-tree GEMMs, fixed-order
    reductions, fused AdamW) end with bit-identical losses and weights."""
    from orion_amd.models.gpt2 import build_gpt2
    from orion_amd.train.engine import Trainer, OptimConfig
    monkeypatch.setenv("ORION_DETERMINISTIC", "1")
    g = torch.Generator(device=DEV).manual_seed(7)
    batches = [(torch.randint(0, 50257, (4, 256), device=DEV, generator=g),
                torch.randint(0, 50257, (4, 256), device=DEV, generator=g)) for _ in range(3)]
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        m = build_gpt2("gpt2", n_layer=2, block_size=256).to(DEV)
        tr = Trainer(m, OptimConfig(warmup_iters=1, lr_decay_iters=10, learning_rate=1e-3))
        losses = [float(tr.step([b])) for b in batches]
        runs.append((losses, tr.arena.params.clone(), tr.opt.master.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_forward_deferred_rescale_growing_scores(D, causal):
    """The forward keeps a stale row max until a tile raises it by more than 2^8
    (csrc/attention.hip): scores that grow along the keys (small steps, deferred) with
    occasional spikes (large steps, rescaled) against the fp32 reference."""
    g = torch.Generator(device=DEV).manual_seed(11)
    B, T, H = 1, 1024, 2
    q = torch.randn(B, T, H, D, device=DEV, generator=g)
    k = torch.randn(B, T, H, D, device=DEV, generator=g)
    ramp = 0.2 + 2.5 * torch.arange(T, device=DEV).float() / T
    k = k * ramp.view(1, T, 1, 1)
    k[:, ::97] *= 6.0
    v = torch.randn(B, T, H, D, device=DEV, generator=g)
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    o, _ = _C().attn_fwd(q, k, v, causal, 1.0 / math.sqrt(D))
    want = ref.attention(q.float(), k.float(), v.float(), causal)
    base = torch.nn.functional.scaled_dot_product_attention(
        q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=causal).transpose(1, 2)
    within_bf16_budget("o", o, want, base)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("case", ["overflow", "underflow", "some_rows"])
def test_attention_extreme_scores(D, causal, case):
    """Score ranges that overflow / underflow exp2 against a fixed reference: overflow: scores
    up to ~+400 (log2 units); underflow: every score shifted by ~-140 / -195 (a shift common
    to a query's keys: the softmax is unchanged); some_rows: only a few query rows extreme.
    Forward and backward (which reads the lse) against the fp32 reference, budgeted by SDPA
    in bf16.  (Round 4 measured a forward without the running max -- exp2 against 0, the
    reference path only for out-of-range blocks -- against these; it was no faster and was
    not kept: docs/PERFORMANCE.md.)"""
    g = torch.Generator(device=DEV).manual_seed(5)
    B, T, H = 1, 512, 2
    q = torch.randn(B, T, H, D, device=DEV, generator=g)
    k = torch.randn(B, T, H, D, device=DEV, generator=g)
    v = torch.randn(B, T, H, D, device=DEV, generator=g)
    do = torch.randn(B, T, H, D, device=DEV, generator=g)
    if case == "overflow":
        q = q * 6.0
        k = k * 6.0
    elif case == "underflow":
        # q . k gains -(16 * 0.75 * D) on every key: -768 / -1536 raw, ~-140 / -195 log2 units
        q[..., 0] = 16.0
        k[..., 0] = -0.75 * D
    else:
        q[:, ::37] *= 12.0
    q, k, v, do = (t.to(torch.bfloat16) for t in (q, k, v, do))
    _check(_run(q, k, v, do, causal, SPLIT), _ref(q, k, v, do, causal), _sdpa_bf16(q, k, v, do, causal))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("form", [0, SPLIT, FUSED])
def test_backward_inverse_rope_forms(D, form):
    """attn_bwd with rope tables returns dq / dk w.r.t. the unrotated q / k: the split kernels
    rotate at their stores, the fused form runs the rope kernel after.  Both equal the plain
    backward followed by the separate inverse rope launch (to bf16 rounding of the stores)."""
    C = _C()
    B, T, H, pos0 = 2, 256, 4, 5
    q, k, v, do = _inputs(B, T, T, H, H, D, seed=9)
    cos, sin = ref.rope_tables(T + pos0, D, device=DEV)
    scale = 1.0 / math.sqrt(D)
    o, lse = C.attn_fwd(q, k, v, True, scale)
    outs = []
    for rope in (False, True):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        if rope:
            C.attn_bwd(do, q, k, v, o, lse, True, scale, dq, dk, dv, form, None, cos, sin, pos0)
        else:
            C.attn_bwd(do, q, k, v, o, lse, True, scale, dq, dk, dv, form)
            C.rope_(dq, cos, sin, pos0, -1.0)
            C.rope_(dk, cos, sin, pos0, -1.0)
        outs.append((dq, dk, dv))
    for a, b in zip(*outs):
        assert rel_err(a, b) < 6e-3, rel_err(a, b)


@pytest.mark.parametrize("env", [{"ORION_ATTN_FWD": "v2"}])
def test_forward_kernel_variants_match_reference(env):
    """The fallback forward kernel (attention.hip's 64-bit-addressed one, taken when offsets
    pass 2 GB; forced here) on causal / full, D 64 / 128, GQA and ragged T.  The selection is
    read once per process, so it runs in a child process (scripts/attn_fwd_diff.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "attn_fwd_diff.py")],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if "max err" in ln]
    assert len(lines) == 7, r.stdout
    assert all("bad rows 0 /" in ln for ln in lines), r.stdout


VARIANT_SWITCHES = {"ORION_ATTN_FWD": "v3", "ORION_ATTN_DQ": "v3", "ORION_ATTN_DELTA": "pass"}


def _variant_switch_cases():
    """Forward and backward through the kernels the switches select.  T = 160: two 128-row query
    tiles and three 64-key tiles, the last of each partial."""
    for D in (64, 128):
        for causal in (True, False):
            q, k, v, do = _inputs(2, 160, 160, 4, 2, D)
            _check(_run(q, k, v, do, causal, 0), _ref(q, k, v, do, causal), _sdpa_bf16(q, k, v, do, causal))
    # packed QKV with the bias output (MHA, D = 64, T % 32 == 0: column sums inside the kernels)
    B, T, H, D, causal = 2, 160, 2, 64, True
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn(B, T, 3 * H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, T, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:2 * H], qkv[:, :, 2 * H:]
    scale = 1.0 / math.sqrt(D)
    o, lse = _C().attn_fwd(q, k, v, causal, scale)
    d = torch.empty_like(qkv)
    db = torch.full((3 * H * D,), float("nan"), device=DEV, dtype=torch.float32)
    _C().attn_bwd(do, q, k, v, o, lse, causal, scale, d[:, :, :H], d[:, :, H:2 * H], d[:, :, 2 * H:], 0, db)
    want, base = _ref(q, k, v, do, causal), _sdpa_bf16(q, k, v, do, causal)
    _check((o, d[:, :, :H], d[:, :, H:2 * H], d[:, :, 2 * H:]), want, base)
    colsum = lambda grads: torch.cat(list(grads), dim=2).reshape(B * T, -1).float().sum(0)
    within_bf16_budget("db", db, colsum(want[1:]), colsum(base[1:]))
    torch.cuda.synchronize()
    print("variant switches ok")


def test_variant_switches_match_reference():
    """ORION_ATTN_FWD=v3, ORION_ATTN_DQ=v3 and ORION_ATTN_DELTA=pass (the forms the defaults replaced)
    against the fp32 reference.  The switches are read once per process, so the cases run in a child
    process: this module as a script."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {**os.environ, **VARIANT_SWITCHES,
           "PYTHONPATH": os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p)}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "variant switches ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("form", [0, SPLIT, FUSED])
@pytest.mark.parametrize("D,Hq,Hkv,T", [(64, 4, 4, 256), (64, 4, 4, 200), (64, 4, 2, 256), (128, 4, 2, 256)])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_packed_qkv_bias_grad_matches_colsum(form, D, Hq, Hkv, T, causal, out_dtype):
    """attn_bwd(..., bias_grad=out) on a packed (B, T, Hq + 2 Hkv, D) dQKV: the QKV bias
    gradient colsum(dQKV) -- from the split kernels' fp32 per-32-token column sums (MHA,
    D = 64, T % 32 == 0: dQ's from the dQ kernel, dK's = 0 and dV's = colsum(dO) from the
    delta pass), from a column sum of the packed bf16 dQKV otherwise -- matches the fp32
    column sum of the reference gradients; dQKV equals the call without the bias output."""
    B = 2
    C = _C()
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn(B, T, Hq + 2 * Hkv, D, device=DEV, dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, T, Hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:]
    scale = 1.0 / math.sqrt(D)
    o, lse = C.attn_fwd(q, k, v, causal, scale)
    d_plain, d_bias = torch.empty_like(qkv), torch.empty_like(qkv)
    views = lambda d: (d[:, :, :Hq], d[:, :, Hq:Hq + Hkv], d[:, :, Hq + Hkv:])
    C.attn_bwd(do, q, k, v, o, lse, causal, scale, *views(d_plain), form)
    db = torch.full(((Hq + 2 * Hkv) * D,), float("nan"), device=DEV, dtype=out_dtype)
    C.attn_bwd(do, q, k, v, o, lse, causal, scale, *views(d_bias), form, db)
    assert rel_err(d_bias, d_plain) < 1e-2
    _, dq, dk, dv = _ref(q, k, v, do, causal)
    want = torch.cat([dq, dk, dv], dim=2).reshape(B * T, -1).sum(0)
    assert torch.isfinite(db.float()).all()
    _, bq, bk, bv = _sdpa_bf16(q, k, v, do, causal)
    base = torch.cat([bq, bk, bv], dim=2).reshape(B * T, -1).float().sum(0)
    within_bf16_budget("db", db, want, base)


def test_gpt2_qkv_bias_grad_through_attention_matches_reference():
    """GPT-2's attention block (ops.linear_attention_qkv): the c_attn bias gradient summed
    inside the attention backward equals the autograd gradient of the fp32 reference."""
    from orion_amd import ops
    _C()
    torch.manual_seed(0)
    B, T, Cm, H = 2, 128, 256, 4
    x = torch.randn(B, T, Cm, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn(3 * Cm, Cm, device=DEV) * 0.05).to(torch.bfloat16).requires_grad_()
    b = (torch.randn(3 * Cm, device=DEV) * 0.1).to(torch.bfloat16).requires_grad_()
    y = ops.linear_attention_qkv(x, w, b, H)
    gy = torch.randn_like(y)
    y.backward(gy)
    xr, wr, br = (t.detach().float().requires_grad_() for t in (x, w, b))
    yr = ref.attention_qkv(torch.nn.functional.linear(xr, wr, br), H, True)
    yr.backward(gy.float())
    xb, wb, bb = (t.detach().clone().requires_grad_() for t in (x, w, b))
    qkv = torch.nn.functional.linear(xb, wb, bb).view(B, T, 3, H, Cm // H)
    ob = torch.nn.functional.scaled_dot_product_attention(
        *(t.transpose(1, 2) for t in qkv.unbind(2)), is_causal=True).transpose(1, 2).reshape(B, T, Cm)
    ob.backward(gy)
    within_bf16_budget("y", y, yr, ob)
    for name, a, r, c in (("x", x.grad, xr.grad, xb.grad), ("w", w.grad, wr.grad, wb.grad),
                          ("b", b.grad, br.grad, bb.grad)):
        assert a is not None
        within_bf16_budget(name, a, r, c)


@pytest.mark.parametrize("B,T,Hq,Hkv,pos0", [(2, 256, 4, 2, 0), (1, 300, 2, 2, 7)])
def test_fused_qkv_rope_attention_node(B, T, Hq, Hkv, pos0, monkeypatch):
    """Round 6: Llama's projection + RoPE + attention as one node (the rotation in the
    projection GEMM's epilogue, ops.linear_rope_attention) -- output and the gradients of x
    and W against the fp32 reference (projection, rope, attention in fp32), within the budget
    of the unfused HIP path (projection, rope pass, attention) on the same bf16 inputs."""
    from orion_amd import ops
    from orion_amd.ops import flash_attn as FA
    D, Cm = 128, 256
    g = torch.Generator(device=DEV).manual_seed(T + Hq)
    x = (torch.randn(B, T, Cm, device=DEV, generator=g) * 0.5).bfloat16()
    w = (torch.randn((Hq + 2 * Hkv) * D, Cm, device=DEV, generator=g) * 0.1).bfloat16()
    do = torch.randn(B, T, Hq, D, device=DEV, generator=g).bfloat16()
    cos, sin = ref.rope_tables(T + pos0 + 4, D, device=DEV)
    assert FA.qkv_rope_eligible(x, w, Hq, Hkv, cos)

    def run(fused):
        monkeypatch.setattr(FA, "_QKV_ROPE", fused)
        xx, ww = x.clone().requires_grad_(), w.clone().requires_grad_()
        o = ops.linear_rope_attention(xx, ww, Hq, Hkv, cos, sin, pos0)
        o.backward(do)
        return o.detach(), xx.grad, ww.grad

    got, base = run(True), run(False)
    xr, wr = x.float().requires_grad_(), w.float().requires_grad_()
    qkv = (xr @ wr.t()).view(B, T, Hq + 2 * Hkv, D)
    c, s = cos[pos0:pos0 + T], sin[pos0:pos0 + T]
    q = ref.rope(qkv[:, :, :Hq], c, s)
    k = ref.rope(qkv[:, :, Hq:Hq + Hkv], c, s)
    o = ref.attention(q, k, qkv[:, :, Hq + Hkv:], True).float()
    o.backward(do.float())
    for name, a, b, cc in zip(("o", "dx", "dw"), got, (o.detach(), xr.grad, wr.grad), base):
        within_bf16_budget(name, a, b, cc)


if __name__ == "__main__":  # the child process of test_variant_switches_match_reference
    _variant_switch_cases()

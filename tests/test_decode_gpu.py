"""The generation kernels of csrc/attn_decode.hip on the GPU: split-KV single-query attention
and the cache append, against the fp32 reference with the budget of tests/tolerance.py
(err(HIP vs fp32) <= 2 x err(stock bf16 vs fp32) + 1e-3; the baseline is SDPA on each row's valid
slice, or ``ref.rope`` on bf16 for the append), and ``forward_cached`` of the models."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from orion_amd import ops
from orion_amd.models.gpt2 import build_gpt2
from orion_amd.models.llama import build_llama
from orion_amd.ops import reference as ref
from orion_amd.ops.decode import attention_decode_torch
from tolerance import within_bf16_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")

TMAX = 320
LENS = [1, 63, 65, 300]
HEADS = [(4, 4), (8, 2), (16, 2), (12, 1)]  # G = 1, 4, 8 and 12 (the 8-row group loops)


def _decode_inputs(D, Hq, Hkv, seed=0, lens=LENS, tmax=TMAX, q_scale=1.0):
    """q, caches whose positions >= the row's length are bf16 NaN, device lengths."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(lens)
    q = (torch.randn(B, Hq, D, device=DEV, generator=g) * q_scale).to(torch.bfloat16)
    kc = torch.randn(B, tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, tmax, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lens):
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    return q, kc, vc, torch.tensor(lens, dtype=torch.int32, device=DEV)


_CASES = {}


def _case(D, Hq, Hkv):
    """Inputs, fp32 reference and SDPA-bf16 baseline of one sweep shape, computed once."""
    key = (D, Hq, Hkv)
    if key not in _CASES:
        q, kc, vc, lens = _decode_inputs(D, Hq, Hkv)
        want = ref.attention_decode(q.float(), kc.float(), vc.float(), lens)
        _CASES[key] = (q, kc, vc, lens, want, attention_decode_torch(q, kc, vc, lens))
    return _CASES[key]


@pytest.mark.parametrize("splits", [0, 1, 3, 8])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_sweep(D, Hq, Hkv, splits):
    """Ragged lengths with NaN beyond them; 8 splits of 320 keys leave rows 0-2 with empty splits."""
    q, kc, vc, lens, want, base = _case(D, Hq, Hkv)
    o = ops.attention_decode(q, kc, vc, lens, splits=splits)
    assert o.shape == (len(LENS), Hq, D) and o.dtype == torch.bfloat16
    assert torch.isfinite(o).all()
    e, b = within_bf16_budget("o", o, want, base)
    print(f"D{D} H{Hq}/{Hkv} splits {splits}: err {e:.3e} baseline {b:.3e}")


@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 4), (128, 8, 2)])
def test_decode_strided_inputs(D, Hq, Hkv):
    """k / v as views into one (B, Tmax, 2, Hkv, D) buffer, q a view of a packed projection."""
    q, kc, vc, lens, want, base = _case(D, Hq, Hkv)
    B = q.shape[0]
    kv = torch.stack((kc, vc), dim=2)  # (B, Tmax, 2, Hkv, D)
    packed = torch.randn(B, 1, Hq + 2 * Hkv, D, device=DEV).to(torch.bfloat16)
    packed[:, 0, :Hq] = q
    qs, ks, vs = packed[:, 0, :Hq], kv[:, :, 0], kv[:, :, 1]
    assert not ks.is_contiguous() and qs.stride(0) != Hq * D
    for splits in (1, 3):
        o = ops.attention_decode(qs, ks, vs, lens, splits=splits)
        within_bf16_budget("o strided", o, want, base)
        assert torch.equal(o, ops.attention_decode(q, kc, vc, lens, splits=splits))


@pytest.mark.parametrize("splits", [1, 3])
def test_decode_extreme_scores(splits):
    """q large enough that the softmax saturates on one key, and one key at -large."""
    D, Hq, Hkv = 64, 4, 2
    q, kc, vc, lens = _decode_inputs(D, Hq, Hkv, seed=1, q_scale=40.0)
    kc[:, 0] = (-100.0 * q[:, ::2].float()).to(torch.bfloat16)  # score ~ -100 |q|^2 / sqrt(D) for its heads
    want = ref.attention_decode(q.float(), kc.float(), vc.float(), lens)
    base = attention_decode_torch(q, kc, vc, lens)
    o = ops.attention_decode(q, kc, vc, lens, splits=splits)
    assert torch.isfinite(o).all()
    within_bf16_budget("o extreme", o, want, base)


@pytest.mark.parametrize("splits", [0, 1, 3])
def test_decode_length_edges(splits):
    D, Hq, Hkv = 64, 8, 2
    q, kc, vc, _ = _decode_inputs(D, Hq, Hkv, seed=2, lens=[TMAX] * 3)
    zero = torch.zeros(3, dtype=torch.int32, device=DEV)
    o = ops.attention_decode(q, kc, vc, zero, splits=splits)
    assert torch.all(o == 0), "length 0 must give zeros"
    full = torch.full((3,), TMAX, dtype=torch.int32, device=DEV)
    over = torch.tensor([TMAX + 1, TMAX + 1000, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.attention_decode(q, kc, vc, over, splits=splits),
                       ops.attention_decode(q, kc, vc, full, splits=splits))


def test_decode_is_deterministic():
    q, kc, vc, lens, _, _ = _case(128, 16, 2)
    a = ops.attention_decode(q, kc, vc, lens, splits=3)
    b = ops.attention_decode(q, kc, vc, lens, splits=3)
    assert torch.equal(a, b)


def test_decode_refuses_bad_inputs():
    q, kc, vc, lens, _, _ = _case(64, 4, 4)
    with pytest.raises(RuntimeError):
        ops.attention_decode(q, kc, vc, lens.cpu())
    with pytest.raises(RuntimeError):
        ops.attention_decode(q[:, :3], kc, vc[:, :, :2], lens)
    with pytest.raises(RuntimeError):
        ops.attention_decode(q[..., :32], kc[..., :32], vc[..., :32], lens)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.attention_decode(q.clone().requires_grad_(), kc, vc, lens)


SENTINEL = 7.0


@pytest.mark.parametrize("with_rope", [False, True], ids=["copy", "rope"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5])
def test_kv_append(T, D, with_rope):
    """Strided k / v / q views of a packed projection, ragged lengths, one row running past Tmax."""
    B, Hq, Hkv, Tmax = 3, 4, 2, 24
    lens_h = [0, 7, Tmax - T + 2]  # the last row: T - 2 tokens fit (none at T = 1)
    g = torch.Generator(device=DEV).manual_seed(T * 1000 + D)
    packed = torch.randn(B, T, Hq + 2 * Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    q, k_new, v_new = packed[:, :, :Hq], packed[:, :, Hq:Hq + Hkv], packed[:, :, Hq + Hkv:]
    kv = torch.full((B, Tmax, 2, Hkv, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    kc, vc = kv[:, :, 0], kv[:, :, 1]
    lens = torch.tensor(lens_h, dtype=torch.int32, device=DEV)
    cos, sin = ref.rope_tables(Tmax + 8, D, device=DEV)
    q_rot = ops.kv_append(k_new, v_new, kc, vc, lens, **(dict(q=q, cos=cos, sin=sin) if with_rope else {}))
    assert lens.tolist() == lens_h

    def bits(t):
        return t.contiguous().view(torch.int16)

    for b, p0 in enumerate(lens_h):
        n = max(0, min(T, Tmax - p0))
        outside = torch.ones(Tmax, dtype=torch.bool, device=DEV)
        outside[p0:p0 + n] = False
        assert torch.all(kc[b, outside] == SENTINEL) and torch.all(vc[b, outside] == SENTINEL)
        if n == 0:
            continue
        assert torch.equal(bits(vc[b, p0:p0 + n]), bits(v_new[b, :n]))
        if not with_rope:
            assert torch.equal(bits(kc[b, p0:p0 + n]), bits(k_new[b, :n]))
            continue
        for name, got, x in (("k", kc[b:b + 1, p0:p0 + n], k_new[b:b + 1, :n]),
                             ("q", q_rot[b:b + 1, :n], q[b:b + 1, :n])):
            want = ref.rope(x.float(), cos[p0:], sin[p0:])
            within_bf16_budget(f"{name} row {b}", got, want, ref.rope(x, cos[p0:], sin[p0:]))
        assert torch.all(q_rot[b, n:] == 0)
    if with_rope:
        assert q_rot.shape == (B, T, Hq, D) and q_rot.is_contiguous()
    else:
        assert q_rot is None


def _gpu_copy(model):
    m = copy.deepcopy(model).to(DEV).to(torch.bfloat16)
    for name, buf in m.named_buffers():
        if name.startswith("rope_"):
            buf.data = buf.data.float()
    return m.eval()


MODELS = {
    "gpt2-tiny": lambda: build_gpt2("gpt2-tiny"),
    "llama-tiny": lambda: build_llama("llama-tiny"),                                  # D 64, GQA 4/2
    "llama-tiny-d128": lambda: build_llama("llama-tiny", dim=512, n_heads=4, n_kv_heads=1),  # D 128, G 4
}


@pytest.mark.parametrize("name", list(MODELS))
def test_models_forward_cached_teacher_forced(name):
    """B 2, prompt 37, 12 decode steps: every step's logits against the CPU fp32 uncached forward,
    budgeted by the same model's full forward on the GPU with stock PyTorch ops."""
    Bm, prompt, steps = 2, 37, 12
    torch.manual_seed(0)
    cpu = MODELS[name]().eval()
    gpu = _gpu_copy(cpu)
    cpu = copy.deepcopy(gpu).float().cpu()  # the bf16-rounded weights, in fp32
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, cpu.config.vocab_size, (Bm, prompt + steps), generator=g)
    dtoks = toks.to(DEV)
    prefixes = range(prompt, prompt + steps + 1)
    with torch.no_grad():
        want = {n: cpu(toks[:, :n])[0][:, -1] for n in prefixes}
        prev = ops.backend()
        try:
            ops.set_backend("torch")
            base = {n: gpu(dtoks[:, :n])[0][:, -1] for n in prefixes}
        finally:
            ops.set_backend(prev)
    cache = gpu.new_cache(Bm, prompt + steps)
    logits = gpu.forward_cached(dtoks[:, :prompt], cache)
    within_bf16_budget("prefill logits", logits.cpu(), want[prompt], base[prompt].cpu())
    for n in range(prompt, prompt + steps):
        logits = gpu.forward_cached(dtoks[:, n:n + 1], cache)
        within_bf16_budget(f"logits after {n + 1} tokens", logits.cpu(), want[n + 1], base[n + 1].cpu())
    assert cache.pos == prompt + steps and cache.lens.tolist() == [prompt + steps] * Bm


def test_generate_with_cache_on_the_gpu():
    torch.manual_seed(0)
    gpu = _gpu_copy(build_llama("llama-tiny", max_seq_len=48))
    prompt = torch.randint(0, gpu.config.vocab_size, (2, 40), device=DEV)
    out = gpu.generate(prompt, 12, top_k=50, use_cache=True)  # 9 cached tokens, 3 past the window
    assert out.shape == (2, 52) and torch.equal(out[:, :40], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < gpu.config.vocab_size


DEBUG_SCRIPT = r"""
import math, torch
from orion_amd.ops._ext import C, load_ext, EXT_PATH
from orion_amd.ops.reference import rope_tables
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
load_ext(required=True)
ops = C()
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
B, T, Hq, Hkv, D, Tmax = 3, 5, 12, 1, 128, 200
kc, vc = r(B, Tmax, Hkv, D), r(B, Tmax, Hkv, D)
lens = torch.tensor([0, 131, 198], dtype=torch.int32, device="cuda")
cos, sin = rope_tables(Tmax, D, device="cuda")
packed = r(B, T, Hq + 2 * Hkv, D)
q = ops.kv_append(packed[:, :, Hq:Hq + Hkv], packed[:, :, Hq + Hkv:], kc, vc, lens, packed[:, :, :Hq], cos, sin)
ops.kv_append(packed[:, :, Hq:Hq + Hkv], packed[:, :, Hq + Hkv:], kc, vc, lens, None, None, None)
for splits in (0, 1, 3):
    o = ops.attn_decode(q[:, 0], kc, vc, lens + T, 1 / math.sqrt(D), splits)
torch.cuda.synchronize()
assert torch.isfinite(o).all()
print("debug build ok")
"""


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_decode_kernels_pass_their_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

"""Fused-op layer: HIP/CDNA4 kernels on the GPU, plain PyTorch on the CPU.

Every public function here dispatches on the device of its inputs:

* CPU tensors -> :mod:`orion_amd.ops.reference` (the numerics oracle);
* GPU tensors -> the hand-written gfx950 kernels in ``csrc/`` (loaded from the
  in-tree ``orion_amd/_C*.so``), wrapped in ``torch.autograd.Function``s.

There is deliberately no silent fallback on the GPU: if the extension is not
built, a GPU call raises.  ``ORION_AMD_OPS=torch`` (or :func:`set_backend`)
selects stock PyTorch GPU ops instead; it exists only so ``bench.py`` can
measure the stock-PyTorch baseline on the same model.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import reference as ref
from ._ext import ext_available, load_ext
from .fp8 import Fp8Weight, quantize_fp8, quantize_kv_fp8
# loaded here, before ``def linear`` below binds the name: the first import of a submodule
# sets it as an attribute of the package, which later would replace the function
from .linear import linear_hip
from .mxfp4 import Mxfp4Weight, quantize_mxfp4

_BACKEND = os.environ.get("ORION_AMD_OPS", "hip")


def set_backend(name: str):
    global _BACKEND
    assert name in ("hip", "torch"), name
    _BACKEND = name


def backend() -> str:
    return _BACKEND


def _gpu(t: torch.Tensor) -> str | None:
    """Return 'hip' / 'torch' for GPU tensors, None for CPU tensors."""
    if not t.is_cuda:
        return None
    if _BACKEND == "hip":
        load_ext(required=True)
        return "hip"
    return "torch"


# --------------------------------------------------------------------------- norms
def layer_norm(x, weight, bias, eps=1e-5):
    b = _gpu(x)
    if b == "hip":
        from .layernorm import layer_norm_hip
        return layer_norm_hip(x, weight, bias, eps)
    if b == "torch":
        return F.layer_norm(x, (x.shape[-1],), weight.to(x.dtype),
                            None if bias is None else bias.to(x.dtype), eps)
    return ref.layer_norm(x, weight, bias, eps)


def add_layer_norm(x, r, weight, bias, eps=1e-5, r_bias=None):
    """Fused residual add + LayerNorm: (s, y) = (x + r [+ r_bias], LayerNorm(s)).
    ``r_bias`` is the bias of the branch's output projection (fused here)."""
    b = _gpu(x)
    if b == "hip":
        from .layernorm import add_layer_norm_hip
        return add_layer_norm_hip(x, r, weight, bias, eps, r_bias)
    if r_bias is not None:
        r = r + r_bias.to(r.dtype)
    s = x + r
    return s, layer_norm(s, weight, bias, eps)


def linear_residual_layer_norm(x, inp, w, rb, ln_w, ln_b, eps=1e-5):
    """A residual site with the branch's output projection: (s, y) = (x + inp W^T + rb,
    LayerNorm(s)).  On the GPU one hipBLASLt GEMM with the bias and the old stream in its
    epilogue, then a LayerNorm that reads only s (ops/residual.py); elsewhere the projection
    then :func:`add_layer_norm`."""
    if _gpu(x) == "hip":
        from .residual import eligible, linear_residual_layer_norm_hip
        if eligible(x, inp, w, rb):
            return linear_residual_layer_norm_hip(x, inp, w, rb, ln_w, ln_b, eps)
    return add_layer_norm(x, linear(inp, w, None), ln_w, ln_b, eps, r_bias=rb)


def mlp_residual_layer_norm(x, h, w_fc, b_fc, w_proj, b_proj, ln_w, ln_b, eps=1e-5):
    """The MLP residual site: (s, y) = (x + mlp(h), LayerNorm(s)) with GPT-2's MLP; on the GPU
    the fused MLP whose fc2 GEMM does the residual add (ops/residual.py)."""
    if _gpu(x) == "hip":
        from .residual import mlp_eligible, mlp_residual_layer_norm_hip
        if mlp_eligible(x, h, w_fc, w_proj, b_proj):
            return mlp_residual_layer_norm_hip(x, h, w_fc, b_fc, w_proj, b_proj, ln_w, ln_b, eps)
    return add_layer_norm(x, mlp(h, w_fc, b_fc, w_proj, None), ln_w, ln_b, eps, r_bias=b_proj)


def linear_residual_rms_norm(x, inp, w, nw, eps=1e-5):
    """Llama's attention site: (s, y) = (x + inp W^T, RMSNorm(s)); on the GPU the o_proj GEMM adds
    the residual stream in its epilogue and the RMSNorm reads only s (ops/residual.py)."""
    if _gpu(x) == "hip":
        from .residual import eligible, linear_residual_rms_norm_hip
        if eligible(x, inp, w, None, need_bias=False):
            return linear_residual_rms_norm_hip(x, inp, w, nw, eps)
    return add_rms_norm(x, linear(inp, w), nw, eps)


def swiglu_residual_rms_norm(x, h, w_gate_up, w_down, nw, eps=1e-5):
    """Llama's feed-forward site: (s, y) = (x + swiglu_mlp(h), RMSNorm(s)); on the GPU down_proj
    adds the residual stream in its epilogue (ops/residual.py)."""
    if _gpu(x) == "hip":
        from .residual import swiglu_eligible, swiglu_residual_rms_norm_hip
        if swiglu_eligible(x, h, w_gate_up, w_down):
            return swiglu_residual_rms_norm_hip(x, h, w_gate_up, w_down, nw, eps)
    return add_rms_norm(x, swiglu_mlp(h, w_gate_up, w_down), nw, eps)


def add_rms_norm(x, r, weight, eps=1e-5):
    """Fused residual add + RMSNorm: (s, y) = (x + r, RMSNorm(x + r))."""
    b = _gpu(x)
    if b == "hip":
        from .layernorm import add_rms_norm_hip
        return add_rms_norm_hip(x, r, weight, eps)
    s = x + r
    return s, rms_norm(s, weight, eps)


def linear(x, weight, bias=None):
    """x W^T + b (hipBLASLt GEMM; bias gradient by the HIP column-sum kernel)."""
    b = _gpu(x)
    if b == "hip":
        return linear_hip(x, weight, bias)
    return F.linear(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype))


def rms_norm(x, weight, eps=1e-5):
    b = _gpu(x)
    if b == "hip":
        from .layernorm import rms_norm_hip
        return rms_norm_hip(x, weight, eps)
    if b == "torch":
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * weight.to(x.dtype)
    return ref.rms_norm(x, weight, eps)


# --------------------------------------------------------------------------- activations
def gelu(x):
    b = _gpu(x)
    if b == "hip":
        from .activations import bias_gelu_hip
        return bias_gelu_hip(x, None)
    if b == "torch":
        return F.gelu(x, approximate="tanh")
    return ref.gelu_tanh(x)


def bias_gelu(x, bias):
    b = _gpu(x)
    if b == "hip":
        from .activations import bias_gelu_hip
        return bias_gelu_hip(x, bias)
    if b == "torch":
        return F.gelu(x + bias.to(x.dtype), approximate="tanh")
    return ref.bias_gelu(x, bias)


def gelu_linear(a, fc_bias, weight, bias=None):
    """linear(gelu(a + fc_bias), weight, bias): the MLP tail.  On the GPU one autograd node
    whose backward is a single GEMM with the GELU derivative and the fc-bias gradient fused
    into its epilogue (ops/activations.py); elsewhere bias_gelu then linear."""
    b = _gpu(a)
    if b == "hip":
        from .activations import fused_mlp_ok, gelu_linear_hip
        if fused_mlp_ok(a, weight):
            return gelu_linear_hip(a, fc_bias, weight, bias)
    h = gelu(a) if fc_bias is None else bias_gelu(a, fc_bias)
    return linear(h, weight, bias)


def mlp(x, w_fc, b_fc, w_proj, b_proj=None):
    """GPT-2's MLP: linear(gelu(x W_fc^T + b_fc), W_proj, b_proj).  On the GPT-2 GPU path
    (``ORION_FUSED_MLP``) both GELU passes live in GEMM epilogues (ops/activations.py
    ``_FusedMLP``); otherwise the fc GEMM then :func:`gelu_linear`."""
    b = _gpu(x)
    if b == "hip":
        from .activations import mlp_hip, mlp_ok
        if mlp_ok(x, w_fc, w_proj):
            return mlp_hip(x, w_fc, b_fc, w_proj, b_proj)
    return gelu_linear(linear(x, w_fc), b_fc, w_proj, b_proj)


def swiglu_mlp(x, w_gate_up, w_down):
    """Llama's feed-forward: linear(swiglu(x W_gu^T), W_down) with W_gu = [W_gate; W_up].  On
    the GPU path the SwiGLU backward runs in the down_proj input-gradient GEMM's epilogue
    (ops/activations.py ``_SwigluMLP``)."""
    b = _gpu(x)
    if b == "hip":
        from .activations import swiglu_mlp_hip, swiglu_mlp_ok
        if swiglu_mlp_ok(x, w_gate_up, w_down):
            return swiglu_mlp_hip(x, w_gate_up, w_down)
    return linear(swiglu(linear(x, w_gate_up)), w_down)


def swiglu(gate_up):
    """silu(gate) * up on a packed (..., 2F) [gate | up] projection -> (..., F)."""
    b = _gpu(gate_up)
    if b == "hip":
        from .activations import swiglu_hip
        return swiglu_hip(gate_up)
    gate, up = gate_up.chunk(2, dim=-1)
    if b == "torch":
        return F.silu(gate) * up
    return ref.swiglu(gate, up)


def embed_layer_norm(idx, wte, wpe, weight, bias, eps=1e-5):
    """GPT-2's input: (x, h) = (wte[idx] + wpe[:T], LayerNorm(x)) for idx (B, T).  On the GPU
    one kernel forward; backward writes the token-table gradient straight into its (tied)
    gradient-arena slice (ops/embedding.py)."""
    b = _gpu(wte)
    if b == "hip" and wte.shape[1] % 8 == 0 and wte.shape[1] <= 2048:
        from .embedding import embed_layer_norm_hip
        return embed_layer_norm_hip(idx, wte, wpe, weight, bias, eps)
    x = add_broadcast(F.embedding(idx, wte), wpe[:idx.shape[1]])
    return x, layer_norm(x, weight, bias, eps)


_TORCH_EMBEDDING = os.environ.get("ORION_EMBEDDING") == "torch"  # A/B: PyTorch's embedding backward


def token_embedding(idx, weight):
    """weight[idx] (Llama's token embedding; ``embedding`` is the submodule's name).  On the GPU
    the backward adds into the table's gradient-arena slice directly (ops/embedding.py)."""
    b = _gpu(weight)
    if b == "hip" and weight.shape[1] % 8 == 0 and weight.dtype == torch.bfloat16 and not _TORCH_EMBEDDING:
        from .embedding import embedding_hip
        return embedding_hip(idx, weight)
    return F.embedding(idx, weight)


def add_broadcast(x, pos):
    """x (B, T, C) + pos (T, C); kept as one op so the GPU path is one kernel."""
    return x + pos.to(x.dtype)


# --------------------------------------------------------------------------- rope
def rope(x, cos, sin, pos0=0):
    """Rotate-half RoPE of x (B, T, H, D) at positions pos0..pos0+T-1 (fp32 tables (Tmax, D/2))."""
    b = _gpu(x)
    if b == "hip":
        from .rotary import rope_hip
        return rope_hip(x, cos, sin, pos0)
    return ref.rope(x, cos[pos0:], sin[pos0:])


def linear_rope_attention(x, weight, n_q, n_kv, cos, sin, pos0=0):
    """Causal attention of (rope(q), rope(k), v) of the packed projection x W^T, W (Hq + 2 Hkv)
    D rows -> (B, T, Hq, D).  GPU path with head dim 128: one fused node, the rotation in the
    projection GEMM's epilogue (flash_attn.qkv_rope_flash_attention); otherwise the projection
    then rope_attention_packed."""
    if _gpu(x) == "hip":
        from .flash_attn import qkv_rope_eligible, qkv_rope_flash_attention
        if qkv_rope_eligible(x, weight, n_q, n_kv, cos):
            return qkv_rope_flash_attention(x, weight, n_q, n_kv, cos, sin, pos0)
    B, T, _ = x.shape
    qkv = linear(x, weight).view(B, T, n_q + 2 * n_kv, weight.shape[0] // (n_q + 2 * n_kv))
    return rope_attention_packed(qkv, n_q, n_kv, cos, sin, pos0)


def rope_attention_packed(qkv, n_q, n_kv, cos, sin, pos0=0):
    """Causal attention of (rope(q), rope(k), v) on a packed (B, T, Hq + 2 Hkv, D) projection
    -> (B, T, Hq, D).  The GPU path is one fused autograd node (no per-view glue)."""
    b = _gpu(qkv)
    if b == "hip":
        from .flash_attn import rope_flash_attention_packed
        return rope_flash_attention_packed(qkv, n_q, n_kv, cos, sin, pos0)
    q = rope(qkv[:, :, :n_q], cos, sin, pos0)
    k = rope(qkv[:, :, n_q:n_q + n_kv], cos, sin, pos0)
    return attention(q, k, qkv[:, :, n_q + n_kv:], causal=True)


# --------------------------------------------------------------------------- attention
def attention_qkv(qkv, n_head, causal=True):
    """Causal self-attention on a packed (B, T, 3C) projection -> (B, T, C)."""
    b = _gpu(qkv)
    if b == "hip":
        from .flash_attn import flash_attention_qkv
        return flash_attention_qkv(qkv, n_head, causal)
    if b == "torch":
        B, T, C3 = qkv.shape
        C = C3 // 3
        q, k, v = qkv.view(B, T, 3, n_head, C // n_head).unbind(2)
        y = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2),
                                           v.transpose(1, 2), is_causal=causal)
        return y.transpose(1, 2).reshape(B, T, C)
    return ref.attention_qkv(qkv, n_head, causal)


def linear_attention_qkv(x, weight, bias, n_head, causal=True):
    """Causal self-attention of the QKV projection x W^T + b -> (B, T, C).  On the HIP path
    the projection's bias gradient comes out of the attention backward (column sums fused
    into the split kernels) instead of a column-sum pass over the packed dQKV."""
    if _gpu(x) == "hip" and bias is not None:
        from .flash_attn import flash_attention_qkv
        qkv = linear_hip(x, weight, bias.detach())
        return flash_attention_qkv(qkv, n_head, causal, bias)
    return attention_qkv(linear(x, weight, bias), n_head, causal)


def attention(q, k, v, causal=True):
    """Attention on (B, T, H, D) tensors (GQA when k/v have fewer heads)."""
    b = _gpu(q)
    if b == "hip":
        from .flash_attn import flash_attention
        return flash_attention(q, k, v, causal)
    if b == "torch":
        rep = q.shape[2] // k.shape[2]
        kk = k.repeat_interleave(rep, 2) if rep > 1 else k
        vv = v.repeat_interleave(rep, 2) if rep > 1 else v
        y = F.scaled_dot_product_attention(q.transpose(1, 2), kk.transpose(1, 2),
                                           vv.transpose(1, 2), is_causal=causal)
        return y.transpose(1, 2)
    return ref.attention(q, k, v, causal)


# --------------------------------------------------------------------------- generation
def attention_decode(q, k_cache, v_cache, kv_lens, scale=None, splits=0, k_scale=None, v_scale=None):
    """One query per row against a key/value cache: q (B, Hq, D), caches (B, Tmax, Hkv, D), kv_lens
    (B,) int32 -> (B, Hq, D).  Row b attends keys [0, min(kv_lens[b], Tmax)); what lies beyond is
    never used (stale NaN included) and an empty row is zeros.  The GPU kernel reads the lengths
    on the device and splits the keys over ``splits`` workgroups per KV head (0: chosen from
    Tmax, so pass the cache cut at the host's bound of the length); inference only.
    ``float8_e4m3fn`` caches (:class:`KVCache` with ``kv_dtype="fp8"``) come with their fp32
    scales ``k_scale`` / ``v_scale`` (B, Hkv, Tmax), value = scale * byte, and run
    csrc/attn_decode.hip's FP8 kernel; bf16 caches refuse scales."""
    fp8 = ref.cache_is_fp8(k_cache, v_cache, k_scale, v_scale)
    b = _gpu(q)
    if b == "hip":
        from .decode import attention_decode_fp8_hip, attention_decode_hip
        if fp8:
            return attention_decode_fp8_hip(q, k_cache, v_cache, k_scale, v_scale, kv_lens, scale, splits)
        return attention_decode_hip(q, k_cache, v_cache, kv_lens, scale, splits)
    if b == "torch":
        from .decode import attention_decode_torch
        return attention_decode_torch(q, k_cache, v_cache, kv_lens, scale, k_scale, v_scale)
    return ref.attention_decode(q, k_cache, v_cache, kv_lens, scale, k_scale, v_scale)


def attention_decode_multi(q, k_cache, v_cache, kv_lens, scale=None, splits=0):
    """A few queries per row against a key/value cache with a causal tail, the attention of a
    speculative verify step: q (B, Tq, Hq, D) with 1 <= Tq <= 16, bf16 caches (B, Tmax, Hkv, D),
    kv_lens (B,) int32 including the Tq tokens of the forward in progress -> (B, Tq, Hq, D).
    Query t of row b attends keys [0, lim), lim = clamp(kv_lens[b] - Tq + 1 + t, 0,
    min(kv_lens[b], Tmax)); a query with lim = 0 yields zeros and keys at or beyond
    min(kv_lens[b], Tmax) are never loaded.  On the GPU one launch of csrc/attn_decode.hip's
    multi-query kernel (plus the combine of the key splits), whose output [:, t] equals bit for bit
    ``attention_decode(q[:, t], ..., kv_lens - (Tq - 1 - t), splits=splits)``: ``splits`` means
    what it means there (0: planned from Tmax).  An FP8 cache raises ``ValueError``.  Inference
    only."""
    if k_cache.dtype == torch.float8_e4m3fn or v_cache.dtype == torch.float8_e4m3fn:
        raise ValueError("attention_decode_multi takes bf16 caches only: an FP8 cache has no multi-query kernel")
    if q.dim() != 4 or not 1 <= q.shape[1] <= 16:
        raise ValueError(f"attention_decode_multi: q must be (B, Tq, Hq, D) with 1 <= Tq <= 16, got {tuple(q.shape)}")
    b = _gpu(q)
    if b == "hip":
        from .decode import attention_decode_multi_hip
        return attention_decode_multi_hip(q, k_cache, v_cache, kv_lens, scale, splits)
    if b == "torch":
        from .decode import attention_decode_multi_torch
        return attention_decode_multi_torch(q, k_cache, v_cache, kv_lens, scale)
    return ref.attention_decode_multi(q, k_cache, v_cache, kv_lens, scale)


def spec_draft(history, cur, out, ngram=3):
    """The n-gram draft of a speculative step: history (B, L) int64 whose columns [0, cur[b]] are
    known, cur (B,) int32, out (B, k + 1) int64, overwritten: out[b, 0] = history[b, cur[b]], and
    the k drafts continue the latest earlier occurrence of the row's last ``ngram`` tokens
    (periodically once the continuation runs into the present); without such an occurrence every
    draft is the current token (``ref.spec_draft`` states the rule).  One launch on the GPU,
    reading ``cur`` on the device; integer-exact."""
    if int(ngram) < 1:
        raise ValueError(f"spec_draft: ngram must be >= 1, got {ngram}")
    if history.is_cuda and _BACKEND == "hip":
        from .decode import spec_draft_hip
        return spec_draft_hip(history, cur, out, ngram)
    if history.is_cuda:
        out.copy_(ref.spec_draft(history.cpu(), cur.cpu(), out.cpu(), ngram))
        return out
    return ref.spec_draft(history, cur, out, ngram)


def spec_accept(tokens, target, start, lens, stop, history):
    """The accept rule of a speculative step: tokens (B, k + 1) int64 (the current token, then the
    drafts), target (B, k + 1) int64 (target[b, t] drawn from the logits of input t: the token at
    column start[b] + 1 + t), start / lens / stop (B,) int32, history (B, L) int64.  With a the
    number of leading drafts that equal the draw before them, e = clamp(min(a + 1, stop[b] -
    start[b]), 0, k + 1) tokens are emitted: history[b, start[b] + 1 + i] = target[b, i] for
    i < e (columns >= L skipped), lens[b] = start[b] + e, and nothing else is written.  One launch
    on the GPU, on device state only."""
    if tokens.is_cuda and _BACKEND == "hip":
        from .decode import spec_accept_hip
        return spec_accept_hip(tokens, target, start, lens, stop, history)
    if tokens.is_cuda:
        h, n = history.cpu(), lens.cpu()
        ref.spec_accept(tokens.cpu(), target.cpu(), start.cpu(), n, stop.cpu(), h)
        history.copy_(h)
        lens.copy_(n)
        return None
    ref.spec_accept(tokens, target, start, lens, stop, history)
    return None


def kv_append(k_new, v_new, k_cache, v_cache, kv_lens, q=None, cos=None, sin=None, k_scale=None, v_scale=None):
    """Write k_new / v_new (B, T, Hkv, D) into the caches at positions kv_lens[b] + t (skipping
    positions >= Tmax; kv_lens itself is unchanged).  With fp32 tables (``ref.rope_tables``) k is
    rotated at its position on the way in, and with q (B, T, Hq, D) the rotated q is returned as a
    new contiguous tensor (else None).  One launch on the GPU; inference only.  Into
    ``float8_e4m3fn`` caches every head row is quantised by :func:`quantize_kv_fp8` (k from its
    fp32 rotated values) and its scale stored in ``k_scale`` / ``v_scale`` (B, Hkv, Tmax); bf16
    caches refuse scales."""
    fp8 = ref.cache_is_fp8(k_cache, v_cache, k_scale, v_scale)
    b = _gpu(k_new)
    if b == "hip":
        from .decode import kv_append_fp8_hip, kv_append_hip
        if fp8:
            return kv_append_fp8_hip(k_new, v_new, k_cache, v_cache, k_scale, v_scale, kv_lens, q, cos, sin)
        return kv_append_hip(k_new, v_new, k_cache, v_cache, kv_lens, q, cos, sin)
    return ref.kv_append(k_new, v_new, k_cache, v_cache, kv_lens, q, cos, sin, k_scale, v_scale)


def linear_decode_eligible(x, weight):
    """Whether the skinny decode kernel (csrc/linear_decode.hip) takes this input on the HIP
    backend: bf16 GPU tensors, at most 16 rows of x with 16-byte aligned unit-stride rows,
    K % 8 == 0, a contiguous weight.  With an :class:`Fp8Weight`, whether the FP8 kernel
    (csrc/linear_decode_fp8.hip) does: the same for bf16 x, with K % 16 == 0; with an
    :class:`Mxfp4Weight`, whether csrc/linear_decode_mxfp4.hip does: K % 32 == 0."""
    if not x.is_cuda or _BACKEND != "hip":
        return False
    from .decode import linear_decode_eligible as ok
    return ok(x, weight)


def _linear_decode_composed(x, weight, bias, norm, norm_weight, norm_bias, eps, act, residual):
    """The same function on the plain ops of this module (each dispatching on its own)."""
    h = x
    if norm == "layer":
        h = layer_norm(x, norm_weight, norm_bias, eps)
    elif norm == "rms":
        h = rms_norm(x, norm_weight, eps)
    if act == "gelu":
        y = linear(h, weight)
        y = gelu(y) if bias is None else bias_gelu(y, bias)
    else:
        y = linear(h, weight, bias)
        if act == "swiglu":
            y = swiglu(y)
    return y if residual is None else y + residual.to(y.dtype)


def linear_decode(x, weight, bias=None, *, norm=None, norm_weight=None, norm_bias=None, eps=1e-5, act=None,
                  residual=None, out=None):
    """The decode step's linear layer, act(norm(x) W^T + bias) + residual, for x (..., K) with few
    rows and weight (N, K): ``norm`` in {None, "layer", "rms"} on the rows of x (``norm_weight``,
    LayerNorm's optional ``norm_bias``), ``act`` in {None, "gelu", "swiglu"} (SwiGLU over a packed
    [gate; up] weight of 2F rows -> (..., F)), ``residual`` a distinct tensor of the output's
    shape.  On the GPU one weight-streaming launch when :func:`linear_decode_eligible` (at most 16
    rows), else the plain ops composed; ``out`` (rows, Nout) takes the result in place.
    ``weight`` may be an :class:`Fp8Weight`: an eligible input streams its bytes through the FP8
    kernel, any other (the CPU, the torch backend, 17 or more rows) takes the path it would take
    with a plain weight, on ``weight.dequant(x.dtype)``.  An :class:`Mxfp4Weight` likewise, through
    the MXFP4 kernel.  Inference only."""
    assert norm in (None, "layer", "rms") and act in (None, "gelu", "swiglu"), (norm, act)
    assert (norm is None) == (norm_weight is None), "norm_weight comes with a norm"
    from .decode import _no_grad
    quantised = isinstance(weight, (Fp8Weight, Mxfp4Weight))
    _no_grad(x, None if quantised else weight, bias, norm_weight, norm_bias, residual)
    b = _gpu(x)
    if b == "hip" and linear_decode_eligible(x, weight):
        from .decode import linear_decode_hip
        return linear_decode_hip(x, weight, bias, norm, norm_weight, norm_bias, eps, act, residual, out)
    if quantised:
        weight = weight.dequant(x.dtype)
    if b is None:
        y = ref.linear_decode(x, weight, bias, norm, norm_weight, norm_bias, eps, act, residual)
    else:
        y = _linear_decode_composed(x, weight, bias, norm, norm_weight, norm_bias, eps, act, residual)
    if out is None:
        return y
    out.copy_(y.reshape(out.shape))
    return out.view(y.shape)


def sample_tokens_eligible(logits):
    """Whether the sampling kernel (csrc/sample.hip) takes these logits on the HIP backend:
    (B, V) bf16 on the GPU with unit stride on V."""
    if not logits.is_cuda or _BACKEND != "hip":
        return False
    from .decode import sample_tokens_eligible as ok
    return ok(logits)


def sample_tokens(logits, temperature=1.0, top_k=None, *, u=None, seed=None, positions=None, out=None,
                  history=None, params=None, u_out=None, rows_per_seq=1, position_offset=0):
    """One token per row of logits (B, V) -> (B, 1) int64 by the models' sampling rule with an
    explicit uniform: z = logits / max(temperature, 1e-6); with ``top_k`` only the entries >= the
    k-th largest of the row are kept (ties at the threshold all stay; None, <= 0 or >= V keeps
    everything); w = exp(z - max z) over the kept entries, and the token is the first kept index
    whose running sum in index order exceeds u sum(w) (the last kept index if rounding leaves
    none).  ``u`` (B,) fp32 is given, or is ``ref.philox_uniform(seed, positions)``: Philox4x32-10
    keyed by the 64-bit ``seed`` (an int or a (1,) int64 tensor) at counter (positions[b], b, 0, 0),
    ``positions`` (B,) int32, so no generator state is advanced.  ``out`` (B,) or (B, 1) int64
    takes the token in place, ``history`` (B, L) int64 also gets it at column positions[b] (skipped
    when that is >= L) and ``u_out`` (B,) fp32 the u that was used.  With ``rows_per_seq`` = R
    row r of the (B R, V) logits belongs to sequence b = r // R at t = r % R and its counter is
    (positions[b] + position_offset + t, b, 0, 0): the draws of R consecutive positions of every
    sequence in one launch (a speculative verify step); ``positions`` stays (B,) and ``history``
    is refused.

    On the GPU one launch when :func:`sample_tokens_eligible` (bf16 on the HIP backend), reading
    the temperature and top_k from ``params`` (``ops.decode.sample_params``; built from the two
    arguments when not given), so a captured launch serves every setting; other GPU inputs take
    the same rule on stock ops in fp32 (top-k mask, cumsum, searchsorted) and CPU tensors the fp64
    reference.  Inference only."""
    from .decode import _no_grad
    _no_grad(logits)
    assert logits.dim() == 2, "sample_tokens: logits must be (B, V)"
    R = int(rows_per_seq)
    if R < 1 or logits.shape[0] % R:
        raise ValueError(f"sample_tokens: rows_per_seq must be >= 1 and divide the {logits.shape[0]} rows, got {R}")
    if R > 1 and history is not None:
        raise ValueError("sample_tokens: history is not taken with rows_per_seq > 1")
    b = _gpu(logits)
    if b == "hip" and sample_tokens_eligible(logits):
        from .decode import sample_params, sample_tokens_hip
        if params is None:
            params = sample_params(temperature, top_k, logits.device)
        if u is None and seed is not None and not isinstance(seed, torch.Tensor):
            seed = torch.tensor([_wrap_i64(seed)], dtype=torch.int64).to(logits.device)
        return sample_tokens_hip(logits, params, u, seed, positions, out, history, u_out, R, position_offset)
    if params is not None:
        from .decode import read_sample_params
        temperature, top_k = read_sample_params(params)
    if u is None:
        assert seed is not None and positions is not None, "sample_tokens: without u, seed and positions are needed"
        u = ref.philox_uniform(seed, positions, R, position_offset)
    if u_out is not None:
        u_out.copy_(u)
    return ref.sample_tokens(logits, temperature, top_k, u, None, positions, out, history,
                             dtype=torch.float64 if b is None else torch.float32)


def _wrap_i64(v):
    """A 64-bit pattern given as any Python int, as the int64 that holds it."""
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >= 1 << 63 else v


# --------------------------------------------------------------------------- loss
def cross_entropy(logits, targets, ignore_index=-1):
    b = _gpu(logits)
    if b == "hip":
        from .xent import fused_cross_entropy
        return fused_cross_entropy(logits, targets, ignore_index)
    if b == "torch":
        return F.cross_entropy(logits.float(), targets, ignore_index=ignore_index)
    return ref.cross_entropy(logits, targets, ignore_index)


def linear_cross_entropy(x, weight, targets, ignore_index=-1):
    """mean CE of softmax(x @ weight^T); x (N, C), weight (V, C) -- the fused LM head + loss."""
    b = _gpu(x)
    if b == "hip":
        from .xent import linear_cross_entropy_hip
        return linear_cross_entropy_hip(x, weight, targets, ignore_index)
    logits = F.linear(x, weight.to(x.dtype))
    if b == "torch":
        return F.cross_entropy(logits.float(), targets, ignore_index=ignore_index)
    return ref.cross_entropy(logits, targets, ignore_index)


__all__ = [
    "set_backend", "backend", "ext_available", "load_ext",
    "layer_norm", "rms_norm", "gelu", "bias_gelu", "swiglu", "add_broadcast", "embed_layer_norm",
    "token_embedding", "rope",
    "attention_qkv", "linear_attention_qkv", "attention", "rope_attention_packed", "linear_rope_attention",
    "cross_entropy", "swiglu_mlp", "linear_residual_layer_norm", "mlp_residual_layer_norm",
    "linear_residual_rms_norm", "swiglu_residual_rms_norm",
    "linear_cross_entropy", "attention_decode", "attention_decode_multi", "spec_draft", "spec_accept",
    "kv_append", "linear_decode", "linear_decode_eligible",
    "sample_tokens", "sample_tokens_eligible", "Fp8Weight", "quantize_fp8", "quantize_kv_fp8",
    "Mxfp4Weight", "quantize_mxfp4",
]


# ------------------------------------------------------------------ parameter-read guards
# ZeRO-1 leaves the weight all-gathers of the previous optimizer step in flight
# (parallel/ddp.py ShardedGradReducer.gather_params).  The fused ops read weights of several
# modules at once from the model's top-level forward (block i's add+LayerNorm takes block
# i+1's ln_1, the embedding takes block 0's), so module forward hooks alone cannot say when a
# weight is first read: every op here that takes weights first hands its arguments to the
# registered guards, which wait for the gathers of the buckets those tensors live in.
_PARAM_GUARDS: list = []


def add_param_guard(fn):
    """Register ``fn(tensors)`` to run before any weight-taking op; returns a remover.  A
    bound method is held weakly (a dropped reducer unregisters itself)."""
    import weakref
    ref_ = weakref.WeakMethod(fn) if hasattr(fn, "__self__") else (lambda: fn)
    _PARAM_GUARDS.append(ref_)

    def remove():
        if ref_ in _PARAM_GUARDS:
            _PARAM_GUARDS.remove(ref_)
    return remove


def _guarded(fn):
    import functools

    @functools.wraps(fn)
    def run(*args, **kw):
        if _PARAM_GUARDS:
            ts = [a for a in args if isinstance(a, torch.Tensor)]
            ts += [a for a in kw.values() if isinstance(a, torch.Tensor)]
            for g in list(_PARAM_GUARDS):
                f = g()
                if f is None:
                    _PARAM_GUARDS.remove(g)
                else:
                    f(ts)
        return fn(*args, **kw)
    run.__wrapped_op__ = fn
    return run


for _name in ("layer_norm", "add_layer_norm", "add_rms_norm", "linear", "rms_norm", "bias_gelu",
              "gelu_linear", "mlp", "swiglu_mlp", "embed_layer_norm", "token_embedding", "add_broadcast",
              "linear_attention_qkv", "linear_rope_attention",
              "linear_cross_entropy", "linear_decode"):
    globals()[_name] = _guarded(globals()[_name])
del _name

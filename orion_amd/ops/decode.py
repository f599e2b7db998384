"""Generation-time ops over the HIP kernels of csrc/attn_decode.hip, csrc/linear_decode.hip,
csrc/linear_decode_fp8.hip and csrc/linear_decode_mxfp4.hip: single-query attention against a
bf16 or FP8 key/value cache (split over keys, lengths read on the device), the cache append with
optional RoPE (quantising into an FP8 cache), and the skinny (M <= 16) linear layer with a fused
norm prologue and bias / activation / residual epilogue, on a bf16 weight, an
:class:`~orion_amd.ops.fp8.Fp8Weight` or an :class:`~orion_amd.ops.mxfp4.Mxfp4Weight`.
Inference only: there is no backward, and an input that requires grad while gradients are
enabled is an error rather than a silently dropped graph."""
from __future__ import annotations

import math

import torch

from ._ext import C
from .fp8 import Fp8Weight, dequantize_kv_fp8
from .mxfp4 import Mxfp4Weight


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("attention_decode / kv_append / linear_decode are inference-only ops: inputs "
                           "must not require grad (run under torch.no_grad())")


NORMS = {None: 0, "layer": 1, "rms": 2}
ACTS = {None: 0, "gelu": 1, "swiglu": 2}
MAX_ROWS = 16  # rows of one MFMA tile: the kernel's upper bound on M


def _rows16(t):
    return t.stride(-1) == 1 and (t.shape[0] == 1 or t.stride(0) % 8 == 0) and t.data_ptr() % 16 == 0


def linear_decode_eligible(x, weight):
    """Whether csrc/linear_decode.hip takes x (..., K) (at most 16 rows that flatten to a view with
    16-byte aligned, unit-stride rows) against weight (N, K): both bf16 on the GPU, K % 8 == 0,
    weight contiguous.  For an :class:`Fp8Weight`, whether csrc/linear_decode_fp8.hip does: the
    same with K % 16 == 0.  For an :class:`Mxfp4Weight`, whether csrc/linear_decode_mxfp4.hip
    does: K, taken from the weight's logical shape, % 32 == 0 and 16-byte aligned codes."""
    kmult, K = 8, weight.shape[-1]
    if isinstance(weight, Fp8Weight):
        kmult, weight = 16, weight.q
    elif isinstance(weight, Mxfp4Weight):
        kmult, weight = 32, weight.q
    elif weight.dtype != torch.bfloat16:
        return False
    if not (x.is_cuda and weight.is_cuda and x.dtype == torch.bfloat16):
        return False
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != K or not weight.is_contiguous():
        return False
    if K < kmult or K % kmult or weight.data_ptr() % 16 or x.numel() == 0 or x.numel() // K > MAX_ROWS:
        return False
    try:
        x2 = x.view(-1, K)
    except RuntimeError:
        return False
    return _rows16(x2)


def linear_decode_hip(x, weight, bias=None, norm=None, norm_weight=None, norm_bias=None, eps=1e-5, act=None,
                      residual=None, out=None):
    """One launch: act(norm(x) W^T + bias) + residual for x (..., K) of at most 16 rows -> (..., Nout);
    ``out`` (rows, Nout) receives the result in place (a static buffer of a captured step)."""
    quantised = isinstance(weight, (Fp8Weight, Mxfp4Weight))
    _no_grad(x, None if quantised else weight, bias, norm_weight, norm_bias, residual)
    K = weight.shape[1]
    n_out = weight.shape[0] // 2 if act == "swiglu" else weight.shape[0]
    r2 = None if residual is None else residual.view(-1, n_out)
    if isinstance(weight, Fp8Weight):
        y = C().linear_decode_fp8(x.view(-1, K), weight.q, weight.scale, bias, NORMS[norm], norm_weight, norm_bias,
                                  float(eps), ACTS[act], r2, out)
    elif isinstance(weight, Mxfp4Weight):
        y = C().linear_decode_mxfp4(x.view(-1, K), weight.q, weight.scale, bias, NORMS[norm], norm_weight,
                                    norm_bias, float(eps), ACTS[act], r2, out)
    else:
        y = C().linear_decode(x.view(-1, K), weight, bias, NORMS[norm], norm_weight, norm_bias, float(eps),
                              ACTS[act], r2, out)
    return y.view(*x.shape[:-1], n_out)


def attention_decode_hip(q, k_cache, v_cache, kv_lens, scale=None, splits=0):
    """q (B, Hq, D), caches (B, Tmax, Hkv, D), kv_lens (B,) int32 on the device -> (B, Hq, D).
    ``splits = 0`` lets the host pick the key split from Tmax: pass a view of the cache cut at
    the host's upper bound of the length."""
    _no_grad(q, k_cache, v_cache)
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    return C().attn_decode(q, k_cache, v_cache, kv_lens, scale, int(splits))


def kv_append_hip(k_new, v_new, k_cache, v_cache, kv_lens, q=None, cos=None, sin=None):
    """One launch: k_new / v_new into the caches at kv_lens[b] + t (k rotated when tables are
    given); returns the rotated q, or None without q."""
    _no_grad(k_new, v_new, k_cache, v_cache, q)
    q_rot = C().kv_append(k_new, v_new, k_cache, v_cache, kv_lens, q, cos, sin)
    return q_rot if q is not None else None


def attention_decode_fp8_tile(D):
    """Keys per workgroup iteration of the decode attention kernel on either cache type
    (csrc/attn_decode_core.h's ``DecodeShape<D>::TILE``: 4 waves x 4 loads x 64 / (D / 8) keys per
    wave-wide load); a split is a whole number of them."""
    return 4 * 4 * (64 // (D // 8))


def attention_decode_fp8_hip(q, k_cache, v_cache, k_scale, v_scale, kv_lens, scale=None, splits=0):
    """:func:`attention_decode_hip` on ``float8_e4m3fn`` caches with fp32 scales (B, Hkv, Tmax)."""
    _no_grad(q, k_cache, v_cache, k_scale, v_scale)
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    return C().attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, kv_lens, scale, int(splits))


def kv_append_fp8_hip(k_new, v_new, k_cache, v_cache, k_scale, v_scale, kv_lens, q=None, cos=None, sin=None):
    """One launch: :func:`kv_append_hip` into ``float8_e4m3fn`` caches, every head row quantised by
    its own amax (``ops.fp8.quantize_kv_fp8``) and its scale stored beside the bytes."""
    _no_grad(k_new, v_new, k_cache, v_cache, k_scale, v_scale, q)
    q_rot = C().kv_append_fp8(k_new, v_new, k_cache, v_cache, k_scale, v_scale, kv_lens, q, cos, sin)
    return q_rot if q is not None else None


def sample_tokens_eligible(logits):
    """Whether csrc/sample.hip takes these logits: (B, V) bf16 on the GPU with unit stride on V
    (any row stride, any alignment of the rows)."""
    return (logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.numel() > 0
            and logits.stride(1) == 1 and logits.shape[1] < 2 ** 31)


def sample_params(temperature=1.0, top_k=None, device=None, out=None):
    """The sampling kernel's device-resident parameters: (2,) int32 holding the fp32 bits of the
    temperature and top_k (0: keep everything).  ``out`` is overwritten in place (a session's
    buffer, read by its captured launch)."""
    import struct
    bits = struct.unpack("<i", struct.pack("<f", float(temperature)))[0]
    k = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    host = torch.tensor([bits, k], dtype=torch.int32)
    if out is None:
        return host.to(device)
    out.copy_(host)
    return out


def read_sample_params(params):
    """(temperature, top_k) back from a :func:`sample_params` tensor (reads it on the host)."""
    import struct
    bits, k = params.tolist()
    return struct.unpack("<f", struct.pack("<i", bits))[0], (k if k > 0 else None)


def sample_tokens_hip(logits, params, u=None, seed=None, positions=None, out=None, history=None, u_out=None,
                      rows_per_seq=1, position_offset=0):
    """One launch, one workgroup per row: the token of every row of logits (B, V) -> (B, 1) int64
    (``out`` when given).  ``params`` from :func:`sample_params`; ``u`` (B,) fp32 or the kernel's
    own Philox draw from ``seed`` (1,) int64 and ``positions`` (B,) int32, all on the device
    (``positions`` (B / R,) with ``rows_per_seq`` = R rows per sequence)."""
    _no_grad(logits)
    if rows_per_seq == 1 and position_offset == 0:
        return C().sample_tokens(logits, params, u, seed, positions, out, history, u_out).view(-1, 1)
    return C().sample_tokens(logits, params, u, seed, positions, out, history, u_out, int(rows_per_seq),
                             int(position_offset)).view(-1, 1)


def attention_decode_multi_hip(q, k_cache, v_cache, kv_lens, scale=None, splits=0):
    """q (B, Tq, Hq, D) with Tq <= 16, caches (B, Tmax, Hkv, D), kv_lens (B,) int32 on the device
    (the Tq new tokens included) -> (B, Tq, Hq, D): the multi-query kernel of csrc/attn_decode.hip, planned as
    :func:`attention_decode_hip` plans (``splits = 0``: from Tmax)."""
    _no_grad(q, k_cache, v_cache)
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    return C().attn_decode_multi(q, k_cache, v_cache, kv_lens, scale, int(splits))


def attention_decode_multi_torch(q, k_cache, v_cache, kv_lens, scale=None):
    """Stock PyTorch: SDPA with an explicit mask on each row's valid slice (reads the lengths on
    the host)."""
    from .reference import decode_multi_bounds
    _no_grad(q, k_cache, v_cache)
    B, Tq, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    out = torch.zeros(B, Tq, Hq, D, dtype=q.dtype, device=q.device)
    for b, n in enumerate(kv_lens.tolist()):
        bounds = decode_multi_bounds(n, Tq, Tmax)
        top = max(bounds)
        if top == 0:
            continue
        k, v = k_cache[b, :top].transpose(0, 1), v_cache[b, :top].transpose(0, 1)  # (Hkv, top, D)
        if rep > 1:
            k, v = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
        lim = torch.tensor(bounds, device=q.device).view(Tq, 1)
        mask = torch.arange(top, device=q.device).view(1, top) < lim  # (Tq, top)
        y = torch.nn.functional.scaled_dot_product_attention(
            q[b].transpose(0, 1)[None], k[None], v[None], attn_mask=mask, scale=scale)[0]  # (Hq, Tq, D)
        y = y.transpose(0, 1).masked_fill(~mask.any(1).view(Tq, 1, 1), 0.0)  # a query without keys is zeros
        out[b] = y
    return out


def spec_draft_hip(history, cur, out, ngram):
    """One launch (csrc/spec_decode.hip): see ``ops.spec_draft``."""
    C().spec_draft(history, cur, out, int(ngram))
    return out


def spec_accept_hip(tokens, target, start, lens, stop, history):
    """One launch (csrc/spec_decode.hip): see ``ops.spec_accept``."""
    C().spec_accept(tokens, target, start, lens, stop, history)


def attention_decode_torch(q, k_cache, v_cache, kv_lens, scale=None, k_scale=None, v_scale=None):
    """Stock PyTorch: SDPA on each row's valid slice (reads the lengths on the host); the slice of
    an FP8 cache is dequantised to ``q.dtype`` first."""
    _no_grad(q, k_cache, v_cache)
    fp8 = k_scale is not None
    B, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=q.dtype, device=q.device)
    for b, n in enumerate(kv_lens.tolist()):
        n = max(0, min(int(n), Tmax))
        if n == 0:
            continue
        k, v = k_cache[b, :n], v_cache[b, :n]
        if fp8:
            k = dequantize_kv_fp8(k, k_scale[b, :, :n], q.dtype)
            v = dequantize_kv_fp8(v, v_scale[b, :, :n], q.dtype)
        k, v = k.transpose(0, 1), v.transpose(0, 1)  # (Hkv, n, D)
        if rep > 1:
            k, v = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
        out[b] = torch.nn.functional.scaled_dot_product_attention(
            q[b][None, :, None, :], k[None], v[None], scale=scale)[0, :, 0]
    return out

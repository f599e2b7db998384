"""Plain-PyTorch reference implementations of every fused op.

These are the CPU execution path and the numerics oracle for the HIP kernels
in ``csrc/``.  They favour clarity over speed and compute in fp32 internally.

Layout conventions shared with the HIP kernels:

* ``qkv`` is the raw output of the fused QKV projection, shape ``(B, T, 3*C)``
  and read as ``(B, T, 3, H, D)``; attention output is ``(B, T, H*D)`` so it
  feeds the output projection with no transpose.
* cross-entropy takes ``logits`` ``(N, V)`` and int64 ``targets`` ``(N,)``;
  ``ignore_index`` rows contribute nothing.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def layer_norm(x, weight, bias, eps=1e-5):
    y = F.layer_norm(x.float(), (x.shape[-1],), weight.float(),
                     None if bias is None else bias.float(), eps)
    return y.to(x.dtype)


def rms_norm(x, weight, eps=1e-5):
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()
    return y.to(x.dtype)


def gelu_tanh(x):
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def bias_gelu(x, bias):
    return F.gelu(x.float() + bias.float(), approximate="tanh").to(x.dtype)


def swiglu(gate, up):
    return (F.silu(gate.float()) * up.float()).to(gate.dtype)


def rope_tables(seq_len, head_dim, theta=10000.0, device=None):
    """cos/sin tables of shape (T, D/2), fp32 (computed once on the host side)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    t = torch.arange(seq_len, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device), ang.sin().float().to(device)


def rope(x, cos, sin):
    """Rotate interleaved-half pairs (x[..., :D/2], x[..., D/2:]) of x (B, T, H, D)."""
    xf = x.float()
    d2 = x.shape[-1] // 2
    x1, x2 = xf[..., :d2], xf[..., d2:]
    c = cos[: x.shape[1]].view(1, x.shape[1], 1, d2)
    s = sin[: x.shape[1]].view(1, x.shape[1], 1, d2)
    out = torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)
    return out.to(x.dtype)


def attention_qkv(qkv, n_head, causal=True, scale=None):
    """softmax(Q K^T * scale [+ causal mask]) V for packed qkv (B, T, 3*C)."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    q, k, v = qkv.float().view(B, T, 3, n_head, D).unbind(2)
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))  # (B, H, T, D)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    p = s.softmax(-1)
    o = (p @ v).transpose(1, 2).reshape(B, T, C)
    return o.to(qkv.dtype)


def attention(q, k, v, causal=True, scale=None):
    """softmax attention for separate q (B,T,Hq,D), k/v (B,T,Hkv,D) with GQA."""
    B, T, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = (qf @ kf.transpose(-1, -2)) * scale
    if causal:
        Tk = k.shape[1]
        mask = torch.ones(T, Tk, dtype=torch.bool, device=q.device).tril(Tk - T)
        s = s.masked_fill(~mask, float("-inf"))
    o = (s.softmax(-1) @ vf).transpose(1, 2)
    return o.to(q.dtype)


def cache_is_fp8(k_cache, v_cache, k_scale, v_scale):
    """Whether the caches are FP8: then both scales (B, Hkv, Tmax) are required, else refused."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if fp8 != (v_cache.dtype == torch.float8_e4m3fn):
        raise ValueError(f"k_cache and v_cache must share a dtype, got {k_cache.dtype} and {v_cache.dtype}")
    if fp8 and (k_scale is None or v_scale is None):
        raise ValueError("float8_e4m3fn caches need k_scale and v_scale (B, Hkv, Tmax)")
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError(f"k_scale / v_scale go with float8_e4m3fn caches, not {k_cache.dtype}")
    if fp8:
        want = (k_cache.shape[0], k_cache.shape[2], k_cache.shape[1])
        if tuple(k_scale.shape) != want or tuple(v_scale.shape) != want:
            raise ValueError(f"k_scale / v_scale must be (B, Hkv, Tmax) = {want}, got {tuple(k_scale.shape)} and "
                             f"{tuple(v_scale.shape)}")
    return fp8


def attention_decode(q, k_cache, v_cache, kv_lens, scale=None, k_scale=None, v_scale=None):
    """One query per row against a key/value cache: q (B, Hq, D), caches (B, Tmax, Hkv, D),
    kv_lens (B,) -> (B, Hq, D).  Row b attends keys [0, min(kv_lens[b], Tmax)); positions beyond
    are never read (they may hold anything), and a row of length 0 is zeros.  FP8 caches
    (``float8_e4m3fn`` with fp32 scales (B, Hkv, Tmax)) are dequantised to fp32, exactly, first."""
    if cache_is_fp8(k_cache, v_cache, k_scale, v_scale):
        from .fp8 import dequantize_kv_fp8
        return attention_decode(q, dequantize_kv_fp8(k_cache, k_scale), dequantize_kv_fp8(v_cache, v_scale),
                                kv_lens, scale)
    B, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=q.device)
    for b, n in enumerate(kv_lens.tolist()):
        n = max(0, min(int(n), Tmax))
        if n == 0:
            continue
        kf = k_cache[b, :n].float().repeat_interleave(rep, dim=1).transpose(0, 1)  # (Hq, n, D)
        vf = v_cache[b, :n].float().repeat_interleave(rep, dim=1).transpose(0, 1)
        s = torch.einsum("hd,hnd->hn", q[b].float(), kf) * scale
        out[b] = torch.einsum("hn,hnd->hd", s.softmax(-1), vf)
    return out.to(q.dtype)


def decode_multi_bounds(n, Tq, Tmax):
    """The key bounds of the Tq queries of a row of length n (the Tq new tokens included):
    query t attends keys [0, clamp(n - Tq + 1 + t, 0, min(n, Tmax)))."""
    top = max(0, min(int(n), Tmax))
    return [max(0, min(int(n) - Tq + 1 + t, top)) for t in range(Tq)]


def attention_decode_multi(q, k_cache, v_cache, kv_lens, scale=None):
    """A few queries per row against a key/value cache with a causal tail: q (B, Tq, Hq, D), caches
    (B, Tmax, Hkv, D), kv_lens (B,) including the Tq tokens of the forward in progress ->
    (B, Tq, Hq, D).  Query t of row b attends keys [0, lim), lim as in :func:`decode_multi_bounds`;
    a query without keys is zeros and nothing at or beyond min(kv_lens[b], Tmax) is read.  fp32
    math, returned in q's dtype; bf16 caches only."""
    if k_cache.dtype == torch.float8_e4m3fn or v_cache.dtype == torch.float8_e4m3fn:
        raise ValueError("attention_decode_multi takes bf16 caches only, not float8_e4m3fn")
    B, Tq, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out = torch.zeros(B, Tq, Hq, D, dtype=torch.float32, device=q.device)
    for b, n in enumerate(kv_lens.tolist()):
        bounds = decode_multi_bounds(n, Tq, Tmax)
        top = max(bounds)
        if top == 0:
            continue
        kf = k_cache[b, :top].float().repeat_interleave(rep, dim=1).transpose(0, 1)  # (Hq, top, D)
        vf = v_cache[b, :top].float().repeat_interleave(rep, dim=1).transpose(0, 1)
        for t, lim in enumerate(bounds):
            if lim == 0:
                continue
            s = torch.einsum("hd,hnd->hn", q[b, t].float(), kf[:, :lim]) * scale
            out[b, t] = torch.einsum("hn,hnd->hd", s.softmax(-1), vf[:, :lim])
    return out.to(q.dtype)


def spec_draft(history, cur, out, ngram):
    """The n-gram draft of a speculative step, in plain Python: history (B, L) int64 with columns
    [0, cur[b]] known, out (B, k + 1) int64.  out[b, 0] = history[b, cur]; with g = ngram and j the
    largest index in [0, cur - g] whose g tokens equal the row's last g, P = cur - g + 1 - j and
    draft i (1..k) = history[b, j + g + ((i - 1) mod P)]: the continuation of the latest earlier
    occurrence, periodic once it runs into the present.  Without a match (or cur < g) every draft
    is history[b, cur]."""
    g = int(ngram)
    assert g >= 1, "ngram must be >= 1"
    L = history.shape[1]
    rows, curs = history.tolist(), cur.tolist()
    for b, h in enumerate(rows):
        c = max(0, min(int(curs[b]), L - 1))
        tail = c - g + 1
        j = -1
        for cand in range(tail - 1, -1, -1):
            if h[cand:cand + g] == h[tail:tail + g]:
                j = cand
                break
        vals = [h[c]] + [h[c] if j < 0 else h[j + g + (i - 1) % (tail - j)] for i in range(1, out.shape[1])]
        out[b] = torch.tensor(vals, dtype=out.dtype)
    return out


def spec_accept(tokens, target, start, lens, stop, history):
    """The accept rule of a speculative step, in plain Python: tokens (B, k + 1) the current token
    then the drafts, target (B, k + 1) the draws from the logits of each input.  a = the number of
    leading i in 1..k with tokens[b, i] == target[b, i - 1]; e = clamp(min(a + 1, stop[b] -
    start[b]), 0, k + 1); history[b, start[b] + 1 + i] = target[b, i] for i < e (columns >= L
    skipped) and lens[b] = start[b] + e.  Returns the list of e."""
    k = tokens.shape[1] - 1
    L = history.shape[1]
    tok, tgt, st, sp = tokens.tolist(), target.tolist(), start.tolist(), stop.tolist()
    es = []
    for b in range(len(tok)):
        a = 0
        while a < k and tok[b][a + 1] == tgt[b][a]:
            a += 1
        e = max(0, min(a + 1, int(sp[b]) - int(st[b]), k + 1))
        for i in range(e):
            col = int(st[b]) + 1 + i
            if 0 <= col < L:
                history[b, col] = tgt[b][i]
        lens[b] = int(st[b]) + e
        es.append(e)
    return es


def kv_append(k_new, v_new, k_cache, v_cache, kv_lens, q=None, cos=None, sin=None, k_scale=None, v_scale=None):
    """Write k_new / v_new (B, T, Hkv, D) into the caches (B, Tmax, Hkv, D) at positions
    kv_lens[b] + t; positions >= Tmax are skipped.  With tables k is rotated at its position
    (fp32, rounded once) and, given q (B, T, Hq, D), the rotated q is returned as a new tensor
    (rows of skipped positions are zero).  kv_lens is not changed.  FP8 caches take each head row
    through ``ops.fp8.quantize_kv_fp8`` (k from its fp32 rotated values): bytes into the caches,
    scales into k_scale / v_scale (B, Hkv, Tmax)."""
    fp8 = cache_is_fp8(k_cache, v_cache, k_scale, v_scale)
    B, T = k_new.shape[:2]
    Tmax = k_cache.shape[1]
    assert q is None or cos is not None, "q is only taken for rotation (pass cos / sin)"
    q_rot = None if q is None else torch.zeros(q.shape, dtype=q.dtype, device=q.device)
    for b, p0 in enumerate(kv_lens.tolist()):
        p0 = int(p0)
        n = max(0, min(T, Tmax - p0))  # tokens of this row that fit
        if n == 0 or p0 < 0:
            continue
        kb = k_new[b:b + 1, :n]
        if cos is not None:
            kb = rope(kb.float() if fp8 else kb, cos[p0:p0 + n], sin[p0:p0 + n])  # fp32 in, fp32 out
            if q is not None:
                q_rot[b:b + 1, :n] = rope(q[b:b + 1, :n], cos[p0:p0 + n], sin[p0:p0 + n])
        if fp8:
            from .fp8 import quantize_kv_fp8
            for cache, sc, x in ((k_cache, k_scale, kb[0]), (v_cache, v_scale, v_new[b, :n])):
                bytes_, s = quantize_kv_fp8(x)  # (n, Hkv, D), (n, Hkv)
                cache[b, p0:p0 + n] = bytes_
                sc[b, :, p0:p0 + n] = s.t()
            continue
        k_cache[b, p0:p0 + n] = kb[0].to(k_cache.dtype)
        v_cache[b, p0:p0 + n] = v_new[b, :n].to(v_cache.dtype)
    return q_rot


def linear_decode(x, weight, bias=None, norm=None, norm_weight=None, norm_bias=None, eps=1e-5, act=None,
                  residual=None):
    """The decode step's fused linear as a composition of the functions above:
    act(norm(x) W^T + bias) + residual with norm in {None, "layer", "rms"} on the rows of x and
    act in {None, "gelu", "swiglu"} (SwiGLU over a packed [gate; up] weight of 2F rows -> F)."""
    assert norm in (None, "layer", "rms") and act in (None, "gelu", "swiglu"), (norm, act)
    h = x
    if norm == "layer":
        h = layer_norm(x, norm_weight, norm_bias, eps)
    elif norm == "rms":
        h = rms_norm(x, norm_weight, eps)
    y = F.linear(h, weight.to(h.dtype))
    if act == "gelu":
        y = gelu_tanh(y) if bias is None else bias_gelu(y, bias)
    else:
        if bias is not None:
            y = y + bias.to(y.dtype)
        if act == "swiglu":
            y = swiglu(*y.chunk(2, dim=-1))
    if residual is not None:
        y = y + residual.to(y.dtype)
    return y


def philox4x32_10(counter, key):
    """Philox4x32-10 in integer math: ``counter`` (..., 4) and ``key`` (2,) of 32-bit words (any
    integer type) -> the four output words, a uint32 array (..., 4).  One round is p0 = 0xD2511F53
    c0, p1 = 0xCD9E8D57 c2 (64-bit products), c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1,
    lo(p0)), then k0 += 0x9E3779B9, k1 += 0xBB67AE85."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c = np.asarray(counter).astype(np.uint64) & m32
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k = [int(v) & 0xFFFFFFFF for v in np.asarray(key).reshape(2).tolist()]
    k0, k1 = k
    for _ in range(10):
        p0 = (np.uint64(0xD2511F53) * c0)  # < 2^64: both factors are below 2^32
        p1 = (np.uint64(0xCD9E8D57) * c2)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform_from_word(x0):
    """A 32-bit word (uint32 array) -> fp32 u = (x0 >> 8) 2^-24 + 2^-25, rounded to fp32 and capped
    at 1 - 2^-24 (the sum of the largest word is a tie that rounds up to 1.0): strictly inside
    (0, 1)."""
    import numpy as np
    u = (np.asarray(x0, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.minimum(u + np.float32(2.0 ** -25), np.float32(1.0 - 2.0 ** -24))


def philox_uniform(seed, positions, rows_per_seq=1, position_offset=0):
    """The sampling kernel's uniforms, bit for bit: row b draws word 0 of Philox4x32-10 with the
    two 32-bit halves of the 64-bit ``seed`` (an int or a one-element tensor) as key and
    (positions[b], b, 0, 0) as counter; u = :func:`uniform_from_word` of it, strictly inside (0, 1).
    ``positions`` (B,) integer tensor -> (B,) fp32 on its device.  With ``rows_per_seq`` = R the
    result is (B R,): row r = b R + t draws from (positions[b] + position_offset + t, b, 0, 0)."""
    import numpy as np
    seed = int(seed.reshape(-1)[0].item()) if isinstance(seed, torch.Tensor) else int(seed)
    seed &= (1 << 64) - 1
    R = int(rows_per_seq)
    pos = positions.detach().cpu().numpy().astype(np.int64)
    seq = np.repeat(np.arange(pos.shape[0]), R)
    pos = np.repeat(pos, R) + int(position_offset) + np.tile(np.arange(R), pos.shape[0])
    ctr = np.zeros((pos.shape[0], 4), dtype=np.int64)
    ctr[:, 0] = pos & 0xFFFFFFFF
    ctr[:, 1] = seq
    x0 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[:, 0]
    return torch.from_numpy(uniform_from_word(x0)).to(positions.device)


def sample_keep_mask(logits, top_k=None):
    """The entries the sampling rule keeps: every one >= the top_k-th largest of its row, ties at
    the threshold included; all of them for top_k None, <= 0 or >= V."""
    V = logits.size(-1)
    if top_k is None or top_k <= 0 or top_k >= V:
        return torch.ones_like(logits, dtype=torch.bool)
    v, _ = torch.topk(logits.float(), int(top_k))
    return ~(logits.float() < v[:, [-1]])


def sample_cdf(logits, temperature=1.0, top_k=None, dtype=torch.float64):
    """Running sums in index order of w = exp(z - max z) over the kept entries of logits (B, V),
    z = logits / max(temperature, 1e-6), and their total Z: ((B, V), (B, 1)) in ``dtype``."""
    keep = sample_keep_mask(logits, top_k)
    z = logits.to(dtype) / max(float(temperature), 1e-6)
    z = z.masked_fill(~keep, -float("inf"))
    w = torch.exp(z - z.max(dim=-1, keepdim=True).values).masked_fill(~keep, 0.0)
    c = torch.cumsum(w, dim=-1)
    return c, c[:, -1:]


def sample_tokens(logits, temperature=1.0, top_k=None, u=None, seed=None, positions=None, out=None, history=None,
                  dtype=torch.float64, rows_per_seq=1, position_offset=0):
    """The models' sampling rule with an explicit uniform per row: the token of row b is the first
    kept index whose running sum (:func:`sample_cdf`, fp64) exceeds u[b] Z, or the last kept
    index if rounding leaves none.  ``u`` (B,) is given or is :func:`philox_uniform` of ``seed``
    and ``positions`` (with ``rows_per_seq`` = R and ``position_offset``: row r of the (B R, V)
    logits is token r % R of sequence r // R, positions stays (B,) and history is refused).
    Returns (B, 1) int64 (``out`` (B,) or (B, 1) when given); with ``history`` (B, L) the token
    also goes to history[b, positions[b]] unless the position is >= L."""
    B, V = logits.shape
    if rows_per_seq != 1 and history is not None:
        raise ValueError("sample_tokens: history is not taken with rows_per_seq > 1")
    if u is None:
        assert seed is not None and positions is not None, "without u, seed and positions are needed"
        u = philox_uniform(seed, positions, rows_per_seq, position_offset)
    c, Z = sample_cdf(logits, temperature, top_k, dtype)
    tok = torch.searchsorted(c, u.to(device=c.device, dtype=dtype).view(B, 1) * Z, right=True)
    keep = sample_keep_mask(logits, top_k)
    last = (keep * torch.arange(V, device=logits.device)).max(dim=-1, keepdim=True).values
    tok = torch.where(tok >= V, last, tok).clamp_(0, V - 1)
    if out is None:
        out = tok
    else:
        out.view(B, 1).copy_(tok)
        out = out.view(B, 1)
    if history is not None:
        assert positions is not None, "history needs positions"
        pos = positions.long()
        ok = (pos >= 0) & (pos < history.size(1))
        rows = torch.arange(B, device=history.device)[ok]
        history[rows, pos[ok]] = tok[ok, 0]
    return out


def cross_entropy(logits, targets, ignore_index=-1):
    return F.cross_entropy(logits.float(), targets, ignore_index=ignore_index)


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
               grad_scale=1.0):
    """In-place decoupled-weight-decay Adam on fp32 tensors (torch.optim.AdamW maths)."""
    g = grad.float() * grad_scale
    param.mul_(1.0 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    param.addcdiv_(exp_avg, denom, value=-lr / bc1)
    return param

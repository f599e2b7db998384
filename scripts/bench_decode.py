#!/usr/bin/env python3
"""Generation benchmark: (i) the split-KV decode attention kernel (csrc/attn_decode.hip) beside
torch SDPA on the same cache view and beside its FP8-cache form (the same file) on the
quantised caches, at the GPT-2, the Llama-GQA and the Llama-2-7B MHA decode shapes; (ii) generated
tokens/s of ``gpt2`` with and without the KV cache (prompt 64 + 256 new tokens at B 1 and 8, and
a long-context point, prompt 768 at B 8) and on the fused decode step, eager (``fused``) and
replayed from one captured HIP graph (``graph``) and with the tokens drawn inside that graph
(``graph_device``: ``sampler="device"``) and from FP8 weights (``graph_device_fp8``: also
``weights="fp8"``), MXFP4 weights (``graph_device_mxfp4``: ``weights="mxfp4"``) or an FP8 key/value
cache (``graph_device_kvfp8``: ``kv="fp8"``), the arms alternating; (iii) the skinny decode linear
(csrc/linear_decode.hip) and its FP8-weight and MXFP4-weight forms (csrc/linear_decode_fp8.hip,
csrc/linear_decode_mxfp4.hip) at every projection shape of ``gpt2`` and of the Llama-2-7B layer
at M = 1, 8, 16 beside the same call through ``F.linear`` with its separate norm / activation /
residual launches; (iv) the sampling kernel (csrc/sample.hip) beside ``sample_logits`` (stock
torch ops) on the same logits at B 1, 8, 16 and V 50,304 and 32,000, top-k 200 and none;
(v) the multi-query decode kernel (csrc/attn_decode.hip) at Tq 4 and 8 beside Tq single-query
calls on the shapes of (i) (``--multi``); (vi) speculative decoding (``--speculative``): generated
tokens/s of ``gpt2`` at B 1 with k 3 and 7 guesses per step beside the plain
``use_cache="graph", sampler="device"`` session, the arms alternating, in three drafting regimes:
all-correct drafts (a ``draft=`` tensor holding the plain run's tokens: the ceiling), all-wrong
drafts (the price of a verify step) and n-gram drafts on a periodic prompt, with the mean tokens
per verify step of each.

The kernel timing rotates over enough distinct caches to exceed the 256 MB Infinity Cache, so
every call streams its K and V from HBM; bytes/s counts the K + V actually read (one pass per
KV head; the FP8 arm's own bytes: one per element and four per (token, head) scale); the linear
timing rotates over weights the same way (each arm over more than 512 MB of its own format) and
counts the weight bytes (the FP8 arm's: one per element and four per row; the MXFP4 arm's: half a
byte per element and one per 32 elements).
Prints one JSON line per measurement.

usage: python scripts/bench_decode.py [--shapes a,b] [--kernel 0|1] [--linear 0|1] [--sample 0|1] [--generate 0|1]
                                      [--multi 0|1] [--speculative 0|1] [--rounds N]
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orion_amd import ops  # noqa: E402
from orion_amd.models.gpt2 import build_gpt2  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X (8.0 TB/s spec)
SHAPES = {"gpt2": dict(B=8, Hq=12, Hkv=12, D=64, T=1024), "llama-gqa": dict(B=8, Hq=32, Hkv=8, D=128, T=4096),
          "llama2-7b-mha": dict(B=16, Hq=32, Hkv=32, D=128, T=4096)}


def _time_us(fns, rounds, calls=40):
    """Median over ``rounds`` of the mean time per call of ``calls`` back-to-back calls, per arm;
    the arms alternate inside every round.  A few milliseconds of matmul are queued ahead of the
    timed window, so the host enqueues all its calls while the GPU is still busy and the events
    bracket kernels running back to back: device time, not the host's launch rate."""
    busy = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    for fn in fns.values():
        for i in range(8):
            fn(i)
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):
                busy @ busy
            a.record()
            for i in range(calls):
                fn(i)
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def bench_kernel(name, B, Hq, Hkv, D, T, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    kv_bytes = 2 * B * T * Hkv * D * 2
    q_bytes = 2 * B * T * Hkv * (D + 4)
    n_buf = max(2, math.ceil(512e6 / kv_bytes))
    n_q = max(2, math.ceil(512e6 / q_bytes))
    caches = [torch.randn(2, B, T, Hkv, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(n_buf)]
    qcaches = []  # (bytes (2, B, T, Hkv, D), scales (2, B, Hkv, T)) of the same or further caches
    for i in range(n_q):
        src = caches[i] if i < n_buf else torch.randn(2, B, T, Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
        qb, qs = ops.quantize_kv_fp8(src)
        qcaches.append((qb, qs.transpose(2, 3).contiguous()))
    q = torch.randn(B, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    sdpa = torch.nn.functional.scaled_dot_product_attention
    q4 = q[:, :, None, :]  # (B, Hq, 1, D)

    def hip(i):
        c = caches[i % n_buf]
        return ops.attention_decode(q, c[0], c[1], lens)

    def fp8(i):
        c, sc = qcaches[i % n_q]
        return ops.attention_decode(q, c[0], c[1], lens, k_scale=sc[0], v_scale=sc[1])

    def torch_sdpa(i):
        c = caches[i % n_buf]
        return sdpa(q4, c[0].transpose(1, 2), c[1].transpose(1, 2), enable_gqa=Hq != Hkv)

    err = (hip(0).float() - torch_sdpa(0)[:, :, 0].float()).abs().max().item()
    err8 = (fp8(0).float() - hip(0).float()).abs().max().item()  # the quantisation of cache 0
    us = _time_us({"hip": hip, "fp8": fp8, "sdpa": torch_sdpa}, rounds)
    res = dict(bench="decode_kernel", shape=name, B=B, Hq=Hq, Hkv=Hkv, D=D, len=T, kv_mbytes=round(kv_bytes / 1e6, 1),
               rotating_caches=n_buf, fp8_kv_mbytes=round(q_bytes / 1e6, 1), fp8_rotating_caches=n_q,
               max_abs_diff_vs_sdpa=round(err, 5), fp8_max_abs_diff_vs_hip=round(err8, 5), hbm_copy_TBs=HBM_COPY_TBS)
    for k, v in us.items():
        res[f"{k}_us"] = round(v, 2)
        res[f"{k}_TBs"] = round((q_bytes if k == "fp8" else kv_bytes) / v / 1e6, 3)
    res["hip_over_copy_rate"] = round(res["hip_TBs"] / HBM_COPY_TBS, 3)
    res["fp8_over_copy_rate"] = round(res["fp8_TBs"] / HBM_COPY_TBS, 3)
    res["fp8_over_hip"] = round(us["hip"] / us["fp8"], 2)  # > 1: the FP8 kernel is faster than the bf16 one
    print(json.dumps(res), flush=True)


def bench_kernel_multi(name, B, Hq, Hkv, D, T, Tq, rounds):
    """One ``ops.attention_decode_multi`` over Tq queries per row beside the Tq single-query calls
    it is bit-equal to, rotating over caches as :func:`bench_kernel` does."""
    g = torch.Generator(device="cuda").manual_seed(0)
    kv_bytes = 2 * B * T * Hkv * D * 2
    n_buf = max(2, math.ceil(512e6 / kv_bytes))
    caches = [torch.randn(2, B, T, Hkv, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(n_buf)]
    q = torch.randn(B, Tq, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    lens_t = [lens - (Tq - 1 - t) for t in range(Tq)]

    def multi(i):
        c = caches[i % n_buf]
        return ops.attention_decode_multi(q, c[0], c[1], lens)

    def singles(i):
        c = caches[i % n_buf]
        return [ops.attention_decode(q[:, t], c[0], c[1], lens_t[t]) for t in range(Tq)]

    assert torch.equal(multi(0), torch.stack(singles(0), dim=1))
    us = _time_us({"multi": multi, "singles": singles}, rounds)
    res = dict(bench="decode_kernel_multi", shape=name, B=B, Hq=Hq, Hkv=Hkv, D=D, len=T, Tq=Tq,
               kv_mbytes=round(kv_bytes / 1e6, 1), rotating_caches=n_buf, hbm_copy_TBs=HBM_COPY_TBS)
    for k, v in us.items():
        res[f"{k}_us"] = round(v, 2)
    res["multi_TBs"] = round(kv_bytes / us["multi"] / 1e6, 3)  # one pass over K and V
    res["multi_over_one_single"] = round(us["multi"] / (us["singles"] / Tq), 2)
    res["singles_over_multi"] = round(us["singles"] / us["multi"], 2)
    print(json.dumps(res), flush=True)


# (name, N, K, norm, act, bias, residual): the decode step's projections with what each fuses
LINEAR_SHAPES = {
    "gpt2": [("c_attn", 2304, 768, "layer", None, True, False), ("attn.c_proj", 768, 768, None, None, True, True),
             ("c_fc", 3072, 768, "layer", "gelu", True, False), ("mlp.c_proj", 768, 3072, None, None, True, True),
             ("lm_head", 50304, 768, "layer", None, False, False)],
    "llama2-7b": [("qkv_proj", 12288, 4096, "rms", None, False, False),
                  ("o_proj", 4096, 4096, None, None, False, True),
                  ("gate_up_proj", 22016, 4096, "rms", "swiglu", False, False),
                  ("down_proj", 4096, 11008, None, None, False, True)],
}


def bench_linear(model, name, N, K, norm, act, bias, residual, M, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)

    def r(*s):
        return torch.randn(*s, device="cuda", generator=g).to(torch.bfloat16)

    w_bytes = N * K * 2
    n_buf = max(2, math.ceil(512e6 / w_bytes))
    ws = [r(N, K) for _ in range(n_buf)]
    q_bytes = N * K + 4 * N
    n_q = max(2, math.ceil(512e6 / q_bytes))
    qs = [ops.quantize_fp8(ws[i] if i < n_buf else r(N, K)) for i in range(n_q)]
    x_bytes = N * K // 2 + N * K // 32
    n_x = max(2, math.ceil(512e6 / x_bytes))
    xs = [ops.quantize_mxfp4(ws[i] if i < n_buf else r(N, K)) for i in range(n_x)]
    n_out = N // 2 if act == "swiglu" else N
    x, b, res = r(M, K), (r(N) if bias else None), (r(M, n_out) if residual else None)
    nw, nb = (r(K) if norm else None), (r(K) if norm == "layer" else None)

    def hip(i):
        return ops.linear_decode(x, ws[i % n_buf], b, norm=norm, norm_weight=nw, norm_bias=nb, act=act, residual=res)

    def fp8(i):
        return ops.linear_decode(x, qs[i % n_q], b, norm=norm, norm_weight=nw, norm_bias=nb, act=act, residual=res)

    def mxfp4(i):
        return ops.linear_decode(x, xs[i % n_x], b, norm=norm, norm_weight=nw, norm_bias=nb, act=act, residual=res)

    def stock(i):
        h = x
        if norm == "layer":
            h = F.layer_norm(x, (K,), nw, nb, 1e-5)
        elif norm == "rms":
            xf = x.float()
            h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(x.dtype) * nw
        y = F.linear(h, ws[i % n_buf], b)
        if act == "gelu":
            y = F.gelu(y, approximate="tanh")
        elif act == "swiglu":
            gate, up = y.chunk(2, dim=-1)
            y = F.silu(gate) * up
        return y if res is None else y + res

    assert ops.linear_decode_eligible(x, ws[0]) and ops.linear_decode_eligible(x, qs[0])
    assert ops.linear_decode_eligible(x, xs[0])
    err = (hip(0).float() - stock(0).float()).abs().max().item()
    us = _time_us({"hip": hip, "fp8": fp8, "mxfp4": mxfp4, "f_linear": stock}, rounds)
    out = dict(bench="linear_decode", model=model, proj=name, M=M, N=N, K=K, norm=norm, act=act, bias=bias,
               residual=residual, w_mbytes=round(w_bytes / 1e6, 2), rotating_weights=n_buf,
               fp8_w_mbytes=round(q_bytes / 1e6, 2), fp8_rotating_weights=n_q,
               mxfp4_w_mbytes=round(x_bytes / 1e6, 2), mxfp4_rotating_weights=n_x,
               max_abs_diff_vs_f_linear=round(err, 4), hbm_copy_TBs=HBM_COPY_TBS)
    for k, v in us.items():
        out[f"{k}_us"] = round(v, 2)
        out[f"{k}_GBs"] = round({"fp8": q_bytes, "mxfp4": x_bytes}.get(k, w_bytes) / v / 1e3, 1)
    out["hip_over_copy_rate"] = round(out["hip_GBs"] / 1e3 / HBM_COPY_TBS, 3)
    out["fp8_over_copy_rate"] = round(out["fp8_GBs"] / 1e3 / HBM_COPY_TBS, 3)
    out["speedup"] = round(us["f_linear"] / us["hip"], 2)
    out["fp8_over_hip"] = round(us["hip"] / us["fp8"], 2)  # > 1: the FP8 kernel is faster than the bf16 one
    out["mxfp4_over_copy_rate"] = round(out["mxfp4_GBs"] / 1e3 / HBM_COPY_TBS, 3)
    out["mxfp4_over_hip"] = round(us["hip"] / us["mxfp4"], 2)  # > 1: the MXFP4 kernel is faster than the bf16 one
    out["mxfp4_over_fp8"] = round(us["fp8"] / us["mxfp4"], 2)  # > 1: faster than the FP8 one
    print(json.dumps(out), flush=True)


def bench_sample(B, V, top_k, rounds):
    """Device time of one ``ops.sample_tokens`` launch beside ``sample_logits`` on the same logits
    (rotating over 8 logits buffers; both draw their own random numbers)."""
    from orion_amd.models.generation import sample_logits
    from orion_amd.ops.decode import sample_params
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = [(torch.randn(B, V, device="cuda", generator=g) * 2.5).to(torch.bfloat16) for _ in range(8)]
    params = sample_params(0.8, top_k, "cuda")
    seed = torch.tensor([1234], dtype=torch.int64, device="cuda")
    pos = torch.arange(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, 1, dtype=torch.long, device="cuda")

    def hip(i):
        return ops.sample_tokens(logits[i % 8], params=params, seed=seed, positions=pos, out=out)

    def stock(i):
        return sample_logits(logits[i % 8], 0.8, top_k)

    assert ops.sample_tokens_eligible(logits[0])
    us = _time_us({"hip": hip, "sample_logits": stock}, rounds)
    res = dict(bench="sample_tokens", B=B, V=V, top_k=top_k, temperature=0.8)
    for k, v in us.items():
        res[f"{k}_us"] = round(v, 2)
    res["speedup"] = round(us["sample_logits"] / us["hip"], 2)
    print(json.dumps(res), flush=True)


def bench_graph_steady(model, B, prompt_len, new_tokens, weights="bf16"):
    """The graph arm without its capture (and, with FP8 weights, without the quantisation):
    per-token time of the sampling loop on a captured session, and of the replay alone (the rest
    is the sampling launches)."""
    from orion_amd.models.generation import sample_logits
    prompt = torch.randint(0, 50257, (B, prompt_len), device="cuda")
    sess = model.decode_session(B, prompt_len + new_tokens, graph=True, weights=weights)
    logits = sess.prefill(prompt)
    nxt = sample_logits(logits, 1.0, 200)
    sess.step(nxt)  # warm-up + capture
    n = new_tokens - 2
    res = {}
    for what in ("token", "replay"):
        sess.reset()
        logits = sess.prefill(prompt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if what == "token":
                nxt = sample_logits(logits, 1.0, 200)
            logits = sess.step(nxt)
        torch.cuda.synchronize()
        res[what] = (time.perf_counter() - t0) / n
    assert sess.captures == 1
    return res


def bench_generate(B, prompt_len, new_tokens, rounds):
    torch.manual_seed(0)
    model = build_gpt2("gpt2").to("cuda").to(torch.bfloat16).eval()
    prompt = torch.randint(0, 50257, (B, prompt_len), device="cuda")
    arms = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "fused": dict(use_cache="fused"),
            "graph": dict(use_cache="graph"), "graph_device": dict(use_cache="graph", sampler="device"),
            "graph_device_fp8": dict(use_cache="graph", sampler="device", weights="fp8"),
            "graph_device_mxfp4": dict(use_cache="graph", sampler="device", weights="mxfp4"),
            "graph_device_kvfp8": dict(use_cache="graph", sampler="device", kv="fp8")}
    for kw in arms.values():  # warm-up: every shape of every arm
        model.generate(prompt, new_tokens, top_k=200, **kw)
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for name, kw in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(prompt, new_tokens, top_k=200, **kw)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
            assert out.shape == (B, prompt_len + new_tokens)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    res = dict(bench="generate", model="gpt2", B=B, prompt=prompt_len, new_tokens=new_tokens, rounds=rounds)
    for k, v in med.items():
        res[f"{k}_s"] = round(v, 4)
        res[f"{k}_tok_per_s"] = round(B * new_tokens / v, 1)
    res["cached_over_uncached"] = round(med["uncached"] / med["cached"], 2)
    best = min(med["cached"], med["uncached"])  # the faster of the two arms that predate the fused step
    res["fused_over_best_baseline"] = round(best / med["fused"], 2)
    res["graph_over_best_baseline"] = round(best / med["graph"], 2)
    res["graph_device_over_graph"] = round(med["graph"] / med["graph_device"], 2)
    res["graph_device_fp8_over_graph_device"] = round(med["graph_device"] / med["graph_device_fp8"], 2)
    res["graph_device_mxfp4_over_graph_device"] = round(med["graph_device"] / med["graph_device_mxfp4"], 2)
    res["graph_device_kvfp8_over_graph_device"] = round(med["graph_device"] / med["graph_device_kvfp8"], 2)
    steady = bench_graph_steady(model, B, prompt_len, new_tokens)
    res["graph_steady_ms_per_token"] = round(steady["token"] * 1e3, 3)
    res["graph_replay_ms_per_token"] = round(steady["replay"] * 1e3, 3)
    res["graph_sampling_ms_per_token"] = round((steady["token"] - steady["replay"]) * 1e3, 3)
    steady = bench_graph_steady(model, B, prompt_len, new_tokens, weights="fp8")
    res["graph_fp8_replay_ms_per_token"] = round(steady["replay"] * 1e3, 3)
    steady = bench_graph_steady(model, B, prompt_len, new_tokens, weights="mxfp4")
    res["graph_mxfp4_replay_ms_per_token"] = round(steady["replay"] * 1e3, 3)
    print(json.dumps(res), flush=True)


def bench_speculative(k, prompt_len, new_tokens, rounds, top_k=200):
    """``gpt2`` (random init) at B 1: the plain captured session beside speculative sessions with k
    guesses per step, every session built and captured before the timed rounds; each timed run
    is reset + prefill + the whole sampling loop under one seed, so all arms emit the same
    tokens.  Tokens/s are medians over alternating rounds; ``*_tok_per_step`` is the mean number
    of tokens a verify step emitted."""
    torch.manual_seed(0)
    model = build_gpt2("gpt2").to("cuda").to(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(1)
    prompts = {"random": torch.randint(0, 50257, (1, prompt_len), generator=g).to("cuda"),
               "periodic": torch.randint(0, 50257, (1, 8), generator=g).repeat(1, prompt_len // 8).to("cuda")}
    max_len = prompt_len + new_tokens - 1

    def run(sess, prompt):
        sess.reset()
        torch.manual_seed(7)
        return sess.generate(prompt, new_tokens, 0.8, top_k)

    plain = model.decode_session(1, max_len, graph=True, sampler="device")
    want = {name: run(plain, p) for name, p in prompts.items()}
    arms = {"plain": (plain, "random"), "plain_periodic": (plain, "periodic")}
    for name, draft in (("all_correct", want["random"]), ("all_wrong", (want["random"] + 1) % 50257)):
        arms[name] = (model.decode_session(1, max_len, graph=True, sampler="device", speculative=k, draft=draft),
                      "random")
    arms["ngram_periodic"] = (model.decode_session(1, max_len, graph=True, sampler="device", speculative=k),
                              "periodic")
    for name, (sess, pname) in arms.items():  # warm-up and capture; the tokens are the plain loop's
        assert torch.equal(run(sess, prompts[pname]), want[pname]), name
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(rounds):
        for name, (sess, pname) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(sess, prompts[pname])
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    res = dict(bench="speculative", model="gpt2", B=1, k=k, prompt=prompt_len, new_tokens=new_tokens, top_k=top_k,
               temperature=0.8, rounds=rounds)
    med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
    for name, v in med.items():
        res[f"{name}_tok_per_s"] = round(new_tokens / v, 1)
        res[f"{name}_spread"] = round((max(ts[name]) - min(ts[name])) / v, 3)
        sess = arms[name][0]
        if sess.speculative is not None:
            res[f"{name}_tok_per_step"] = round(sess.spec_emitted / sess.spec_steps, 2)
    res["all_correct_over_plain"] = round(med["plain"] / med["all_correct"], 2)
    res["all_wrong_over_plain"] = round(med["plain"] / med["all_wrong"], 2)
    res["ngram_periodic_over_plain_periodic"] = round(med["plain_periodic"] / med["ngram_periodic"], 2)
    print(json.dumps(res), flush=True)


def bench_weight_bytes():
    """Bytes of projection weight a decode session holds, bf16 beside fp8 and mxfp4: ``gpt2`` from
    real sessions (with the relative logit error of the quantised sessions' last step against the
    unquantised model, random init), the Llama-2-7B shape from its projection shapes alone."""
    from orion_amd.models.llama import build_llama
    torch.manual_seed(0)
    model = build_gpt2("gpt2").to("cuda").to(torch.bfloat16).eval()
    prompt = torch.randint(0, 50257, (8, 64), device="cuda")
    s16, s8 = model.decode_session(8, 128), model.decode_session(8, 128, weights="fp8")
    s4 = model.decode_session(8, 128, weights="mxfp4")
    a, b, c = s16.prefill(prompt).float(), s8.prefill(prompt).float(), s4.prefill(prompt).float()
    for tok in torch.randint(0, 50257, (16, 8, 1), device="cuda"):
        a, b, c = s16.step(tok).float(), s8.step(tok).float(), s4.step(tok).float()
    res = dict(bench="decode_weight_bytes", gpt2_bf16_mbytes=round(s16.weight_bytes / 1e6, 1),
               gpt2_fp8_mbytes=round(s8.weight_bytes / 1e6, 1),
               gpt2_fp8_rel_logit_err_vs_bf16_random_init=round(((a - b).norm() / a.norm()).item(), 4),
               gpt2_mxfp4_mbytes=round(s4.weight_bytes / 1e6, 1),
               gpt2_mxfp4_rel_logit_err_vs_bf16_random_init=round(((a - c).norm() / a.norm()).item(), 4))
    with torch.device("meta"):
        shapes = [tuple(w.shape) for _, w in build_llama("llama2-7b").decode_projections()]
    res["llama2_7b_bf16_mbytes"] = round(sum(2 * n * k for n, k in shapes) / 1e6, 1)
    res["llama2_7b_fp8_mbytes"] = round(sum(n * k + 4 * n for n, k in shapes) / 1e6, 1)
    res["llama2_7b_mxfp4_mbytes"] = round(sum(n * k // 2 + n * k // 32 for n, k in shapes) / 1e6, 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=1)
    ap.add_argument("--linear", type=int, default=1)
    ap.add_argument("--sample", type=int, default=1)
    ap.add_argument("--generate", type=int, default=1)
    ap.add_argument("--multi", type=int, default=1)
    ap.add_argument("--speculative", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES), help="decode-kernel shapes, comma-separated")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode.py needs a GPU")
    ops.load_ext(required=True)
    with torch.no_grad():
        if a.kernel:
            for name in a.shapes.split(","):
                bench_kernel(name, rounds=max(a.rounds, 5) * 2, **SHAPES[name])
        if a.multi:
            for name in a.shapes.split(","):
                for Tq in (4, 8):
                    bench_kernel_multi(name, Tq=Tq, rounds=max(a.rounds, 5) * 2, **SHAPES[name])
        if a.linear:
            for model, shapes in LINEAR_SHAPES.items():
                for shape in shapes:
                    for M in (1, 8, 16):
                        bench_linear(model, *shape, M=M, rounds=max(a.rounds, 5))
        if a.sample:
            for V in (50304, 32000):
                for B in (1, 8, 16):
                    for top_k in (200, None):
                        bench_sample(B, V, top_k, rounds=max(a.rounds, 5))
        if a.generate:
            bench_weight_bytes()
            for B in (1, 8):
                bench_generate(B, 64, 256, a.rounds)
            bench_generate(8, 768, 256, a.rounds)  # a long context: where re-running the prefix costs
        if a.speculative:
            for k in (3, 7):
                bench_speculative(k, 64, 256, max(a.rounds, 5))
            bench_speculative(7, 64, 256, max(a.rounds, 5), top_k=1)  # greedy: a random-init model repeats itself


if __name__ == "__main__":
    main()

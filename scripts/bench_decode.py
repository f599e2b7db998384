#!/usr/bin/env python3
"""Generation benchmark: (i) the split-KV decode attention kernel (csrc/attn_decode.hip) beside
torch SDPA on the same cache view, at the GPT-2 and the Llama-GQA decode shapes; (ii) generated
tokens/s of ``gpt2`` with and without the KV cache (prompt 64 + 256 new tokens at B 1 and 8, and
a long-context point, prompt 768 at B 8), the two arms alternating.

The kernel timing rotates over enough distinct caches to exceed the 256 MB Infinity Cache, so
every call streams its K and V from HBM; bytes/s counts the K + V actually read (one pass per
KV head).  Prints one JSON line per measurement.

usage: python scripts/bench_decode.py [--kernel 0|1] [--generate 0|1] [--rounds N]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orion_amd import ops  # noqa: E402
from orion_amd.models.gpt2 import build_gpt2  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X (8.0 TB/s spec)
SHAPES = {"gpt2": dict(B=8, Hq=12, Hkv=12, D=64, T=1024), "llama-gqa": dict(B=8, Hq=32, Hkv=8, D=128, T=4096)}


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
    n_buf = max(2, math.ceil(512e6 / kv_bytes))
    caches = [torch.randn(2, B, T, Hkv, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(n_buf)]
    q = torch.randn(B, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    sdpa = torch.nn.functional.scaled_dot_product_attention
    q4 = q[:, :, None, :]  # (B, Hq, 1, D)

    def hip(i):
        c = caches[i % n_buf]
        return ops.attention_decode(q, c[0], c[1], lens)

    def torch_sdpa(i):
        c = caches[i % n_buf]
        return sdpa(q4, c[0].transpose(1, 2), c[1].transpose(1, 2), enable_gqa=Hq != Hkv)

    err = (hip(0).float() - torch_sdpa(0)[:, :, 0].float()).abs().max().item()
    us = _time_us({"hip": hip, "sdpa": torch_sdpa}, rounds)
    res = dict(bench="decode_kernel", shape=name, B=B, Hq=Hq, Hkv=Hkv, D=D, len=T, kv_mbytes=round(kv_bytes / 1e6, 1),
               rotating_caches=n_buf, max_abs_diff_vs_sdpa=round(err, 5), hbm_copy_TBs=HBM_COPY_TBS)
    for k, v in us.items():
        res[f"{k}_us"] = round(v, 2)
        res[f"{k}_TBs"] = round(kv_bytes / v / 1e6, 3)
    res["hip_over_copy_rate"] = round(res["hip_TBs"] / HBM_COPY_TBS, 3)
    print(json.dumps(res), flush=True)


def bench_generate(B, prompt_len, new_tokens, rounds):
    torch.manual_seed(0)
    model = build_gpt2("gpt2").to("cuda").to(torch.bfloat16).eval()
    prompt = torch.randint(0, 50257, (B, prompt_len), device="cuda")
    arms = {"cached": True, "uncached": False}
    for use_cache in arms.values():  # warm-up: every shape of both arms
        model.generate(prompt, new_tokens, top_k=200, use_cache=use_cache)
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for name, use_cache in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(prompt, new_tokens, top_k=200, use_cache=use_cache)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
            assert out.shape == (B, prompt_len + new_tokens)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    res = dict(bench="generate", model="gpt2", B=B, prompt=prompt_len, new_tokens=new_tokens, rounds=rounds)
    for k, v in med.items():
        res[f"{k}_s"] = round(v, 4)
        res[f"{k}_tok_per_s"] = round(B * new_tokens / v, 1)
    res["cached_over_uncached"] = round(med["uncached"] / med["cached"], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=1)
    ap.add_argument("--generate", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode.py needs a GPU")
    ops.load_ext(required=True)
    with torch.no_grad():
        if a.kernel:
            for name, s in SHAPES.items():
                bench_kernel(name, rounds=max(a.rounds, 5) * 2, **s)
        if a.generate:
            for B in (1, 8):
                bench_generate(B, 64, 256, a.rounds)
            bench_generate(8, 768, 256, a.rounds)  # a long context: where re-running the prefix costs


if __name__ == "__main__":
    main()

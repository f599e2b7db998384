#!/usr/bin/env python3
"""Every generation mode once on ``gpt2-tiny`` and ``llama-tiny`` (B 2, prompt 37, 12 new tokens):
uncached, ``use_cache=True``, ``"fused"``, ``"graph"`` and ``"graph"`` with ``sampler="device"``.
Meant to run under a kernel trace: two commits launch the same kernels when their per-kernel call
counts agree.  Prints one JSON line per (model, mode) with the drawn tokens, which two commits
share under the fixed seed.

usage: python scripts/generate_modes.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orion_amd import ops  # noqa: E402
from orion_amd.models import build_model  # noqa: E402

B, PROMPT, NEW = 2, 37, 12
MODES = {"uncached": dict(use_cache=False), "cached": dict(use_cache=True), "fused": dict(use_cache="fused"),
         "graph": dict(use_cache="graph"), "graph_device": dict(use_cache="graph", sampler="device")}


def main():
    if not torch.cuda.is_available():
        sys.exit("generate_modes.py needs a GPU")
    ops.load_ext(required=True)
    for name in ("gpt2-tiny", "llama-tiny"):
        torch.manual_seed(0)
        model = build_model(name).to("cuda").to(torch.bfloat16).eval()
        for bname, buf in model.named_buffers():
            if bname.startswith("rope_"):
                buf.data = buf.data.float()
        prompt = torch.randint(0, model.config.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(1))
        prompt = prompt.to("cuda")
        for mode, kw in MODES.items():
            torch.manual_seed(3)
            out = model.generate(prompt, NEW, temperature=0.8, top_k=50, **kw)
            torch.cuda.synchronize()
            assert out.shape == (B, PROMPT + NEW) and torch.equal(out[:, :PROMPT], prompt)
            print(json.dumps(dict(model=name, mode=mode, tokens=out[:, PROMPT:].tolist())), flush=True)


if __name__ == "__main__":
    main()

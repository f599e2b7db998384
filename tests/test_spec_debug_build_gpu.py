"""The debug build (orion_amd/_C_debug.so: device-side bounds asserts via ORION_DASSERT) runs the
smallest draft, accept and multi-query attention cases without tripping an assert; a child process
loads it through ORION_AMD_EXT, as in tests/test_sample_debug_build_gpu.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "orion_amd", "_C_debug.so")

SCRIPT = r"""
import torch
from orion_amd import ops
from orion_amd.ops._ext import EXT_PATH
from orion_amd.ops import reference as ref
assert EXT_PATH.endswith("_C_debug.so"), EXT_PATH
ops.load_ext(required=True)
# draft: a match at j = 0 and a row with cur < g
h = torch.tensor([[1, 2, 3, 9, 8, 1, 2, 3], [5, 5, 5, 0, 0, 0, 0, 0]])
cur = torch.tensor([7, 2], dtype=torch.int32)
out = torch.zeros(2, 5, dtype=torch.int64, device="cuda")
ops.spec_draft(h.cuda(), cur.cuda(), out, 3)
assert out.cpu().tolist() == [[3, 9, 8, 1, 2], [5, 5, 5, 5, 5]], out
# accept: a = 1 with room, and a = 3 at the end of the history (columns >= L skipped)
tokens = torch.tensor([[10, 7, 2, 3], [10, 7, 8, 9]])
target = torch.tensor([[7, 8, 9, 6], [7, 8, 9, 6]])
start = torch.tensor([4, 6], dtype=torch.int32)
stop = torch.tensor([100, 100], dtype=torch.int32)
hist = torch.full((2, 8), -1, dtype=torch.int64, device="cuda")
lens = (start + 4).cuda()
ops.spec_accept(tokens.cuda(), target.cuda(), start.cuda(), lens, stop.cuda(), hist)
rh, rl = torch.full((2, 8), -1, dtype=torch.int64), start + 4
ref.spec_accept(tokens, target, start, rl, stop, rh)
assert torch.equal(hist.cpu(), rh) and torch.equal(lens.cpu(), rl)
# multi-query attention: Tq 3, GQA 4/2, D 64, a short row, a row past the first tile and one past Tmax
g = torch.Generator().manual_seed(0)
q = torch.randn(3, 3, 4, 64, generator=g).to(torch.bfloat16).cuda()
kc = torch.randn(3, 160, 2, 64, generator=g).to(torch.bfloat16).cuda()
vc = torch.randn(3, 160, 2, 64, generator=g).to(torch.bfloat16).cuda()
kv = torch.tensor([2, 130, 161], dtype=torch.int32, device="cuda")
want = ref.attention_decode_multi(q.float(), kc.float(), vc.float(), kv)
for splits in (1, 2, 0):
    # a sanity bound of a few bf16 ulps of |o| <= 4 (2^-6 each): the numerics are measured on the
    # release build by tests/test_attention_decode_multi_gpu.py, this run is about the asserts
    o = ops.attention_decode_multi(q, kc, vc, kv, splits=splits)
    assert (o.float() - want).abs().max().item() < 0.05, splits
torch.cuda.synchronize()
print("debug build ok")
"""


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_speculative_kernels_pass_their_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

"""The debug build (orion_amd/_C_debug.so: device-side bounds asserts via ORION_DASSERT) runs the
sampling kernel on ragged rows, staged in LDS and not, without tripping an assert; a child process
loads it through ORION_AMD_EXT, as in tests/test_debug_build_gpu.py."""
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
g = torch.Generator().manual_seed(0)
for B, V, pad in ((3, 1001, 3), (2, 66001, 0), (1, 1, 0)):
    host = torch.randn(B, V + pad, generator=g).to(torch.bfloat16)
    logits = host.cuda()[:, pad:]
    pos = torch.arange(B, dtype=torch.int32, device="cuda") + 5
    hist = torch.zeros(B, 6, dtype=torch.long, device="cuda")
    u = torch.zeros(B, device="cuda")
    for k in (None, 50):
        tok = ops.sample_tokens(logits, 0.9, k, seed=11, positions=pos, history=hist, u_out=u)
        assert 0 <= int(tok.min()) and int(tok.max()) < V
        assert bool(ref.sample_keep_mask(host[:, pad:], k).gather(1, tok.cpu()).all()), (B, V, k)
        assert torch.equal(u.cpu(), ref.philox_uniform(11, pos.cpu()))
        assert torch.equal(hist[0, 5:], tok[0])
torch.cuda.synchronize()
print("debug build ok")
"""


@pytest.mark.skipif(not os.path.isfile(DEBUG_SO),
                    reason="debug build not present (ORION_AMD_DEBUG=1 python -m orion_amd.build)")
def test_debug_build_sampling_passes_its_bounds_asserts():
    env = dict(os.environ, ORION_AMD_EXT=DEBUG_SO,
               PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    out = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True,
                         timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build ok" in out.stdout

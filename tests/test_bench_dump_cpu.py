"""``bench.py --dump-outputs DIR`` on the CPU rehearsal path: the last timed step's loss, gradient
norm and samples of the weights / fp32 master / gradients land as float32 ``.npy`` files, the run
selects deterministic mode, and two runs with the same arguments write identical outputs."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"loss", "grad_norm", "params_sample", "master_sample", "grads_sample"}


def _run(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in
           ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ORION_DETERMINISTIC")}
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--device", "cpu", "--model", "gpt2-tiny",
                          "--seq-len", "64", "--micro-batch", "2", "--steps", str(steps), "--warmup", "1",
                          "--dump-outputs", str(out_dir)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    rec, a = _run(tmp_path / "a", 2)
    assert set(a) == NAMES
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["deterministic"] is True
    # the dumped loss is the one the result line reports (rounded there to 4 places)
    assert abs(float(a["loss"][0]) - rec["loss"]) <= 5.1e-5
    assert a["params_sample"].size == a["master_sample"].size == a["grads_sample"].size > 1000
    assert a["grad_norm"][0] > 0 and np.abs(a["grads_sample"]).max() > 0
    # same arguments: same inputs and the same outputs, bit for bit
    _, b = _run(tmp_path / "b", 2)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)

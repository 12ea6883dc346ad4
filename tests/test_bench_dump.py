"""bench.py --dump-outputs (-m gpu): the arrays written are what the last timed step returned, and two runs with the same arguments write the same
arrays bit for bit (the inputs are seeded, so two builds can be compared output for output)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("R", "t", "n_match", "n_inliers", "ok")


def _bench(dump_dir, batch, steps):
    # batch 16: two sub-batch streams and the certificate deferred by one call, as in the default headline configuration (two alternating output sets)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch),
           "--no-extras", "--no-traffic", "--no-cpu-baseline", "--no-stream", "--no-rccl-check", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    js = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(js) == 1, r.stdout[-800:]
    return json.loads(js[0]), {k: np.load(os.path.join(dump_dir, k + ".npy")) for k in NAMES}


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    batch, steps = 16, 3
    line, a = _bench(tmp_path / "a", batch, steps)
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert a["R"].shape == (batch, 3, 3) and a["t"].shape == (batch, 3, 1) and all(a[k].shape == (batch,) for k in ("n_match", "n_inliers", "ok"))
    assert all(v.dtype == np.float64 for v in a.values())
    assert int(a["ok"].sum()) == line["poses_ok_per_step"]
    # the line's result records are packed from the last timed step's outputs (batch (steps - 1) mod 4 of the rotated resident batches): rebuilt here
    # from the dumped arrays, they must hash the same
    rec = np.zeros((batch, 16), np.float64)
    rec[:, 0] = ((steps - 1) % 4) * batch + np.arange(batch)
    rec[:, 1], rec[:, 2], rec[:, 3] = a["ok"], a["n_match"], a["n_inliers"]
    rec[:, 4:13] = a["R"].reshape(batch, 9)
    rec[:, 13:16] = a["t"].reshape(batch, 3)
    assert hashlib.sha256(rec.tobytes()).hexdigest() == line["multi_gpu"]["records_sha256"]
    _, b = _bench(tmp_path / "b", batch, steps)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k

"""bench.py without --full (-m gpu): a plain run sets up, warms up, times its steps and prints the line, and measures none of the figures that
take runs of their own; --full brings them back (here the single-stream per-kernel pass: kernels, roofline, single-stream step time)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    # batch 16: two sub-batch streams and the deferred certificate, as in the default headline configuration
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    js = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(js) == 1, r.stdout[-800:]
    return json.loads(js[0])


def test_plain_run_measures_the_headline_only():
    a = _bench()
    assert a["full"] is False and a["steps"] == 3 and a["warmup"] == 1 and a["value"] > 0 and a["ms_per_step"] > 0
    assert a["config"]["sub_batch_streams"] == 2 and a["poses_ok_per_step"] >= 15
    assert a["precision_guarantee"]["certificate"]["calls"] == 4          # warm-up + timed steps, no other pass
    assert a["extra_configs"] == [] and "cpu_baseline" not in a
    assert a["kernels"] == [] and "roofline" not in a and a["config"]["single_stream_ms_per_step"] is None
    assert a["traffic"]["measured_hbm_mb_per_step"] is None and a["pcie_inclusive"]["stream"] is None
    assert a["multi_gpu"]["rccl_selfcheck_world1"] is None


def test_full_run_adds_the_per_kernel_pass_and_computes_the_same_records():
    a = _bench("--no-rccl-check")
    b = _bench("--full", "--no-extras", "--no-traffic", "--no-cpu-baseline", "--no-stream", "--no-rccl-check")
    assert b["full"] is True and b["config"]["single_stream_ms_per_step"] > 0
    assert b["precision_guarantee"]["certificate"]["calls"] == 8          # the single-stream pass's calls as well
    names = {k["name"] for k in b["kernels"]}
    assert b["roofline"]["kernel"] in names and len(names) > 5
    assert b["multi_gpu"]["records_sha256"] == a["multi_gpu"]["records_sha256"]   # the extra pass changes nothing the timed steps return

"""Cost of the certificate's re-run ladder and of GN_PREC_F16X2_F16X2_ATTN (mode 5), in one process on one GPU; prints one JSON line.

    python tools/bench_ladder.py [--batch 32] [--kpts 1024] [--reps 3] [--out FILE]

  * certified pairs/s of the headline mode with the ladder off and on, for margin-built, mid-margin and default-init weights (32 x 1024 per call);
  * the per-pair cost of a re-run at each rung -- a matcher call of n pairs in mode-5 arithmetic (middle level) and in exact f32 -- at n = 1, 4, 16;
  * mode 5 against GN_PREC_F32 in pairs/s at the full batch.
Every figure is the median of --reps timed repetitions after one warm-up call.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gisnav_amd import _lib  # noqa: E402
from gisnav_amd.engine import PoseEngine  # noqa: E402
from gisnav_amd.synthetic import make_pair  # noqa: E402
from gisnav_amd.weights import default_init_state_dict, synthetic_state_dict  # noqa: E402

MID_MARGIN = dict(ffn_out_std=1.2e-3, final_scale=12.0, matchability_bias=2.0, matchability_std=0.05)
FAMILIES = {"margin_built": (lambda: synthetic_state_dict(0), 0.5), "mid_margin": (lambda: synthetic_state_dict(0, **MID_MARGIN), 0.01),
            "default_init": (lambda: default_init_state_dict(0), 0.0)}
HEADLINE = "f16x2_f16_attn"


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _match(eng, inp):
    return lambda: eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, K = a.batch, a.kpts
    pairs = [make_pair(9000 + i, n_q=K - 7 * (i % 5), n_r=K - 13 * (i % 3)) for i in range(B)]
    cal = [make_pair(9500 + i, n_q=K, n_r=K - 24) for i in range(B)]
    res = {"source_digest": _lib.library_digest(), "batch": B, "kpts": K, "reps": a.reps, "certified_pairs_per_s": {}, "rerun_ms_per_pair": {}}
    for name, (make, th) in FAMILIES.items():
        sd = make()
        eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
        inp = eng.stage_inputs(pairs)
        row = {}
        for ladder in (False, True):
            eng.set_certify("off")
            eng.set_certify_ladder(ladder)
            c = eng.calibrate_certify(eng.stage_inputs(cal), safety=4.0)
            eng.set_certify("rerun")
            eng.certify_stats(reset=True)
            t = _timed(_match(eng, inp), a.reps)
            st, ls = eng.certify_stats(), eng.certify_ladder_stats()
            row["ladder_on" if ladder else "ladder_off"] = {"pairs_per_s": B / t, "eps": c["eps"], "eps_mid": c.get("eps_mid"),
                                                            "flagged_margin_per_call": st["flagged_margin"] / max(1, st["calls"]),
                                                            "f32_rerun_per_call": st["rerun_pairs"] / max(1, st["calls"]),
                                                            "mid_certified_per_call": ls["mid_certified"] / max(1, st["calls"])}
        res["certified_pairs_per_s"][name] = row
        del eng
    sd = synthetic_state_dict(0)
    rates = {}
    for prec in ("f16x2_f16x2_attn", "f32"):
        eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=0.5)
        rates[prec] = B / _timed(_match(eng, eng.stage_inputs(pairs)), a.reps)
        for n in (1, 4, 16):
            if n <= B:
                inp = eng.stage_inputs(pairs[:n])
                res["rerun_ms_per_pair"].setdefault("middle" if prec != "f32" else "f32", {})[str(n)] = 1e3 * _timed(_match(eng, inp), a.reps) / n
        del eng
    res["pairs_per_s_at_batch"] = rates
    res["mode5_over_f32"] = rates["f16x2_f16x2_attn"] / rates["f32"]
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Cost of lens distortion in the PnP stage (DESIGN.md "Lens distortion"): the 32-pair step (gn_estimate, two sub-batch streams as the bench runs,
1024 keypoints per side, headline precision) with distortion off and on, interleaved in one process and timed by HIP events; the PnP stage alone
(k_pnp_hyp + k_pnp_refine) on the same batch's correspondences, off and on; and, with --parent-lib, distortion off against a library built from the
parent commit, to show that the `DIST = false` kernels did not move.  One process holds one library, so the last comparison alternates child
processes (this build, parent, this build, parent, ...), each of which measures the off path only.  Medians over 24 alternating repetitions; the
spread (90th - 10th percentile) of the off path is printed next to every difference.

    python tools/dist_cost.py [out.json] [--parent-lib /path/to/parent/libgisnav_amd.so]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = (-0.05, 0.002, 5e-4, -3e-4, 0.0)
B, SUB, REPS = 32, 2, 24


def med(v):
    return float(np.median(v))


def spread(v):
    return float(np.percentile(v, 90) - np.percentile(v, 10))


def measure(with_on: bool) -> dict:
    import torch
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import K_MATRIX, make_pair
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    inp = eng.stage_inputs([make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)])
    eng.set_substreams(SUB)
    out = eng.alloc_outputs(B)
    modes = (False, True) if with_on else (False,)

    def setd(on):
        if with_on:
            eng.set_distortion(D if on else None)

    for on in modes * 2:
        setd(on)
        for _ in range(5):
            eng.estimate(inp, K_MATRIX, out=out)
    eng.flush(); torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for rep in range(REPS):
        for on in (modes if rep % 2 == 0 else modes[::-1]):
            setd(on)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                eng.estimate(inp, K_MATRIX, out=out)
            eng.flush()
            e1.record(); e1.synchronize()
            ms[on].append(e0.elapsed_time(e1) / 10)
    # the PnP stage alone on the staged points of this batch
    setd(False)
    idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])
    pnp = {m: [] for m in modes}
    for rep in range(REPS):
        for on in (modes if rep % 2 == 0 else modes[::-1]):
            setd(on)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                eng.pnp_ransac(obj, mkp, nm, K_MATRIX, min_pts=15)
            e1.record(); e1.synchronize()
            pnp[on].append(e0.elapsed_time(e1) / 20)
    setd(False)
    res = dict(step_off_ms=med(ms[False]), step_off_spread_ms=spread(ms[False]), pnp_off_ms=med(pnp[False]), pnp_off_spread_ms=spread(pnp[False]),
               inliers_off=[int(x) for x in eng.estimate(inp, K_MATRIX)["n_inliers"].cpu()[:4]])
    if with_on:
        res.update(step_on_ms=med(ms[True]), step_delta_pct=100.0 * (med(ms[True]) / med(ms[False]) - 1.0),
                   pnp_on_ms=med(pnp[True]), pnp_delta_pct=100.0 * (med(pnp[True]) / med(pnp[False]) - 1.0))
    eng.set_substreams(1)
    del eng
    return res


def main():
    args = [a for a in sys.argv[1:]]
    if "--child-off" in args:                                   # one off-only measurement with whatever library GISNAV_AMD_LIB names
        if os.environ.get("GISNAV_AMD_ALLOW_STALE") == "1":     # an older library: bind only what it exports (the off path needs nothing newer)
            import ctypes
            import torch  # noqa: F401  (first: the library must share torch's HIP runtime, see _lib.load)
            from gisnav_amd import _lib
            raw = ctypes.CDLL(_lib.LIB_PATH)
            for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
                del _lib.SIGNATURES[name]
        print("CHILD " + json.dumps(measure(False)), flush=True)
        return
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    res = {"this_build": measure(True)}
    print("this_build", json.dumps(res["this_build"]), flush=True)
    if parent:
        runs = {"this": [], "parent": []}
        for rep in range(3):
            for who in (("this", "parent") if rep % 2 == 0 else ("parent", "this")):
                env = dict(os.environ)
                if who == "parent":
                    env.update(GISNAV_AMD_LIB=parent, GISNAV_AMD_ALLOW_STALE="1")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-off"], env=env, capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit(f"child ({who}) failed ({r.returncode}): {r.stderr[-800:]}")
                runs[who].append(json.loads(line[0][6:]))
                print(who, line[0][6:], flush=True)
        cmp_ = {}
        for key in ("step_off_ms", "pnp_off_ms"):
            a, b = [x[key] for x in runs["this"]], [x[key] for x in runs["parent"]]
            cmp_[key] = dict(this=a, parent=b, this_median=med(a), parent_median=med(b), delta_pct=100.0 * (med(a) / med(b) - 1.0))
        cmp_["same_inliers"] = all(x["inliers_off"] == runs["parent"][0]["inliers_off"] for x in runs["this"] + runs["parent"])
        res["off_against_parent"] = cmp_
        print("off_against_parent", json.dumps(cmp_), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

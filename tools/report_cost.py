"""Cost of the pose stage's report.

  * on: gn_estimate_report against gn_estimate of the same build, interleaved in one process and timed by HIP events, at B = 32 (one stream, and two
    sub-batch streams as the bench runs) and B = 1, 1024 keypoints per side, headline precision; and the PnP stage alone (k_pnp_hyp + k_pnp_refine
    [+ k_pnp_report]) on the same batch's correspondences.  Medians over 24 alternating repetitions.
  * off, with --parent-lib PATH: the 32-pair step (gn_estimate, two sub-batch streams) and the PnP stage of this build against a library built from
    the parent commit, as alternating child processes (three each), with both builds' run-to-run spreads.

    python tools/report_cost.py [out.json] [--parent-lib PATH]
"""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

med = lambda v: float(np.median(v))  # noqa: E731
spread = lambda v: float(np.percentile(v, 90) - np.percentile(v, 10))  # noqa: E731


def _setup(B, sub):
    import torch  # noqa: F401
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import make_pair
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    inp = eng.stage_inputs([make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)])
    eng.set_substreams(sub)
    return eng, inp


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / inner


def measure_on():
    import torch
    from gisnav_amd.synthetic import K_MATRIX
    res = {}
    for B, sub in ((32, 1), (32, 2), (1, 1)):
        eng, inp = _setup(B, sub)
        outs = {False: eng.alloc_outputs(B), True: eng.alloc_outputs(B, report=True)}
        inner = 10 if B == 32 else 50
        for rep_ in (False, True, False, True):
            for _ in range(5):
                eng.estimate(inp, K_MATRIX, out=outs[rep_], report=rep_)
        eng.flush(); torch.cuda.synchronize()
        ms = {False: [], True: []}
        for r in range(24):
            for rep_ in ((False, True) if r % 2 == 0 else (True, False)):
                def step(rep_=rep_):
                    eng.estimate(inp, K_MATRIX, out=outs[rep_], report=rep_)
                ms[rep_].append(_timed_flush(eng, step, inner))
        # the PnP stage alone on the staged points of this batch
        eng.set_substreams(1)
        idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])
        rout = eng._alloc_report(B, obj.shape[1])
        pnp = {False: [], True: []}
        for r in range(24):
            for rep_ in ((False, True) if r % 2 == 0 else (True, False)):
                kw = dict(report=True, report_out=rout) if rep_ else {}
                pnp[rep_].append(_timed(lambda: eng.pnp_ransac(obj, mkp, nm, K_MATRIX, min_pts=15, **kw), 20))
        got = eng.estimate(inp, K_MATRIX, report=True)
        torch.cuda.synchronize()
        key = f"B{B}_sub{sub}"
        res[key] = dict(estimate_ms=med(ms[False]), estimate_report_ms=med(ms[True]), estimate_spread_ms=spread(ms[False]),
                        estimate_report_spread_ms=spread(ms[True]), delta_pct=100.0 * (med(ms[True]) / med(ms[False]) - 1.0),
                        pnp_ms=med(pnp[False]), pnp_report_ms=med(pnp[True]), pnp_spread_ms=spread(pnp[False]),
                        pnp_delta_us=1000.0 * (med(pnp[True]) - med(pnp[False])),
                        matches=[int(x) for x in got["n_match"].cpu()[:4]], inliers=[int(x) for x in got["n_inliers"].cpu()[:4]])
        print(key, json.dumps(res[key]), flush=True)
        del eng
    return res


def _timed_flush(eng, step, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        step()
    eng.flush()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / inner


def measure_off():
    """The calls every build has: the 32-pair gn_estimate step on two sub-batch streams, and gn_pnp_ransac on its correspondences."""
    import torch
    from gisnav_amd.synthetic import K_MATRIX
    eng, inp = _setup(32, 2)
    out = eng.alloc_outputs(32)
    step = lambda: eng.estimate(inp, K_MATRIX, out=out)  # noqa: E731
    for _ in range(10):
        step()
    eng.flush(); torch.cuda.synchronize()
    ms = [_timed_flush(eng, step, 10) for _ in range(48)]
    eng.set_substreams(1)
    idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])
    pnp = [_timed(lambda: eng.pnp_ransac(obj, mkp, nm, K_MATRIX, min_pts=15), 20) for _ in range(48)]
    res = dict(step_ms=med(ms), step_p10_ms=float(np.percentile(ms, 10)), step_p90_ms=float(np.percentile(ms, 90)), pnp_ms=med(pnp),
               pnp_p10_ms=float(np.percentile(pnp, 10)), pnp_p90_ms=float(np.percentile(pnp, 90)),
               inliers=[int(x) for x in eng.estimate(inp, K_MATRIX)["n_inliers"].cpu()[:4]])
    del eng
    return res


def child(env_lib):
    env = dict(os.environ)
    if env_lib:
        env.update(GISNAV_AMD_LIB=env_lib, GISNAV_AMD_ALLOW_STALE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-off"], env=env, capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"child ({env_lib or 'this build'}) failed ({r.returncode}): {r.stderr[-800:]}")
    return json.loads(line[0][6:])


def main():
    args = list(sys.argv[1:])
    if "--child-off" in args:                                        # one measurement with whatever library GISNAV_AMD_LIB names
        if os.environ.get("GISNAV_AMD_ALLOW_STALE") == "1":          # another library: bind only what it exports
            import ctypes
            import torch  # noqa: F401  (first: the library must share torch's HIP runtime, see _lib.load)
            from gisnav_amd import _lib
            raw = ctypes.CDLL(_lib.LIB_PATH)
            for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
                del _lib.SIGNATURES[name]
        print("CHILD " + json.dumps(measure_off()), flush=True)
        return
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    res = {"on": measure_on()}
    if parent:
        runs = {"this": [], "parent": []}
        for r in range(3):
            for who in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                runs[who].append(child(parent if who == "parent" else None))
                print(who, json.dumps(runs[who][-1]), flush=True)
        cmp_ = {}
        for key in ("step_ms", "pnp_ms"):
            a, b = [x[key] for x in runs["this"]], [x[key] for x in runs["parent"]]
            cmp_[key] = dict(this=a, parent=b, this_median=med(a), parent_median=med(b), delta_pct=100.0 * (med(a) / med(b) - 1.0),
                             this_run_to_run_pct=100.0 * (max(a) - min(a)) / med(a), parent_run_to_run_pct=100.0 * (max(b) - min(b)) / med(b))
        for who in runs:
            cmp_[f"{who}_step_p10_p90_ms"] = [min(x["step_p10_ms"] for x in runs[who]), max(x["step_p90_ms"] for x in runs[who])]
        cmp_["same_inliers"] = all(x["inliers"] == runs["parent"][0]["inliers"] for x in runs["this"] + runs["parent"])
        res["off_against_parent"] = cmp_
        print("off_against_parent", json.dumps(cmp_), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

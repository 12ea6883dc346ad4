"""Cost of iterations_count in the PnP stage (DESIGN.md "RANSAC beyond 16 hypotheses"), timed by HIP events, interleaved in one process:

  * the PnP stage alone (gn_pnp_ransac) at counts 10 (the two classic launches), 64, 100, 300, 1000 and 4096, for B = 1 and B = 32, on
    (a) the bench's clean correspondences (matcher output of 1024-keypoint synthetic pairs: the loop adapts to a handful of iterations) and
    (b) scene-A-like lists (60 correspondences, half of them gross outliers: the loop needs ~145);
  * the early-stop cost: on (a), 4096 requested against one round requested -- what the launches that return at once cost, per skipped round;
  * with --parent-lib: the 32-pair step (gn_estimate, two sub-batch streams, headline precision) and the PnP stage at the default count
    against a library built from the parent commit.  One process holds one library, so child processes alternate (this, parent, this, ...);
  * with --round-lib R=/path/to/lib (repeatable): the same PnP figures from libraries built with another round size
    (hipcc ... -DGN_RANSAC_ROUND=R for gn_api.hip and gn_pnp.hip), each in a child process.

Medians over alternating repetitions; the spread is the 90th minus the 10th percentile.

    python tools/ransac_cost.py [out.json] [--parent-lib PATH] [--round-lib 32=PATH] [--round-lib 128=PATH]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SUB, REPS = 32, 2, 12
COUNTS = (10, 64, 100, 300, 1000, 4096)


def med(v):
    return float(np.median(v))


def spread(v):
    return float(np.percentile(v, 90) - np.percentile(v, 10))


def outlier_scene(seed, n=60, outliers=0.5):
    """tests/golden/make_ransac_iters_golden.py::scene (seed 100 is the fixture's scene A)."""
    from gisnav_amd.synthetic import make_pair
    rng = np.random.default_rng(seed)
    p = make_pair(9000 + seed, n_q=max(n, 64), n_r=max(4 * n, 256))
    m = np.nonzero(p.gt_q2r >= 0)[0][:n]
    q = p.kp_q[m].astype(np.float32).copy()
    r = p.kp_r[p.gt_q2r[m]].astype(np.float32).copy()
    k = int(outliers * len(q))
    q[rng.permutation(len(q))[:k]] = rng.uniform(0, 480, (k, 2)).astype(np.float32)
    x, y = np.transpose(np.floor(r).astype(int))
    return np.hstack((r, p.dem[y, x].reshape(-1, 1))).astype(np.float32), q


def time_pnp(eng, obj, img, n, counts, min_pts, reps=REPS, inner=5):
    """{count: (median ms, spread ms)} of gn_pnp_ransac on the given lists, the counts interleaved; (niters, evaluated) of pair 0 per count."""
    import torch
    from gisnav_amd.synthetic import K_MATRIX
    for c in counts:
        eng.pnp_ransac(obj, img, n, K_MATRIX, iterations=c, min_pts=min_pts)
    torch.cuda.synchronize()
    ms = {c: [] for c in counts}
    for rep in range(reps):
        for c in (counts if rep % 2 == 0 else counts[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                eng.pnp_ransac(obj, img, n, K_MATRIX, iterations=c, min_pts=min_pts)
            e1.record(); e1.synchronize()
            ms[c].append(e0.elapsed_time(e1) / inner)
    out = {}
    for c in counts:
        eng.pnp_ransac(obj, img, n, K_MATRIX, iterations=c, min_pts=min_pts)
        niters, evaluated = eng.ransac_last_counts(obj.shape[0]) if hasattr(eng.lib, "gn_ransac_last_counts") else ([-1], [-1])
        out[str(c)] = dict(ms=med(ms[c]), spread_ms=spread(ms[c]), niters=int(niters[0]), evaluated=int(evaluated[0]))
    return out


def measure(with_counts: bool, round_size: int = 64) -> dict:
    import torch
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import K_MATRIX, make_pair
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    inp = eng.stage_inputs([make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)])
    eng.set_substreams(SUB)
    out = eng.alloc_outputs(B)
    for _ in range(10):
        eng.estimate(inp, K_MATRIX, out=out)
    eng.flush(); torch.cuda.synchronize()
    step = []
    for rep in range(2 * REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            eng.estimate(inp, K_MATRIX, out=out)
        eng.flush()
        e1.record(); e1.synchronize()
        step.append(e0.elapsed_time(e1) / 10)
    eng.set_substreams(1)
    idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])
    counts = tuple(sorted(set(COUNTS + (round_size,)))) if with_counts else (10,)
    res = dict(step_default_ms=med(step), step_default_spread_ms=spread(step),
               step_default_p10_ms=float(np.percentile(step, 10)), step_default_p90_ms=float(np.percentile(step, 90)),
               inliers_default=[int(x) for x in eng.estimate(inp, K_MATRIX)["n_inliers"].cpu()[:4]],
               clean_B32=time_pnp(eng, obj, mkp, nm, counts, 15))
    if with_counts:
        res["clean_B1"] = time_pnp(eng, obj[:1], mkp[:1], nm[:1], counts, 15)
        scenes = [outlier_scene(100 + i) for i in range(B)]
        o = torch.from_numpy(np.stack([s[0] for s in scenes])).to(eng.device)
        u = torch.from_numpy(np.stack([s[1] for s in scenes])).to(eng.device)
        n = torch.full((B,), o.shape[1], dtype=torch.int32, device=eng.device)
        res["outliers_B32"] = time_pnp(eng, o, u, n, counts, 5)
        res["outliers_B1"] = time_pnp(eng, o[:1], u[:1], n[:1], counts, 5)
        # the launches of rounds that return at once: 4096 requested against one round requested, on lists that stop inside the first round
        skipped = -(-4096 // round_size) - 1
        for key in ("clean_B32", "clean_B1"):
            t = res[key]
            t["early_return_us_per_skipped_round"] = 1000.0 * (t["4096"]["ms"] - t[str(round_size)]["ms"]) / skipped
        res["round_size"] = round_size
    del eng
    return res


def child(env_lib, flag, round_size=64):
    env = dict(os.environ, GISNAV_RANSAC_COST_ROUND=str(round_size))
    if env_lib:
        env.update(GISNAV_AMD_LIB=env_lib, GISNAV_AMD_ALLOW_STALE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), flag], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"child ({env_lib or 'this build'}) failed ({r.returncode}): {r.stderr[-800:]}")
    return json.loads(line[0][6:])


def main():
    args = list(sys.argv[1:])
    if "--child-default" in args or "--child-counts" in args:       # one measurement with whatever library GISNAV_AMD_LIB names
        if os.environ.get("GISNAV_AMD_ALLOW_STALE") == "1":          # another library: bind only what it exports
            import ctypes
            import torch  # noqa: F401  (first: the library must share torch's HIP runtime, see _lib.load)
            from gisnav_amd import _lib
            raw = ctypes.CDLL(_lib.LIB_PATH)
            for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
                del _lib.SIGNATURES[name]
        print("CHILD " + json.dumps(measure("--child-counts" in args, int(os.environ.get("GISNAV_RANSAC_COST_ROUND", "64")))), flush=True)
        return
    parent, round_libs = None, {}
    while "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    while "--round-lib" in args:
        i = args.index("--round-lib")
        r, path = args[i + 1].split("=", 1)
        round_libs[r] = os.path.abspath(path)
        del args[i:i + 2]
    res = {"this_build": measure(True)}
    print("this_build", json.dumps(res["this_build"]), flush=True)
    for r, path in round_libs.items():
        res[f"round_{r}"] = child(path, "--child-counts", int(r))
        print(f"round_{r}", json.dumps(res[f"round_{r}"]), flush=True)
    if parent:
        runs = {"this": [], "parent": []}
        for rep in range(3):
            for who in (("this", "parent") if rep % 2 == 0 else ("parent", "this")):
                runs[who].append(child(parent if who == "parent" else None, "--child-default"))
                print(who, json.dumps(runs[who][-1]), flush=True)
        cmp_ = {}
        for key, get in (("step_default_ms", lambda x: x["step_default_ms"]), ("pnp_default_ms", lambda x: x["clean_B32"]["10"]["ms"])):
            a, b = [get(x) for x in runs["this"]], [get(x) for x in runs["parent"]]
            cmp_[key] = dict(this=a, parent=b, this_median=med(a), parent_median=med(b), delta_pct=100.0 * (med(a) / med(b) - 1.0))
        cmp_["this_step_p10_p90_ms"] = [min(x["step_default_p10_ms"] for x in runs["this"]), max(x["step_default_p90_ms"] for x in runs["this"])]
        cmp_["same_inliers"] = all(x["inliers_default"] == runs["parent"][0]["inliers_default"] for x in runs["this"] + runs["parent"])
        res["default_against_parent"] = cmp_
        print("default_against_parent", json.dumps(cmp_), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

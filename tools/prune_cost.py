"""Cost of LightGlue point pruning (gn_set_width_pruning; DESIGN.md "Point pruning") -> profiles/width_pruning.json, under the loaded library's digest.

Two steps in the headline precision ("f16x2_f16_attn") with certification off: 32 pairs x 1024 keypoints and 8 pairs x 2048.

  (b), (c) in ONE process per shape, the three settings interleaved and timed by HIP events around gn_estimate:
      off       pruning unset
      neutral   on with min_kpts above N: nothing is ever pruned -- the pure overhead of the extra launches (k_prune_init, one k_prune and one
                list rebuild per layer, k_unprune_idx) and of the cross tail -> next self projection fusion that pruning gives up
      half      on with test weights whose layer-2 matchability bias sits at the median of that layer's z (taken from the CPU restatement of the
                batch's first pair, tests/width_pruning_ref.py), min_kpts 256: about half of every side leaves behind the third layer; step time and
                the mean per-layer kept counts
  (a) with --parent-tree DIR (a built checkout of the parent commit): `bench.py --dump-outputs` of this tree and of the parent as alternating child
      processes (pruning unset, everything else the bench's default), the dumped arrays compared for equality and the step times side by side.

    python tools/prune_cost.py [out.json] [--parent-tree DIR] [--bench-steps K]
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRECISION = "f16x2_f16_attn"
SHAPES = {"32x1024": (32, 1024), "8x2048": (8, 2048)}
HALF_LAYER, HALF_MIN_KPTS, WC = 2, 256, 0.99
med = lambda v: float(np.median(v))  # noqa: E731
spread = lambda v: float(np.percentile(v, 90) - np.percentile(v, 10))  # noqa: E731


def half_weights(pair):
    """synthetic_state_dict(0) with matchability bias +30 on every layer (kept by all) but HALF_LAYER, whose bias puts the threshold at the median
    of its z over both sides of `pair` (f32 CPU restatement; the weight is scaled 100x so that the cut is not a near-tie of thousands of rows)."""
    import torch
    import width_pruning_ref as wp
    from gisnav_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(0)
    for i in range(9):
        sd[f"log_assignment.{i}.matchability.bias"] = np.array([30.0], np.float32)
    wk = f"log_assignment.{HALF_LAYER}.matchability.weight"
    sd[wk] = (100.0 * sd[wk]).astype(np.float32)
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    r = wp.forward(sd, wp.sift_inputs(pair), "sift", width_confidence=WC, min_kpts=HALF_MIN_KPTS, dtype=torch.float32, stop_before_layer=HALF_LAYER + 1)
    u = np.concatenate([r["z"][(HALF_LAYER, s)].numpy() - 30.0 for s in (0, 1)])
    sd[f"log_assignment.{HALF_LAYER}.matchability.bias"] = np.array([wp.tau(WC) - float(np.median(u))], np.float32)
    return sd


def measure(name, reps=12, inner=5):
    import torch
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import K_MATRIX, make_pair
    B, N = SHAPES[name]
    pairs = [make_pair(100 + i, n_q=N, n_r=N) for i in range(B)]
    eng = PoseEngine(0, max_batch=B, max_kpts=N, precision=PRECISION, state_dict=half_weights(pairs[0]))
    eng.set_certify("off")
    inp = eng.stage_inputs(pairs)
    out = eng.alloc_outputs(B)
    settings = {"off": (-1.0, None), "neutral": (WC, 2 * N), "half": (WC, HALF_MIN_KPTS)}

    def run(key, n):
        eng.set_width_pruning(*settings[key])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            eng.estimate(inp, K_MATRIX, out=out)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n
    for key in settings:
        run(key, 5)
    ms = {k: [] for k in settings}
    order = list(settings)
    for r in range(reps):
        for key in order[r % 3:] + order[:r % 3]:
            ms[key].append(run(key, inner))
    res = {"pairs": B, "kpts": N}
    for key in settings:
        res[key] = {"step_ms": med(ms[key]), "spread_ms": spread(ms[key])}
    for key in ("neutral", "half"):
        res[key]["vs_off_pct"] = 100.0 * (res[key]["step_ms"] / res["off"]["step_ms"] - 1.0)
    # per-layer kept counts and what the settings return
    for key in settings:
        run(key, 1)
        torch.cuda.synchronize()
        res[key]["n_match_mean"] = float(out["n_match"].float().mean())
        res[key]["ok"] = int(out["ok"].sum())
        if key != "off":
            c = eng.debug_read("prune_counts", 2 * B * 9, dtype=np.int32).reshape(2 * B, 9)[:, :8]
            res[key]["kept_mean_after_layer"] = [float(x) for x in c.mean(axis=0)]
    res["half"]["min_kpts"], res["neutral"]["min_kpts"], res["width_confidence"] = HALF_MIN_KPTS, 2 * N, WC
    print(name, json.dumps(res), flush=True)
    del eng
    return res


def bench_child(tree, B, N, steps, dump):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "5", "--batch", str(B), "--kpts", str(N), "--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"bench.py in {tree} failed ({r.returncode}): {r.stderr[-800:]}")
    return json.loads(lines[-1])


def against_parent(parent, steps):
    res = {}
    for name, (B, N) in SHAPES.items():
        runs = {"this": [], "parent": []}
        equal = True
        with tempfile.TemporaryDirectory() as tmp:
            for r in range(2):
                for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                    d = os.path.join(tmp, f"{who}{r}")
                    line = bench_child(parent if who == "parent" else ROOT, B, N, steps, d)
                    runs[who].append(float(line["ms_per_step"]))
                    print(name, who, line["ms_per_step"], flush=True)
            ref = os.path.join(tmp, "parent0")
            names = sorted(os.listdir(ref))
            for who, r in (("this", 0), ("this", 1), ("parent", 1)):
                d = os.path.join(tmp, f"{who}{r}")
                equal &= sorted(os.listdir(d)) == names and all(np.array_equal(np.load(os.path.join(d, f)), np.load(os.path.join(ref, f))) for f in names)
        res[name] = {"this_ms_per_step": runs["this"], "parent_ms_per_step": runs["parent"], "order": "parent, this, this, parent",
                     "delta_pct": 100.0 * (med(runs["this"]) / med(runs["parent"]) - 1.0), "dumped_arrays": names, "dumps_equal": bool(equal)}
        print(name, json.dumps(res[name]), flush=True)
    return res


def main():
    args = list(sys.argv[1:])
    parent, steps = None, 30
    if "--parent-tree" in args:
        i = args.index("--parent-tree")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    if "--bench-steps" in args:
        i = args.index("--bench-steps")
        steps = int(args[i + 1])
        del args[i:i + 2]
    from gisnav_amd import _lib
    res = {"library_digest": _lib.library_digest(), "precision": PRECISION, "certify": "off", "steps": {k: measure(k) for k in SHAPES}}
    path = args[0] if args else os.path.join(ROOT, "profiles", "width_pruning.json")
    for part in range(2 if parent else 1):      # (written before the bench children start, and again with their part)
        if part == 1:
            res["off_against_parent_bench"] = against_parent(parent, steps)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()

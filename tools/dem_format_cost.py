"""Cost of the elevation-raster formats (DESIGN.md "Elevation rasters: element types, scale, offset, voids"): the 32-pair step (gn_estimate, two
sub-batch streams as the bench runs, 1024 keypoints per side, headline precision) and the gather stage alone, for

    u8            the default: a uint8 raster, nothing set (k_gather)
    u16, f32      the same heights re-encoded as uint16 / float32 under a scale and an offset (k_gather_dem<T>, the wide grid)
    u8_nodata     a uint8 raster with a void value that no cell holds (k_gather_dem_voids<uint8_t>: one workgroup per pair)
    i16_void10    an int16 raster with 10 % of the cells under the reference keypoints void

interleaved in one process and timed by HIP events; medians over alternating repetitions, the spread (90th - 10th percentile) of the default
printed next to every difference.  The gather stage is one gn_gather_points_scored call on the batch's own match list between two events, the
launch included (the list is restored from a copy before every call: the void settings shorten it in place).  With --parent DIR (a built
checkout of the parent commit) the unset path is also measured against the parent: `bench.py --gpus 1` in fresh alternating processes, both
trees, with the spread between the runs of one tree.  No threshold is applied here: the numbers go to profiles/dem_format.json.

    python tools/dem_format_cost.py [out.json] [--parent DIR]
"""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SUB, REPS = 32, 2, 12
SETTINGS = ("u8", "u16", "f32", "u8_nodata", "i16_void10")


def med(v):
    return float(np.median(v))


def spread(v):
    return float(np.percentile(v, 90) - np.percentile(v, 10))


def against_parent(parent, runs=3, steps=40, warmup=10):
    """bench.py in fresh processes, parent and this tree alternating; ms per step of every run, and whether the --dump-outputs arrays agree."""
    import tempfile
    ms = {"parent": [], "this": []}
    dumps = {name: tempfile.mkdtemp(prefix=f"dem_format_{name}_") for name in ms}
    for r in range(runs):
        for name, tree in ((("parent", parent), ("this", ROOT)) if r % 2 == 0 else (("this", ROOT), ("parent", parent))):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", dumps[name]],
                               cwd=tree, capture_output=True, text=True, timeout=600, check=True)
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            ms[name].append(1e3 * B / float(line["value"]) if "value" in line else float(line["ms_per_step"]))
    names = sorted(f for f in os.listdir(dumps["parent"]) if f.endswith(".npy"))
    same = {f[:-4]: bool(np.load(os.path.join(dumps["parent"], f)).tobytes() == np.load(os.path.join(dumps["this"], f)).tobytes()) for f in names}
    return dict(dump_outputs_bitwise_equal=same, runs_per_tree=runs, steps=steps, parent_ms=ms["parent"], this_ms=ms["this"], parent_median_ms=med(ms["parent"]), this_median_ms=med(ms["this"]),
                parent_run_to_run_ms=max(ms["parent"]) - min(ms["parent"]), this_run_to_run_ms=max(ms["this"]) - min(ms["this"]),
                delta_pct=100.0 * (med(ms["this"]) / med(ms["parent"]) - 1.0))


def main():
    import torch
    from gisnav_amd.engine import PoseEngine, _ptr
    from gisnav_amd.synthetic import K_MATRIX, make_pair
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    pairs = [make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)]

    def encoded(fn):
        return eng.stage_inputs([dataclasses.replace(p, dem=fn(p)) for p in pairs])

    def void10(p):
        d = (64 * p.dem.astype(np.int64) - 2000).astype(np.int16)
        h, w = d.shape
        yi = np.clip(np.floor(p.kp_r[:, 1]).astype(int), 0, h - 1)
        xi = np.clip(np.floor(p.kp_r[:, 0]).astype(int), 0, w - 1)
        pick = np.random.default_rng(5).random(len(yi)) < 0.10
        d[yi[pick], xi[pick]] = -32768
        return d

    # setting -> (inputs, (scale, offset, nodata))
    cfg = {"u8": (encoded(lambda p: p.dem), (1.0, 0.0, None)),
           "u16": (encoded(lambda p: (64 * p.dem.astype(np.int64) + 1000).astype(np.uint16)), (1.0 / 64, -15.625, None)),
           "f32": (encoded(lambda p: (p.dem.astype(np.float32) / np.float32(4) + np.float32(100.5))), (4.0, -402.0, None)),
           "u8_nodata": (encoded(lambda p: p.dem), (1.0, 0.0, 255)),
           "i16_void10": (encoded(void10), (1.0 / 64, 31.25, -32768))}
    eng.set_substreams(SUB)
    out = eng.alloc_outputs(B)

    def step(s):
        eng.set_dem_format(*cfg[s][1])
        eng.estimate(cfg[s][0], K_MATRIX, out=out)

    for s in SETTINGS * 2:
        for _ in range(5):
            step(s)
    eng.flush(); torch.cuda.synchronize()
    ms = {s: [] for s in SETTINGS}
    for rep in range(REPS):
        for s in (SETTINGS if rep % 2 == 0 else SETTINGS[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                step(s)
            eng.flush()
            e1.record(); e1.synchronize()
            ms[s].append(e0.elapsed_time(e1) / 10)
    dropped = None
    step("i16_void10"); eng.flush(); torch.cuda.synchronize()
    dropped = eng.dem_last_dropped(B)
    n_after = out["n_match"].cpu().numpy().copy()
    # the gather stage alone, on the batch's own match list
    eng.set_substreams(1)
    eng.set_dem_format()
    inp = cfg["u8"][0]
    idx0, score0, nm0 = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    idx, score, nm = idx0.clone(), score0.clone(), nm0.clone()
    mkp = torch.zeros((B, eng.kmax, 2), dtype=torch.float32, device=eng.device)
    obj = torch.zeros((B, eng.kmax, 3), dtype=torch.float32, device=eng.device)
    gm = {s: [] for s in SETTINGS}
    for rep in range(REPS):
        for s in (SETTINGS if rep % 2 == 0 else SETTINGS[::-1]):
            eng.set_dem_format(*cfg[s][1])
            dem = cfg[s][0]["dem"]
            eng._apply_dem_format(dem)
            t = []
            for _ in range(20):
                idx.copy_(idx0); score.copy_(score0); nm.copy_(nm0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = eng.lib.gn_gather_points_scored(eng.ctx, B, inp["kpt_format"], _ptr(inp["kpt_q"]), inp["kpt_q"].shape[1], _ptr(inp["kpt_r"]),
                                                     inp["kpt_r"].shape[1], _ptr(idx), _ptr(score), _ptr(nm), _ptr(dem), dem.shape[1], dem.shape[2],
                                                     _ptr(mkp), _ptr(obj), eng._stream())
                e1.record(); e1.synchronize()
                assert rc == 0, rc
                t.append(e0.elapsed_time(e1))
            gm[s].append(med(t[2:]))
    eng.set_dem_format()
    res = {"workload": f"{B} x 1024, f16x2_f16_attn, {SUB} sub-batch streams for the step, medians of {REPS} alternating repetitions; gather = one "
                       "gn_gather_points_scored call between two HIP events (launch included)",
           "matches_per_pair_median": float(np.median(nm0.cpu().numpy())), "i16_void10_dropped_per_pair_median": float(np.median(dropped)),
           "i16_void10_matches_left_median": float(np.median(n_after))}
    for s in SETTINGS:
        res[s] = dict(step_ms=med(ms[s]), step_spread_ms=spread(ms[s]), step_delta_pct=100.0 * (med(ms[s]) / med(ms["u8"]) - 1.0),
                      gather_ms=med(gm[s]), gather_spread_ms=spread(gm[s]), gather_delta_ms=med(gm[s]) - med(gm["u8"]))
    del eng
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--parent" in sys.argv:
        res["unset_against_parent"] = against_parent(os.path.abspath(sys.argv[sys.argv.index("--parent") + 1]))
        args = [a for a in args if os.path.abspath(a) != os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])]
    print(json.dumps(res, indent=1), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

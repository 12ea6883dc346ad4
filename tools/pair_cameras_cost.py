"""Cost of the per-pair camera table (DESIGN.md "Per-pair cameras"): the 32-pair step (gn_estimate, two sub-batch streams as the bench runs, 1024
keypoints per side, headline precision) with the camera by value and with a table of 32 identical rows, for model 0 (pinhole) and model 1
(plumb-bob), the four settings interleaved in one process and timed by HIP events; the PnP stage alone on the same batch's correspondences, the
same four settings; and what the table replaces: two cameras x 16 pairs as TWO calls of 16 pairs (one per camera, gn_set_distortion in between)
against ONE 32-pair call with a table.  Medians over alternating repetitions; the spread (90th - 10th percentile) of the by-value path is printed
next to every difference.  No threshold is applied here: the numbers go to profiles/pair_cameras.json.

    python tools/pair_cameras_cost.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = (-0.05, 0.002, 5e-4, -3e-4, 0.0)
B, SUB, REPS = 32, 2, 16
SETTINGS = (("value", 0), ("table", 0), ("value", 1), ("table", 1))      # (camera source, model)


def med(v):
    return float(np.median(v))


def spread(v):
    return float(np.percentile(v, 90) - np.percentile(v, 10))


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    import torch
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import K_MATRIX, make_pair
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    inp = eng.stage_inputs([make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)])
    eng.set_substreams(SUB)
    out = eng.alloc_outputs(B)
    Ks = np.repeat(K_MATRIX[None], B, axis=0)
    tables = {0: eng.pair_cameras(Ks), 1: eng.pair_cameras(Ks, np.repeat(np.array(D)[None], B, axis=0))}
    with_table = {m: dict(inp, cameras=tables[m][0], camera_model=tables[m][1]) for m in (0, 1)}

    def step(src, model):
        eng.set_distortion(D if (src == "value" and model) else None)
        if src == "value":
            eng.estimate(inp, K_MATRIX, out=out)
        else:
            eng.estimate(with_table[model], None, out=out)

    for s in SETTINGS * 2:
        for _ in range(5):
            step(*s)
    eng.flush(); torch.cuda.synchronize()
    ms = {s: [] for s in SETTINGS}
    for rep in range(REPS):
        for s in (SETTINGS if rep % 2 == 0 else SETTINGS[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                step(*s)
            eng.flush()
            e1.record(); e1.synchronize()
            ms[s].append(e0.elapsed_time(e1) / 10)
    # the PnP stage alone on the staged points of this batch
    eng.set_distortion(None)
    idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])

    def pnp(src, model):
        eng.set_distortion(D if (src == "value" and model) else None)
        if src == "value":
            eng.pnp_ransac(obj, mkp, nm, K_MATRIX, min_pts=15)
        else:
            eng.pnp_ransac(obj, mkp, nm, None, min_pts=15, cameras=tables[model][0], camera_model=model)

    pm = {s: [] for s in SETTINGS}
    for rep in range(REPS):
        for s in (SETTINGS if rep % 2 == 0 else SETTINGS[::-1]):
            pm[s].append(timed(lambda: pnp(*s), 20))
    # what the table replaces: two cameras x 16 pairs.  Two calls of 16 pairs, one per camera (the second with its own coefficients), against one
    # call of 32 with a table whose halves differ
    K2 = K_MATRIX * np.array([[1.5, 1, 1], [1, 1.5, 1], [1, 1, 1]])
    D2 = (-0.11, 0.03, -4e-4, 6e-4, -0.004)
    half = [{k: (v[h * 16:(h + 1) * 16] if isinstance(v, torch.Tensor) else v) for k, v in inp.items()} for h in (0, 1)]
    outs = [{k: v[h * 16:(h + 1) * 16] for k, v in out.items()} for h in (0, 1)]
    two = eng.pair_cameras(np.concatenate([Ks[:16], np.repeat(K2[None], 16, axis=0)]),
                           np.concatenate([np.repeat(np.array(D)[None], 16, axis=0), np.repeat(np.array(D2)[None], 16, axis=0)]))
    two_inp = dict(inp, cameras=two[0], camera_model=two[1])

    def two_calls():
        eng.set_distortion(D)
        eng.estimate(half[0], K_MATRIX, out=outs[0])
        eng.set_distortion(D2)
        eng.estimate(half[1], K2, out=outs[1])

    def one_call():
        eng.set_distortion(None)
        eng.estimate(two_inp, None, out=out)

    alt = {"two_calls": [], "one_table_call": []}
    for f in (two_calls, one_call) * 2:
        for _ in range(5):
            f()
    eng.flush(); torch.cuda.synchronize()
    for rep in range(REPS):
        for name, f in ((("two_calls", two_calls), ("one_table_call", one_call)) if rep % 2 == 0 else (("one_table_call", one_call), ("two_calls", two_calls))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                f()
            eng.flush()
            e1.record(); e1.synchronize()
            alt[name].append(e0.elapsed_time(e1) / 10)
    eng.set_distortion(None)
    res = {"workload": f"{B} x 1024, f16x2_f16_attn, {SUB} sub-batch streams, medians of {REPS} alternating repetitions"}
    for model in (0, 1):
        v, t = ("value", model), ("table", model)
        res[f"model{model}"] = dict(
            step_value_ms=med(ms[v]), step_value_spread_ms=spread(ms[v]), step_table_ms=med(ms[t]), step_delta_pct=100.0 * (med(ms[t]) / med(ms[v]) - 1.0),
            pnp_value_ms=med(pm[v]), pnp_value_spread_ms=spread(pm[v]), pnp_table_ms=med(pm[t]), pnp_delta_pct=100.0 * (med(pm[t]) / med(pm[v]) - 1.0))
    res["two_cameras_x_16_pairs"] = dict(two_calls_ms=med(alt["two_calls"]), two_calls_spread_ms=spread(alt["two_calls"]),
                                         one_table_call_ms=med(alt["one_table_call"]), one_table_call_spread_ms=spread(alt["one_table_call"]),
                                         table_against_two_calls_pct=100.0 * (med(alt["one_table_call"]) / med(alt["two_calls"]) - 1.0))
    eng.set_substreams(1)
    del eng
    print(json.dumps(res, indent=1), flush=True)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

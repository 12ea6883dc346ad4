#!/usr/bin/env python3
"""What LoFTR's certificate costs on the clock (needs an MI355X).

Workload: 640x480 seeded synthetic pairs (gisnav_amd.loftr_synthetic), fine level on, B = 1 and B = 8, one batched call per measurement, in five
configurations: exact f32; split fp16; split with flags (mode 1); split with re-run and nothing flagged (mode 2, the calibrated eps -- the tool
stops if that flags a pair of this workload); split with re-run and every pair flagged (eps forced to 0.9: the whole batch runs twice).  Every
configuration is warmed up (graph capture included), then they alternate in windows of at least `--window` seconds, each closed by a device
synchronisation; figures are pairs/s and ms per pair over all rounds, and per round for the spread.  Output: --out (profiles/loftr_certify.json).

`--only split` times the split configuration alone and needs nothing of the certificate: the form in which a build without it can be run beside
this one (alternate the two processes on one lease and compare their `split` lines; the spread of one build against itself comes first).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GISNAV_AMD_TREE", ROOT))       # (GISNAV_AMD_TREE: time another checkout's library with this file)

from gisnav_amd import loftr_synthetic as olf  # noqa: E402
from gisnav_amd.loftr import LoFTR  # noqa: E402

H, W = 480, 640


def window(fn, seconds):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of configurations (default: all five)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_certify.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = olf.synthetic_state_dict(0)
    batches = [int(b) for b in args.batches.split(",")]
    bmax = max(batches)
    pairs = [olf.synthetic_pair(1 + i, H, W) for i in range(bmax)]
    i0 = torch.stack([p[0] for p in pairs])[:, None].to(dev)
    i1 = torch.stack([p[1] for p in pairs])[:, None].to(dev)
    configs = {"exact_f32": dict(arithmetic="exact_f32"), "split": dict(arithmetic="split_fp16"), "split_flags": dict(arithmetic="split_fp16", certify="flags"),
               "split_rerun_none_flagged": dict(arithmetic="split_fp16", certify="rerun"), "split_rerun_all_flagged": dict(arithmetic="split_fp16", certify="rerun", certify_eps=0.9)}
    if args.only:
        configs = {k: configs[k] for k in args.only.split(",")}
    ms = {}
    cal = None
    for k, kw in configs.items():
        ms[k] = LoFTR(state_dict=sd, **kw).to(dev).eval()
        ms[k]._ensure(H, W, bmax)
        if "certify" in kw and "certify_eps" not in kw:
            cal = ms[k].calibrate_certify(i0, i1)
    rows = []
    for B in batches:
        a, b = i0[:B], i1[:B]
        forms = {k: (lambda m=m: m.match_segments(a, b)) for k, m in ms.items()}
        for k, fn in forms.items():
            seg = fn(); fn()
            flags = seg.get("uncertain")
            if (k == "split_rerun_all_flagged" and not bool(flags.all())) or (k == "split_rerun_none_flagged" and bool(flags.any())):
                raise SystemExit(f"{k} B={B}: flagged {flags.tolist()}, which is not the configuration to be timed")
        acc = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                acc[k].append(window(fn, args.window))
        row = {"B": B, "H": H, "W": W, "fine": True, "label": args.label}
        for k, ws in acc.items():
            n, dt = sum(w[0] for w in ws), sum(w[1] for w in ws)
            row[k] = {"pairs_per_s": round(n * B / dt, 2), "ms_per_pair": round(dt / (n * B) * 1e3, 4), "ms_per_pair_rounds": [round(w[1] / (w[0] * B) * 1e3, 4) for w in ws]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    stats = {k: m.certify_stats() for k, m in ms.items() if hasattr(m, "certify_stats")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_loftr_certify.py", "window_s": args.window, "rounds": args.rounds, "label": args.label, "calibration": cal, "certify_stats": stats, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batched LoFTR against back-to-back single-pair calls (needs an MI355X).

Workload: 640x480 seeded synthetic pairs (gisnav_amd.loftr_synthetic), both arithmetics, fine level on, B in {1, 2, 4, 8}.  Figure: pairs/s of ONE
batched call (`LoFTR` on a (B, 1, H, W) input -> gn_loftr_match_batch) against B single-pair calls on the same build, in one process: every shape
is warmed up first (graph capture included), then the two forms alternate in windows of at least `--window` seconds, each ending in a device
synchronisation.  In exact-f32 arithmetic the call that leaves the counts on the device (`match_segments(host_counts=False)`, no stream
synchronisation inside the call) is timed as a third form.  A digest of every pair's outputs is printed for the batched and the sequential form:
they must be equal (a pair's bits do not depend on the batch).  Output: profiles/loftr_batch.json.

`--trace-only B` runs a few calls of one shape and nothing else: the process to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gisnav_amd import loftr_synthetic as olf  # noqa: E402
from gisnav_amd.loftr import LoFTR  # noqa: E402

H, W = 480, 640


def digest(k0, k1, conf):
    h = hashlib.sha256()
    for t in (k0, k1, conf):
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def window(fn, seconds):
    """Calls of fn() for at least `seconds`, the window closed by a synchronise; returns (calls, elapsed)."""
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
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_batch.json"))
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--arithmetic", default="exact_f32,split_fp16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = olf.synthetic_state_dict(0)
    batches = [int(b) for b in args.batches.split(",")]
    bmax = max(batches + [args.trace_only])
    pairs = [olf.synthetic_pair(1 + i, H, W) for i in range(bmax)]
    i0 = torch.stack([p[0] for p in pairs])[:, None].to(dev)
    i1 = torch.stack([p[1] for p in pairs])[:, None].to(dev)
    if args.trace_only:
        B = args.trace_only
        m = LoFTR(state_dict=sd, arithmetic=args.arithmetic.split(",")[0]).to(dev).eval()
        for _ in range(6):
            m({"image0": i0[:B], "image1": i1[:B]})
        torch.cuda.synchronize()
        return
    results = []
    for arith in args.arithmetic.split(","):
        single = LoFTR(state_dict=sd, arithmetic=arith).to(dev).eval()
        batched = LoFTR(state_dict=sd, arithmetic=arith).to(dev).eval()
        batched._ensure(H, W, bmax)
        seq_out = [single({"image0": i0[b], "image1": i1[b]}) for b in range(bmax)]        # warm-up of the single-pair shape, and the digests
        seq_dig = [digest(o["keypoints0"], o["keypoints1"], o["confidence"]) for o in seq_out]
        for B in batches:
            data = {"image0": i0[:B], "image1": i1[:B]}
            out = batched(data)                                                              # warm-up (captures the (arithmetic, B) graph)
            bi = out["batch_indexes"]
            bat_dig = [digest(out["keypoints0"][bi == b], out["keypoints1"][bi == b], out["confidence"][bi == b]) for b in range(B)]
            print(f"digest {arith} B={B} batched    {' '.join(bat_dig)}")
            print(f"digest {arith} B={B} sequential {' '.join(seq_dig[:B])}")
            if bat_dig != seq_dig[:B]:
                raise SystemExit("a pair's outputs differ between the batched and the sequential form")
            forms = {"batched": lambda: batched(data),
                     "sequential": lambda: [single({"image0": i0[b], "image1": i1[b]}) for b in range(B)]}
            if arith == "exact_f32":
                forms["batched_no_sync"] = lambda: batched.match_segments(data["image0"], data["image1"], host_counts=False)
            for fn in forms.values():
                fn()
            acc = {k: [0, 0.0] for k in forms}
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    n, dt = window(fn, args.window)
                    acc[k][0] += n; acc[k][1] += dt
            row = {"arithmetic": arith, "B": B, "H": H, "W": W, "fine": True, "matches": [int((bi == b).sum()) for b in range(B)]}
            for k, (n, dt) in acc.items():
                row[f"{k}_pairs_per_s"] = round(n * B / dt, 2)
                row[f"{k}_ms_per_pair"] = round(dt / (n * B) * 1e3, 3)
            row["batched_over_sequential"] = round(row["batched_pairs_per_s"] / row["sequential_pairs_per_s"], 3)
            print(json.dumps(row), flush=True)
            results.append(row)
        del single, batched
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_loftr_batch.py", "window_s": args.window, "rounds": args.rounds, "rows": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Does LoFTR's certificate ever vouch for a pair whose split-fp16 coarse (i, j) list differs from exact f32's?  (needs an MI355X)

For every setting -- image size, `noise` and `shift` of the synthetic pairs, `mlp_out_gain` of the synthetic weights (1.0 = low-margin: every
transformer layer replaces the stream instead of perturbing it) -- eps is calibrated on the first pairs (`LoFTR.calibrate_certify`, safety 4)
and `--pairs` seeded pairs are matched in batches by an exact-f32 matcher and by a split-fp16 matcher with `certify="flags"`.  Per setting:
the index mismatches between the two (symmetric difference of the (i, j) sets), how many of them sit in flagged pairs -- which must be ALL
of them --, and the flagged fraction.  Prints one JSON line per setting and a verdict line; writes profiles/loftr_certify_sweep.json.

    python tools/loftr_certify_sweep.py [--pairs 12] [--batch 6] [--quick]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gisnav_amd import loftr_synthetic as olf  # noqa: E402
from gisnav_amd.loftr import LoFTR  # noqa: E402

SIZES = [(128, 160), (136, 200), (240, 320)]
NOISES = [0.01, 0.1, 0.2]
SHIFTS = [(16, 8), (24, 16), (20, 12)]          # (20, 12): no multiple of 8, the coarse cells do not correspond exactly
GAINS = [0.25, 1.0]


def ids(seg, b):
    n = seg["n_host"][b]
    return {(int(i), int(j)) for i, j in seg["ij"][b, :n].cpu().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="one size, two noises, one shift")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_certify_sweep.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes, noises, shifts = (SIZES[:1], NOISES[:2], SHIFTS[:1]) if args.quick else (SIZES, NOISES, SHIFTS)
    rows, t0 = [], time.time()
    for gain in GAINS:
        sd = olf.synthetic_state_dict(0, mlp_out_gain=gain)
        for (h, w) in sizes:
            exact = LoFTR(state_dict=sd, arithmetic="exact_f32", fine=False).to(dev).eval()
            split = LoFTR(state_dict=sd, arithmetic="split_fp16", fine=False, certify="flags").to(dev).eval()
            for noise in noises:
                for shift in shifts:
                    row = {"H": h, "W": w, "noise": noise, "shift": list(shift), "mlp_out_gain": gain, "pairs": 0, "matches_f32": 0, "mismatches": 0,
                           "mismatches_in_flagged_pairs": 0, "pairs_with_mismatch": 0, "flagged": 0}
                    for s0 in range(0, args.pairs, args.batch):
                        seeds = range(1 + s0, 1 + min(args.pairs, s0 + args.batch))
                        ps = [olf.synthetic_pair(s, h, w, shift=shift, noise=noise) for s in seeds]
                        i0 = torch.stack([p[0] for p in ps])[:, None].to(dev); i1 = torch.stack([p[1] for p in ps])[:, None].to(dev)
                        if s0 == 0:
                            row.update({k: v for k, v in split.calibrate_certify(i0, i1).items()})
                        a, b = exact.match_segments(i0, i1), split.match_segments(i0, i1)
                        for k in range(len(ps)):
                            d = len(ids(a, k) ^ ids(b, k))
                            flag = bool(b["uncertain"][k])
                            row["pairs"] += 1; row["matches_f32"] += a["n_host"][k]; row["mismatches"] += d; row["pairs_with_mismatch"] += d > 0
                            row["flagged"] += flag; row["mismatches_in_flagged_pairs"] += d if flag else 0
                    row["flagged_fraction"] = round(row["flagged"] / row["pairs"], 3)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del exact, split
    tot = {k: sum(r[k] for r in rows) for k in ("pairs", "matches_f32", "mismatches", "mismatches_in_flagged_pairs", "pairs_with_mismatch", "flagged")}
    ok = tot["mismatches"] == tot["mismatches_in_flagged_pairs"]
    tot["seconds"] = round(time.time() - t0, 1)
    print(("VERDICT: every index mismatch sits in a flagged pair " if ok else "VERDICT: THE CERTIFICATE VOUCHED FOR A WRONG PAIR ") + json.dumps(tot))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/loftr_certify_sweep.py", "totals": tot, "sound": ok, "rows": rows}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

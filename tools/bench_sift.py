#!/usr/bin/env python
"""Measurement of SIFT extraction on one MI355X next to the oracle on the host.  One JSON line.
    python tools/bench_sift.py [--steps 20] [--size 480 640] [--batch B] [--nOctaveLayers 3 --contrastThreshold 0.04 --edgeThreshold 10 --sigma 1.6]
                               [--general-blur]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from gisnav_amd.sift import SIFT  # noqa: E402
from test_sift import blob_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--max-kp", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=1, help="images per call (gn_sift_detect_and_compute_batch)")
    ap.add_argument("--nOctaveLayers", type=int, default=3)
    ap.add_argument("--contrastThreshold", type=float, default=0.04)
    ap.add_argument("--edgeThreshold", type=float, default=10.0)
    ap.add_argument("--sigma", type=float, default=1.6)
    ap.add_argument("--general-blur", action="store_true", help="developer switch: every pyramid level through the two-launch blur (gn_debug_set_variant 50)")
    ap.add_argument("--no-oracle", action="store_true", help="skip the host oracle (cpu_baseline is null)")
    args = ap.parse_args()
    H, W = args.size
    img = blob_image(11, H, W, n=900)
    params = dict(nOctaveLayers=args.nOctaveLayers, contrastThreshold=args.contrastThreshold, edgeThreshold=args.edgeThreshold, sigma=args.sigma)
    sift = SIFT(max_keypoints=args.max_kp, **params)
    if args.general_blur:
        assert sift._eng.lib.gn_debug_set_variant(sift._eng.ctx, 50, 1) == 0
    B = args.batch
    if B > 1:
        imgs = np.stack([blob_image(11 + b, H, W, n=900) for b in range(B)])
        imgs[0] = img
        t = torch.as_tensor(imgs, device=sift._eng.device)
        call = lambda: sift.detect_and_compute_batch_device(t)
    else:
        t = torch.as_tensor(img, device=sift._eng.device)
        call = lambda: sift.detect_and_compute_device(t)
    for _ in range(args.warmup):
        out = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3 / B          # per image
    n_kp = int(out[4][0]) if B > 1 else int(out[0].shape[0])
    okp, cpu_s = None, None
    if not args.no_oracle:
        from oracle import sift as osift
        t1 = time.perf_counter()
        pyr = osift.build_pyramids(img, args.nOctaveLayers, args.sigma)
        okp = osift.sort_and_dedup(osift.detect(img, args.nOctaveLayers, args.contrastThreshold, args.edgeThreshold, args.sigma, pyramids=pyr))
        osift.compute(pyr[0], okp)
        cpu_s = time.perf_counter() - t1
    # scale space: every level of the doubled pyramid is read once and written once (+ its DoG level) by the fused blur
    px = sum((2 * H >> o) * (2 * W >> o) for o in range(12) if min(2 * H >> o, 2 * W >> o) >= 1)
    n_g = args.nOctaveLayers + 3
    alg_bytes = px * 4 * (n_g * 2 + n_g - 1)          # nOctaveLayers + 3 levels x (read + write) + nOctaveLayers + 2 DoG levels x 1 write
    default = (args.nOctaveLayers, args.contrastThreshold, args.edgeThreshold, args.sigma) == (3, 0.04, 10.0, 1.6)
    line = {"metric": "SIFT detectAndCompute images/sec (" + ("cv2.SIFT_create() defaults" if default else "cv2.SIFT_create(%d, %g, %g, %g)" % (
                args.nOctaveLayers, args.contrastThreshold, args.edgeThreshold, args.sigma)) + (", two-launch blur" if args.general_blur else "") + ")", "value": round(1e3 / ms, 1), "unit": "images/s", "n_gpus": 1,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms * B, 3), "ms_per_image": round(ms, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (no FMA contraction; bit-identical to the oracle)", "data": "synthetic",
            "config": {"workload": f"{H}x{W} u8 image, {n_kp} keypoints (oracle: {None if okp is None else len(okp)})", "images_per_call": B, **params,
                       "general_blur": bool(args.general_blur)},
            "roofline": {"kernel": "whole call: k_blur_fused x21 + k_sift_tail + k_sift_find + k_sift_refine + k_sift_rank + k_sift_descriptor", "bound": "hbm",
                         "achieved": round(alg_bytes / (ms * 1e-3) / 1e9, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(alg_bytes / (ms * 1e-3) / 1e9 / 8000.0, 5),
                         "traffic": None, "note": "fully stream-ordered (one host sync at the end to read the keypoint count); ~31 dependent launches, each >= 4-5 us "
                                                  "of dispatch latency at this image size, so the call is latency- not bandwidth-bound (see DESIGN.md 7)"},
            "cpu_baseline": None if cpu_s is None else {"value": round(1.0 / cpu_s, 3), "unit": "images/s", "cores": 1, "kind": "port",
                             "sample": f"1 image; numpy restatement of cv2.SIFT (oracle/sift.py); cpu={platform.processor() or platform.machine()}"}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

"""Golden fixture for iterations_count above 16 in the PnP stage (tests/test_gpu_ransac_iterations.py, tests/test_ransac_iterations_host.py):
scenes with gross outliers and, for each listed count, what the repo's own restatements of cv2.solvePnPRansac return --
oracle/pnp_ransac.py::solve_pnp_ransac for the pinhole scenes, tests/pnp_distorted_ref.py::solve_pnp_ransac_dist for the distorted one --
together with the final adapted iteration count.  The oracle costs milliseconds per hypothesis, so the GPU tests read this file instead.

    python tests/golden/make_ransac_iters_golden.py

`scene` restates tests/sweeps/fuzz_pnp.py::scene (that module runs on import).  The counts hold ROUND - 1, ROUND, ROUND + 1 and 2 ROUND + 1 for
the round size of the kernels (kRansacRound = 64).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gisnav_amd.synthetic import K_MATRIX, make_pair  # noqa: E402
from oracle import pnp_ransac as pr  # noqa: E402
import pnp_distorted_ref as pdr  # noqa: E402

ROUND = 64
OUT = os.path.join(HERE, "pnp_ransac_iters.npz")

# name: (seed, n, outlier fraction, flat DEM)
SCENES = {"A": (100, 60, 0.5, False), "B": (102, 300, 0.6, False), "C": (100, 200, 0.8, False), "D": (101, 60, 0.5, False),
          "E": (103, 120, 0.7, True), "clean": (36, 200, 0.0, False)}
SCENES.update({f"P{i}": (200 + i, 60, 0.5, False) for i in range(8)})
COUNTS = {"A": (10, 16, 17, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1, 144, 145, 146, 300, 4096),
          "B": (16, 17, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND, 2 * ROUND + 1, 300, 1000),
          "C": (10, 17, ROUND, 300), "D": (10, ROUND), "E": (10, 17, ROUND, 300), "clean": (4096,)}
COUNTS.update({f"P{i}": (10, 100, 300) for i in range(8)})
DIST_SCENE = (120, 7, False)      # pnp_distorted_ref.make_scene(n, seed, planar), then half of the image points replaced
DIST_COUNTS = (10, 100)


def scene(seed, n, outliers=0.0, flat=False):
    rng = np.random.default_rng(seed)
    p = make_pair(9000 + seed, n_q=max(n, 64), n_r=max(4 * n, 256), flat_dem=flat)
    m = np.nonzero(p.gt_q2r >= 0)[0][:n]
    q = p.kp_q[m].astype(np.float32).copy()
    r = p.kp_r[p.gt_q2r[m]].astype(np.float32).copy()
    k = int(outliers * len(q))
    if k:
        q[rng.permutation(len(q))[:k]] = rng.uniform(0, 480, (k, 2)).astype(np.float32)
    x, y = np.transpose(np.floor(r).astype(int))
    z = np.zeros(len(r)) if flat else p.dem[y, x]
    return np.hstack((r, z.reshape(-1, 1))).astype(np.float32), q


def dist_scene():
    n, seed, planar = DIST_SCENE
    obj, img, _, _, _ = pdr.make_scene(n, seed, planar)
    rng = np.random.default_rng(1000 + seed)
    k = n // 2
    img = img.copy()
    img[rng.permutation(n)[:k]] = rng.uniform((0, 0), (640, 480), (k, 2)).astype(np.float32)
    return obj, img


def run(solver, module, count):
    """(ok, n_inliers, R, t, final adapted niters, inlier indices) of one restated solvePnPRansac call; niters is what RANSACUpdateNumIters
    last returned (the requested count when it was never called)."""
    orig = module.ransac_update_num_iters
    log = []

    def wrap(p, ep, mp, mi):
        v = orig(p, ep, mp, mi)
        log.append(v)
        return v
    module.ransac_update_num_iters = wrap
    try:
        ok, r, t, inl = solver(count)
    finally:
        module.ransac_update_num_iters = orig
    niters = log[-1] if log else count
    if not ok:
        return 0, 0, np.eye(3), np.zeros(3), niters, np.zeros(0, int)
    return 1, len(inl), pr.rodrigues_vec2mat(r), np.asarray(t, np.float64).reshape(3), niters, np.asarray(inl).reshape(-1)


def main():
    out = {"round": np.int32(ROUND), "K": np.asarray(K_MATRIX, np.float64), "dist_K": pdr.K_TEST, "dist_d": pdr.D_TEST}
    jobs = []
    for name, (seed, n, fr, flat) in SCENES.items():
        obj, img = scene(seed, n, fr, flat)
        out[f"{name}_obj"], out[f"{name}_img"] = obj, img
        jobs.append((name, COUNTS[name], pr, lambda c, obj=obj, img=img: pr.solve_pnp_ransac(obj, img, K_MATRIX, c)))
    obj, img = dist_scene()
    out["dist_obj"], out["dist_img"] = obj, img
    uses = pdr if hasattr(pdr, "ransac_update_num_iters") else pr
    jobs.append(("dist", DIST_COUNTS, uses, lambda c, obj=obj, img=img: pdr.solve_pnp_ransac_dist(obj, img, pdr.K_TEST, pdr.D_TEST, c)))
    for name, counts, module, solver in jobs:
        rows = [run(solver, module, c) for c in counts]
        out[f"{name}_counts"] = np.asarray(counts, np.int32)
        out[f"{name}_ok"] = np.asarray([r[0] for r in rows], np.uint8)
        out[f"{name}_ninl"] = np.asarray([r[1] for r in rows], np.int32)
        out[f"{name}_R"] = np.stack([r[2] for r in rows])
        out[f"{name}_t"] = np.stack([r[3] for r in rows])
        out[f"{name}_niters"] = np.asarray([r[4] for r in rows], np.int32)
        mask = np.zeros((len(rows), len(out[f"{name}_obj"])), np.uint8)      # the winner's inlier set per row
        for i, r in enumerate(rows):
            mask[i, r[5]] = 1
        out[f"{name}_inl"] = mask
        print(name, [(int(c), int(r[0]), int(r[1]), int(r[4])) for c, r in zip(counts, rows)], flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""The fixed scenes of the pose-stage report tests (tests/test_pnp_report_host.py, tests/test_gpu_pnp_report.py) -- a test helper, not a test.

Every scene is listed here as a constant.  The host test asserts from the oracle alone that each scene's inlier set is STABLE: the restated
solvePnPRansac returns the same set at reproj_error = 8 (1 - 1e-3), 8 and 8 (1 + 1e-3), so no point sits close enough to the threshold for the
GPU's f32 scoring and the oracle's to disagree about it.  That is a condition on the inputs, checked when a scene is chosen; a scene that fails
it is replaced in these lists, never skipped at run time.
"""
import os

import numpy as np

import pnp_distorted_ref as ref

K, D = ref.K_TEST, ref.D_TEST
REPROJ = 8.0
MIN_PTS = 15

# 1. one call, pinhole: (n, seed, planar) of pnp_distorted_ref.make_scene with d = 0 (every fourth point displaced by 40-120 px).  The 4- and
#    5-point pairs are the first 4 / 5 inliers of their scene (as tests/test_gpu_pnp_distortion.py cuts them): solvePnPRansac's branches without
#    a RANSAC loop.  12 points stay below MIN_PTS.  63, 65, 130, 300: no multiple of 64, on both sides of one chunk, 300 past 256.
ONE_CALL = ((4, (24, 1, False)), (5, (24, 1, True)), (12, (12, 5, True)), (63, (63, 11, True)), (65, (65, 12, False)), (130, (130, 13, True)),
            (300, (300, 14, False)))
KSTRIDE = 384

# 2. round path: two 60-point scenes of tests/golden/pnp_ransac_iters.npz at iterations_count = 300
ROUND_SCENES = ("A", "P1")
ROUND_COUNT = 300
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_ransac_iters.npz")

# 3. distortion on: three of pnp_distorted_ref's scenes under D_TEST
DIST_SCENES = ((24, 2, False), (64, 3, True), (64, 4, False))


def one_call_scenes():
    """[(obj (n,3) f32, img (n,2) f32)] of ONE_CALL."""
    out = []
    for n, (m, seed, planar) in ONE_CALL:
        o, u, _, _, inl = ref.make_scene(m, seed, planar, K, np.zeros(5))
        out.append((o[inl][:n], u[inl][:n]) if n < m else (o, u))
    assert [len(o) for o, _ in out] == [n for n, _ in ONE_CALL]
    return out


def round_scenes():
    g = np.load(GOLDEN)
    return [(g[f"{s}_obj"], g[f"{s}_img"]) for s in ROUND_SCENES], g["K"]


def dist_scenes():
    return [ref.make_scene(n, seed, planar)[:2] for n, seed, planar in DIST_SCENES]

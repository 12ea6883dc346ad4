"""The five cameras and five scenes of the per-pair camera tests (gn_set_pair_cameras; DESIGN.md "Per-pair cameras") -- a test helper, not a test.

Scene b is tests/pnp_distorted_ref.make_scene(points[b], seed = 1 + b, planar for even b) seen through camera b.  The cameras differ enough
that a scene solved with its neighbour's camera either finds no model or misses t by more than 10 (tests/test_pair_cameras_host.py
re-asserts it): a table row that reaches the wrong pair cannot pass a test built on them.
"""
from __future__ import annotations

import functools

import numpy as np

import pnp_distorted_ref as ref
from oracle import pnp_ransac as pr


def k_matrix(fx, fy, cx, cy) -> np.ndarray:
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# (fx, fy, cx, cy), (k1, k2, p1, p2, k3), points
_CAMERAS = (
    ((ref.K_TEST[0, 0], ref.K_TEST[1, 1], ref.K_TEST[0, 2], ref.K_TEST[1, 2]), tuple(ref.D_TEST), 16),
    ((410.9392, 395.0, 331.5, 236.0), (-0.11, 0.03, -4e-4, 6e-4, -0.004), 24),
    ((300.0, 310.0, 300.0, 250.0), (0.0, 0.0, 0.0, 0.0, 0.0), 64),
    ((205.4696, 205.4696, 320.0, 180.0), (0.04, -0.003, 2e-4, 1e-4, 0.0), 24),      # the reference's 640 x 360 camera
    ((520.0, 515.0, 640.0, 360.0), (-0.2, 0.05, 0.0, 0.0, 0.0), 64),
)
NB = len(_CAMERAS)
KS = np.stack([k_matrix(*c[0]) for c in _CAMERAS])            # (5, 3, 3)
DS = np.array([c[1] for c in _CAMERAS], np.float64)          # (5, 5)
POINTS = tuple(c[2] for c in _CAMERAS)
TRUE_INLIERS = (12, 18, 48, 18, 48)


def table_rows(Ks=KS, Ds=DS) -> np.ndarray:
    """(B, 9) f64: fx, fy, cx, cy, k1, k2, p1, p2, k3 -- written out here, independently of PoseEngine.pair_cameras"""
    Ks, Ds = np.asarray(Ks, np.float64), np.asarray(Ds, np.float64)
    return np.column_stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2], Ds])


@functools.lru_cache(maxsize=None)
def scenes():
    """[(obj (n, 3) f32, img (n, 2) f32, rvec, tvec, inlier mask)] for b = 0 .. 4, each through its own camera"""
    return tuple(ref.make_scene(POINTS[b], 1 + b, b % 2 == 0, KS[b], DS[b]) for b in range(NB))


@functools.lru_cache(maxsize=None)
def restated(b: int, cam: int):
    """scene b solved by the fp64 restatement with camera `cam`: (ok, rvec (3,1), tvec (3,1), inliers)"""
    o, u, *_ = scenes()[b]
    return ref.solve_pnp_ransac_dist(o, u, KS[cam], DS[cam])


def half_displaced(b: int):
    """scene b with every second point displaced as make_scene displaces its outliers (40-120 px): 50 % outliers, for iteration counts > 16"""
    o, u, rv, tv, _ = scenes()[b]
    n = len(o)
    rng = np.random.default_rng(100 + b)
    img = ref.project_points_dist(o.astype(np.float64), rv, tv, KS[b], DS[b])
    out = np.arange(1, n, 2)
    ang, mag = rng.uniform(0, 2 * np.pi, len(out)), rng.uniform(40, 120, len(out))
    img[out] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
    inl = np.ones(n, bool)
    inl[out] = False
    return o, img.astype(np.float32), rv, tv, inl


def pose_error(R, t, w_r, w_t):
    """(|dR|_F, |dt| / |t|) of a returned (R (3,3), t) against the restatement's (rvec, tvec)"""
    w_t = np.asarray(w_t, np.float64).reshape(3)
    return (float(np.linalg.norm(np.asarray(R).reshape(3, 3) - pr.rodrigues_vec2mat(np.asarray(w_r).reshape(3)))),
            float(np.linalg.norm(np.asarray(t).reshape(3) - w_t) / np.linalg.norm(w_t)))

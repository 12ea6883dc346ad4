"""Scenes of the elevation-raster tests (tests/test_dem_format_host.py, tests/test_gpu_dem_format.py).  numpy and the synthetic scenes only: no GPU."""
from __future__ import annotations

import dataclasses

import numpy as np

from gisnav_amd.synthetic import K_MATRIX, make_pair

import dem_format_ref as ref

# One uint8 DEM d, re-encoded so that the lift returns d exactly: (dtype, encode(d), scale, offset)
ENCODINGS = {
    "uint16": (lambda d: (64 * d.astype(np.int64) + 1000).astype(np.uint16), 1.0 / 64, -15.625),
    "int16": (lambda d: (64 * d.astype(np.int64) - 2000).astype(np.int16), 1.0 / 64, 31.25),
    "float32": (lambda d: (d.astype(np.float32) / np.float32(4) + np.float32(100.5)).astype(np.float32), 4.0, -402.0),
}


def reencode(pair, name: str):
    """(pair with its uint8 DEM re-encoded as `name`, scale, offset); the lift of the new raster is the uint8 raster, cell for cell."""
    enc, scale, offset = ENCODINGS[name]
    dem = enc(pair.dem)
    assert np.array_equal(ref.lift(dem, scale, offset), pair.dem.astype(np.float32))
    return dataclasses.replace(pair, dem=dem), scale, offset


TALL_SCALE = 0.03


def tall_scene(i: int, n: int = 300):
    """make_pair(i, n, n) on a uint16 raster with raw relief 0 .. 3300 read at scale 0.03 (z up to 99 where the uint8 scenes stop at 40): the
    matched query keypoints are recomputed as the projections of the reference keypoints lifted with THAT raster.  Returns the pair."""
    p = make_pair(i, n, n)
    h, w = p.dem.shape
    raw = np.rint(p.dem.astype(np.float64) * (3300.0 / 40.0)).astype(np.uint16)
    yi, xi = ref.cells(p.kp_r, h, w)
    z = ref.lift(raw[yi, xi], TALL_SCALE).astype(np.float64)
    world = np.column_stack([p.kp_r.astype(np.float64), z])
    cam = world @ p.R_gt.T + p.t_gt.T
    uv = (cam[:, :2] / cam[:, 2:3]) * np.array([K_MATRIX[0, 0], K_MATRIX[1, 1]]) + np.array([K_MATRIX[0, 2], K_MATRIX[1, 2]])
    kp_q = p.kp_q.copy()
    m = p.gt_q2r >= 0
    kp_q[m] = uv[p.gt_q2r[m]].astype(np.float32)
    return dataclasses.replace(p, kp_q=kp_q, dem=raw)


def gt_points(p, dem, scale=1.0, offset=0.0):
    """(obj (k, 3) f32, img (k, 2) f32) of the scene's ground-truth matches, the reference side lifted with `dem`."""
    m = np.nonzero(p.gt_q2r >= 0)[0]
    r = p.kp_r[p.gt_q2r[m]]
    yi, xi = ref.cells(r, *dem.shape)
    return np.column_stack([r, ref.lift(dem[yi, xi], scale, offset)]).astype(np.float32), p.kp_q[m].astype(np.float32)


def void_cells(p, fraction: float, seed: int, every: bool = False):
    """The pair's uint16 raster as int16 with `fraction` of the cells under its reference keypoints (all of them with every=True) set to -32768."""
    dem = p.dem.astype(np.int16).copy()
    yi, xi = ref.cells(p.kp_r, *dem.shape)
    pick = np.ones(len(yi), bool) if every else np.random.default_rng(seed).random(len(yi)) < fraction
    dem[yi[pick], xi[pick]] = -32768
    return dataclasses.replace(p, dem=dem)


def warp_raster(name: str, H: int = 61, W: int = 83, seed: int = 5):
    """A raster of dtype `name` that uses the type's range (values near both ends, so saturation and the sign matter)."""
    rng = np.random.default_rng(seed)
    if name == "uint8":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if name == "uint16":
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    if name == "int16":
        return rng.integers(-32768, 32768, (H, W)).astype(np.int16)
    return (rng.standard_normal((H, W)) * 1000.0).astype(np.float32)


VOID_VALUE = {"uint8": 255, "uint16": 65535, "int16": -32768, "float32": -9999.0}


def with_voids(dem: np.ndarray, crop_shape, block: bool):
    """`dem` with its void value cleared elsewhere and then written into one cell near the centre (block=False) or into a 6 x 9 block that
    touches the left edge of the centre crop (block=True)."""
    nd = VOID_VALUE[dem.dtype.name]
    d = dem.copy()
    d[d == nd] = 7
    H, W = d.shape
    dx, dy = W // 2 - crop_shape[1] // 2, H // 2 - crop_shape[0] // 2
    if block:
        d[dy + 10:dy + 16, dx:dx + 9] = nd
    else:
        d[H // 2 + 3, W // 2 - 5] = nd
    return d, nd

"""numpy restatements of the elevation-raster semantics (DESIGN.md "Elevation rasters: element types, scale, offset, voids"), for the tests:

  lift           z = (float)(raw * scale + offset): product and sum in f64, rounded once each, then rounded to f32
  is_void        raw == nodata; for a float raster every non-finite cell too
  gather         gn_gather_points under a DEM format: cell choice (floorf, clamped), lift, stable removal of the matches on void cells
  warp_dem       the DEM channel of gn_stereo_reference_dem for the non-8-bit types, in np.float32 arithmetic elementwise (numpy rounds every
                 f32 product and sum on its own, which is the kernel's rounding order), rint + saturation for the integer types, and the void rule

Nothing here imports the package: the restatements stand on numpy (and on the warp oracle's coordinate arithmetic) alone.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import stereo_warp as sw  # noqa: E402

LIMITS = {"uint8": (0, 255), "uint16": (0, 65535), "int16": (-32768, 32767)}


def lift(raw: np.ndarray, scale: float = 1.0, offset: float = 0.0) -> np.ndarray:
    prod = np.asarray(raw).astype(np.float64) * np.float64(scale)      # rounded once
    return (prod + np.float64(offset)).astype(np.float32)              # rounded once, then to f32


def is_void(raw: np.ndarray, nodata) -> np.ndarray:
    raw = np.asarray(raw)
    if nodata is None:
        return np.zeros(raw.shape, bool)
    void = raw.astype(np.float64) == np.float64(nodata)
    if raw.dtype.kind == "f":
        void |= ~np.isfinite(raw)
    return void


def cells(xy: np.ndarray, H: int, W: int):
    """(yi, xi) of f32 keypoints: floorf, clamped to the raster."""
    xy = np.asarray(xy, np.float32)
    xi = np.clip(np.floor(xy[:, 0]).astype(np.int64), 0, W - 1)
    yi = np.clip(np.floor(xy[:, 1]).astype(np.int64), 0, H - 1)
    return yi, xi


def gather(kpt_q, kpt_r, idx, n_match, dem, scale=1.0, offset=0.0, nodata=None, score=None):
    """kpt_q / kpt_r [B][S][>= 2] f32 (x, y first), idx [B][kmax][2], n_match [B], dem [B][H][W] (any of the four dtypes), score [B][kmax] or None.
    Returns dict(idx, score, n_match, mkp_q [B][kmax][2], obj [B][kmax][3], dropped [B]): the first n_match[b] rows of every list are defined."""
    B, kmax = idx.shape[0], idx.shape[1]
    H, W = dem.shape[1], dem.shape[2]
    out = dict(idx=np.zeros_like(idx), score=None if score is None else np.zeros_like(score), n_match=np.zeros(B, np.int32),
               mkp_q=np.zeros((B, kmax, 2), np.float32), obj=np.zeros((B, kmax, 3), np.float32), dropped=np.zeros(B, np.int32))
    for b in range(B):
        n = int(n_match[b])
        iq, ir = idx[b, :n, 0], idx[b, :n, 1]
        q, r = np.asarray(kpt_q[b], np.float32)[iq, :2], np.asarray(kpt_r[b], np.float32)[ir, :2]
        yi, xi = cells(r, H, W)
        raw = dem[b][yi, xi]
        keep = ~is_void(raw, nodata)
        m = int(keep.sum())
        out["idx"][b, :m] = idx[b, :n][keep]
        if score is not None:
            out["score"][b, :m] = score[b, :n][keep]
        out["mkp_q"][b, :m] = q[keep]
        out["obj"][b, :m, :2] = r[keep]
        out["obj"][b, :m, 2] = lift(raw, scale, offset)[keep]
        out["n_match"][b], out["dropped"][b] = m, n - m
    return out


def warp_coords(H: int, W: int, angle_degrees: float, crop_shape):
    """Source cell (sy, sx) and 1/32 fractions (fy, fx) of every output cell of the rotated, centre-cropped raster: the coordinate arithmetic
    of cv2.warpAffine's fixed-point path as oracle/stereo_warp.py states it."""
    center = (W // 2, H // 2)
    m = sw.get_rotation_matrix_2d(center, angle_degrees, 1.0)
    dx, dy = center[0] - crop_shape[1] // 2, center[1] - crop_shape[0] // 2
    M = sw.invert_affine(m).reshape(6)
    xs = np.arange(W, dtype=np.float64)[dx:dx + crop_shape[1]]
    ys = np.arange(H, dtype=np.float64)[dy:dy + crop_shape[0]]
    adelta = np.rint(M[0] * xs * 1024).astype(np.int64)
    bdelta = np.rint(M[3] * xs * 1024).astype(np.int64)
    X0 = np.rint((M[1] * ys + M[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((M[4] * ys + M[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return np.clip(Y >> 5, -32768, 32767), np.clip(X >> 5, -32768, 32767), Y & 31, X & 31


def warp_dem(dem: np.ndarray, angle_degrees: float, crop_shape, nodata=None) -> np.ndarray:
    """The DEM channel of gn_stereo_reference_dem for uint16 / int16 / float32 (a uint8 raster keeps the fixed-point form: warp_dem_u8)."""
    dem = np.asarray(dem)
    assert dem.dtype.name in ("uint16", "int16", "float32")
    H, W = dem.shape
    sy, sx, fy, fx = warp_coords(H, W, angle_degrees, crop_shape)
    f32 = np.float32
    wts = [((32 - fx) * (32 - fy)).astype(f32) / f32(1024), (fx * (32 - fy)).astype(f32) / f32(1024),
           ((32 - fx) * fy).astype(f32) / f32(1024), (fx * fy).astype(f32) / f32(1024)]
    hole = np.zeros(sy.shape, bool)
    prods = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            yy, xx = sy + oy, sx + ox
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            live = wts[k] != 0
            raw = dem[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            t = np.where(inside & live, raw.astype(f32), f32(0))      # taps outside the source, and taps of zero weight, read 0
            prods.append((t * wts[k]).astype(f32))
            if nodata is not None:
                hole |= live & (~inside | is_void(raw, nodata))
        v = (((prods[0] + prods[1]).astype(f32) + prods[2]).astype(f32) + prods[3]).astype(f32)
        if dem.dtype.kind == "f":
            out = v
        else:
            lo, hi = LIMITS[dem.dtype.name]
            out = np.clip(np.rint(v), lo, hi).astype(dem.dtype)      # rint: half to even
    if nodata is not None:
        out = np.where(hole, np.asarray(nodata).astype(dem.dtype), out)
    return out.astype(dem.dtype)


def warp_dem_u8(dem: np.ndarray, angle_degrees: float, crop_shape, nodata=None) -> np.ndarray:
    """uint8: the fixed-point channel of gn_stereo_reference (oracle/stereo_warp.py), with the void rule on top."""
    dem = np.asarray(dem, np.uint8)
    H, W = dem.shape
    out = sw.rotate_and_crop_center(dem, angle_degrees, crop_shape)[0]
    if nodata is None:
        return out
    sy, sx, fy, fx = warp_coords(H, W, angle_degrees, crop_shape)
    wts = [(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy]
    hole = np.zeros(sy.shape, bool)
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + oy, sx + ox
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        raw = dem[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        hole |= (wts[k] != 0) & (~inside | is_void(raw, nodata))
    return np.where(hole, np.uint8(nodata), out).astype(np.uint8)


def crop(dem: np.ndarray, crop_shape) -> np.ndarray:
    """The centre crop gn_stereo_reference_dem takes at angle 0."""
    H, W = dem.shape
    dx, dy = W // 2 - crop_shape[1] // 2, H // 2 - crop_shape[0] // 2
    return dem[dy:dy + crop_shape[0], dx:dx + crop_shape[1]]

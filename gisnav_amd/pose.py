"""Seam B2: `compute_pose(camera_info, mkp_qry, mkp_ref, elevation)`.

Mirror of ros/gisnav/gisnav/core/_shared.py:89-125 (also used by TwistNode with a zero DEM,
core/twist_node.py:289): numpy in, `(R (3,3) f64, t (3,1) f64)` out.  The DEM lookup is the
host-side marshalling of the reference's `_compute_3d_points`; RANSAC, EPnP, the iterative refinement
and Rodrigues run in `gn_pnp_ransac` on the GPU.  Returns None where the reference would fail
(cv2 returning no model).  `return_covariance=True` adds the 6x6 covariance of (rvec, tvec) from the
inliers (`gn_pnp_ransac_cov`, DESIGN.md "Pose covariance"), or None in its place when it is not defined.
`use_distortion=True` passes `camera_info.d` as distCoeffs (`gn_set_distortion`); the default ignores it, as the reference does.
`ransac_iterations=N` (1 .. 4096) is cv2.solvePnPRansac's iterationsCount for this call; the default is the reference's 10, and the
engine's own `set_ransac` state is neither read nor changed.
`return_inliers=True` appends cv2.solvePnPRansac's fourth return value: `inliers`, an (n_inliers, 1) int32 array of ascending indices into
`mkp_qry` / `mkp_ref` (`gn_pnp_ransac_report`); `return_residuals=True` after it the per-point pixel residual (n,) f32 at the returned pose.

`compute_pose_batch(camera_infos, mkp_qry_list, mkp_ref_list, elevations)` is the same seam for B messages that each carry their own
`CameraInfo`: one `gn_pnp_ransac` call with a per-pair camera table (`gn_set_pair_cameras`), one result per message.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import PoseEngine, RANSAC_ITERATIONS, check_dem_format, check_ransac_iterations

_default_engine: Optional[PoseEngine] = None


def _engine(max_pts: int) -> PoseEngine:
    global _default_engine
    if _default_engine is None or _default_engine.kmax < max_pts:
        _default_engine = PoseEngine(0, max_batch=1, max_kpts=max(max_pts, 1024))
    return _default_engine


def init(device: int = 0, max_points: int = 4096) -> PoseEngine:
    """Create the module-level solver context ahead of time (otherwise the first compute_pose call pays the hipMalloc inside
    the ROS callback)."""
    global _default_engine
    if _default_engine is None or _default_engine.kmax < max_points or (_default_engine.device.index or 0) != device:
        _default_engine = PoseEngine(device, max_batch=1, max_kpts=max(max_points, 1024))
    return _default_engine


def distortion_of(camera_info) -> np.ndarray:
    """The plumb-bob coefficients of a CameraInfo-like object as distCoeffs: `d` (missing or empty = none: an empty array).  A
    `distortion_model` other than "" or "plumb_bob" raises ValueError -- ignoring it would silently bias the pose."""
    model = getattr(camera_info, "distortion_model", "") or ""
    if model not in ("", "plumb_bob"):
        raise ValueError(f"distortion model {model!r} is not supported (plumb_bob only)")
    d = getattr(camera_info, "d", None)
    return np.zeros(0, np.float64) if d is None else np.asarray(d, np.float64).reshape(-1)


def lift_points(mkp_qry, mkp_ref, elevation, dem_scale: float = 1.0, dem_offset: float = 0.0, dem_nodata=None):
    """The host-side twin of gn_gather_points' lift under a DEM format (PoseEngine.set_dem_format): object points (n', 3) f32 = reference
    keypoint + z = (float)(raw * dem_scale + dem_offset) of the cell under it (product and sum in f64, rounded once each; z = 0 without a
    raster), and the query points (n', 2) f32 of the same rows.  With dem_nodata, rows whose cell is void (raw == dem_nodata; non-finite for a
    float raster) are dropped, order kept: n' <= n.  The raster keeps its dtype (uint8 / uint16 / int16 / float32); the argument rules are
    check_dem_format's."""
    obj = np.zeros((len(mkp_ref), 3), np.float32)
    obj[:, :2] = mkp_ref
    img = np.ascontiguousarray(mkp_qry, dtype=np.float32)
    if elevation is None:
        return obj, img
    elevation = np.asarray(elevation)
    cell = np.floor(np.asarray(mkp_ref)).astype(np.intp)
    raw = elevation[cell[:, 1], cell[:, 0]]
    if dem_scale == 1.0 and dem_offset == 0.0 and dem_nodata is None:      # nothing set: the raster as it always was read, whatever its dtype
        obj[:, 2] = raw
        return obj, img
    _, scale, offset, has_nodata, nodata = check_dem_format(elevation.dtype, dem_scale, dem_offset, dem_nodata)
    if scale == 1.0 and offset == 0.0:
        obj[:, 2] = raw
    else:
        obj[:, 2] = (raw.astype(np.float64) * scale + offset).astype(np.float32)
    if has_nodata:
        void = raw.astype(np.float64) == nodata
        if raw.dtype.kind == "f":
            void |= ~np.isfinite(raw)
        obj, img = np.ascontiguousarray(obj[~void]), np.ascontiguousarray(img[~void])
    return obj, img


def compute_pose(camera_info, mkp_qry: np.ndarray, mkp_ref: np.ndarray, elevation: Optional[np.ndarray],
                 engine: Optional[PoseEngine] = None, return_covariance: bool = False, sigma_px: float = 0.0,
                 use_distortion: bool = False, ransac_iterations: Optional[int] = None, return_inliers: bool = False,
                 return_residuals: bool = False, dem_scale: float = 1.0, dem_offset: float = 0.0,
                 dem_nodata=None) -> Optional[Tuple[np.ndarray, ...]]:
    iterations = RANSAC_ITERATIONS if ransac_iterations is None else check_ransac_iterations(ransac_iterations)
    dist = distortion_of(camera_info) if use_distortion else None      # (checked before anything else: an unsupported model raises)
    # the lift: reference keypoint + the DEM cell under it under (dem_scale, dem_offset); rows on a void cell (dem_nodata) are dropped here,
    # so everything below -- the 4-point rule, PnP, return_inliers' indices -- sees the shortened list
    if len(mkp_qry) < 4:
        return None
    obj, img = lift_points(mkp_qry, mkp_ref, elevation, dem_scale, dem_offset, dem_nodata)
    n = len(img)
    if n < 4:                     # cv2.solvePnPRansac asserts npoints >= 4 (the reference would raise); the shim reports "no pose"
        return None
    eng = engine or _engine(n)
    # (obj / img: the f32 arrays gn_pnp_ransac reads; reference: _shared.py:95-102)
    k_matrix = np.asarray(camera_info.k, dtype=np.float64).reshape((3, 3))
    report = return_inliers or return_residuals
    res = eng.pnp_ransac_host(obj, img, k_matrix, iterations, min_pts=4,   # n == 4: OpenCV's P3P branch
                              covariance=return_covariance, sigma_px=sigma_px, dist=dist, **({"report": True} if report else {}))
    if not res[3]:
        return None
    out = (res[0], res[1]) + (((res[4] if res[6] else None),) if return_covariance else ())
    if return_inliers:
        out += (res[-2],)
    if return_residuals:
        out += (res[-1],)
    return out


_batch_engine: Optional[PoseEngine] = None


def _engine_batch(B: int, max_pts: int) -> PoseEngine:
    global _batch_engine
    if _batch_engine is None or _batch_engine.kmax < max_pts or _batch_engine.max_batch < B:
        _batch_engine = PoseEngine(0, max_batch=max(B, 32), max_kpts=max(max_pts, 1024))
    return _batch_engine


def compute_pose_batch(camera_infos: Sequence, mkp_qry_list: Sequence[np.ndarray], mkp_ref_list: Sequence[np.ndarray],
                       elevations: Sequence[Optional[np.ndarray]], *, use_distortion: bool = False, ransac_iterations: Optional[int] = None,
                       return_inliers: bool = False, engine: Optional[PoseEngine] = None, dem_scale: float = 1.0, dem_offset: float = 0.0,
                       dem_nodata=None) -> List[Optional[Tuple[np.ndarray, ...]]]:
    """compute_pose for B messages with their own CameraInfo each, as ONE PnP call: message b is solved with camera_infos[b].k (and, with
    use_distortion, camera_infos[b].d) through a per-pair camera table.  Returns a list with, per message, what compute_pose returns: (R, t),
    with return_inliers (R, t, inliers), or None (fewer than 4 points, or no model).
    use_distortion=True reads every camera_info.d through distortion_of (an unsupported model raises, before any GPU call) and runs the
    plumb-bob kernels for the whole batch whenever any message has a non-zero coefficient: a message without coefficients is then a pinhole
    camera run through them -- the same pose as compute_pose's up to rounding (1e-8 relative), the same bits for the messages that have some."""
    B = len(camera_infos)
    if not (len(mkp_qry_list) == len(mkp_ref_list) == len(elevations) == B):
        raise ValueError("compute_pose_batch: camera_infos, mkp_qry_list, mkp_ref_list and elevations must have one entry per message")
    iterations = RANSAC_ITERATIONS if ransac_iterations is None else check_ransac_iterations(ransac_iterations)
    dists = None
    if use_distortion:
        dists = np.zeros((B, 5), np.float64)
        for b, ci in enumerate(camera_infos):
            d = distortion_of(ci)
            if d.size not in (0, 4, 5):
                raise ValueError(f"message {b}: {d.size} distortion coefficients (plumb-bob has 4 or 5)")
            dists[b, :d.size] = d
        if not dists.any():
            dists = None      # no message is distorted: the pinhole kernels, as compute_pose runs them
    results: List[Optional[Tuple[np.ndarray, ...]]] = [None] * B
    # compute_pose's lift per message (dem_scale / dem_offset / dem_nodata: one format for the batch); rows on void cells are dropped here
    lifted = [lift_points(mkp_qry_list[b], mkp_ref_list[b], elevations[b], dem_scale, dem_offset, dem_nodata) if len(mkp_qry_list[b]) >= 4 else None
              for b in range(B)]
    live = [b for b in range(B) if lifted[b] is not None and len(lifted[b][1]) >= 4]      # (compute_pose: fewer than 4 points = no pose)
    if not live:
        return results
    n = np.array([len(lifted[b][1]) for b in live], np.int32)
    S = int(n.max())
    eng = engine or _engine_batch(len(live), S)
    obj = np.zeros((len(live), S, 3), np.float32)
    img = np.zeros((len(live), S, 2), np.float32)
    for k, b in enumerate(live):
        obj[k, :n[k]], img[k, :n[k]] = lifted[b]
    K = np.stack([np.asarray(camera_infos[b].k, np.float64).reshape(3, 3) for b in live])
    cams, model = eng.pair_cameras(K, None if dists is None else dists[live])
    res = eng.pnp_ransac(eng.to_device("cpb_obj", obj), eng.to_device("cpb_img", img), eng.to_device("cpb_n", n, torch.int32), None, iterations,
                         min_pts=4, report=return_inliers, cameras=cams, camera_model=model)
    R, t, n_inl, ok = eng.to_host(*res[:4])
    idx = eng.to_host(res[-2])[0] if return_inliers else None
    for k, b in enumerate(live):
        if not ok[k]:
            continue
        results[b] = (R[k], t[k]) + ((idx[k, :int(n_inl[k])].reshape(-1, 1).astype(np.int32),) if return_inliers else ())
    return results

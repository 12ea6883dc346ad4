"""Host-side mirror of `kornia.feature.LoFTR` -- the detector-free matcher BASELINE.json's north_star / configs[1] name ("LoFTR matcher on
1 MI355X, HIP conv + attention kernels, fp32").  The reference tree no longer contains it (only the word: docs/vitepress/docs/glossary.md:186);
older GISNav releases called `LoFTR(pretrained="outdoor")({"image0": ..., "image1": ...})` and read `keypoints0`, `keypoints1`, `confidence`
from the result -- the call signature and output dictionary mirrored here.  Marshalling only: backbone, linear-attention transformer,
dual-softmax coarse matching and the fine level run in libgisnav_amd.so (`gn_loftr_*`, csrc/gn_loftr.hip)."""
from __future__ import annotations

import contextlib

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib


class LoFTR:
    """`LoFTR(state_dict=...).to("cuda:0").eval()`; `out = m({"image0": img0, "image1": img1})` with (B, 1, H, W), (B, H, W) or (H, W) float
    images in [0, 1] of equal size (H, W multiples of 8) -> {"keypoints0" (M, 2), "keypoints1" (M, 2), "confidence" (M,), "batch_indexes" (M,)}
    on the input device: the matches of all B pairs in ascending (pair, coarse cell of image0) order, `batch_indexes` the pair of each (kornia's
    layout).  The B pairs go through ONE call of the library (gn_loftr_match_batch); a pair's rows do not depend on the batch it is in, bit for
    bit.  `fine=False` stops after the coarse level (keypoints on the 1/8 grid).  `certify="flags" | "rerun"` (off by default)
    certifies each pair's coarse (i, j) list against exact f32: flagged pairs are reported (`match_segments(...)["uncertain"]`) or, with
    "rerun" on `arithmetic="split_fp16"`, repeated on the exact-f32 kernels inside the call; eps from `certify_eps=` or `calibrate_certify`."""

    def __init__(self, pretrained: Optional[str] = None, *, state_dict: Optional[Dict] = None, max_matches: Optional[int] = None, fine: bool = True, graph: bool = True,
                 arithmetic: str = "exact_f32", certify=False, certify_eps: Optional[float] = None):
        if state_dict is None:
            state_dict = self._find_pretrained(pretrained or "outdoor")
        # max_matches None = every mutual match (at most one per coarse cell of image0), as kornia returns them; a number caps the list (first in raster order)
        self._sd, self._max, self._fine, self._graph = state_dict, (None if max_matches is None else int(max_matches)), bool(fine), bool(graph)
        self._arith = {"exact_f32": 0, "split_fp16": 1}[arithmetic]   # split_fp16: f32-accurate 2-term fp16 operands (gn_loftr_set_arithmetic)
        # certify (gn_loftr_set_certify): False off; "flags" marks the pairs whose coarse (i, j) list the arithmetic's error could change;
        # "rerun" (split_fp16 only) also repeats them on the exact-f32 kernels inside the call.  eps: `certify_eps` for every image shape, or
        # the one `calibrate_certify` measured, kept per (H, W) and re-applied when the context is re-created
        if certify not in (False, None, "flags", "rerun"):
            raise _lib.GnError(f"certify must be False, 'flags' or 'rerun', got {certify!r}")
        self._certify = {"flags": 1, "rerun": 2}.get(certify, 0)
        if self._certify == 2 and self._arith != 1:
            raise _lib.GnError("certify='rerun' repeats flagged pairs in exact f32: it needs arithmetic='split_fp16'")
        if certify_eps is not None and not 0.0 <= float(certify_eps) < 1.0:
            raise _lib.GnError(f"certify_eps must lie in [0, 1), got {certify_eps!r}")
        self._eps_all, self._eps = (None if certify_eps is None else float(certify_eps)), {}
        self._ctx, self._shape, self._device, self._pairs = None, None, None, 0
        self._knobs = {}                               # debug_variant: developer knobs, re-applied to every context this object creates
        self.lib = None

    @staticmethod
    def _find_pretrained(name: str):
        """kornia downloads `loftr_{name}.ckpt` through torch.hub; this mirror looks in the same cache directory (and in
        $GISNAV_AMD_LOFTR_WEIGHTS) but never downloads."""
        import os
        cands = [os.environ.get("GISNAV_AMD_LOFTR_WEIGHTS")]
        try:
            cands.append(os.path.join(torch.hub.get_dir(), "checkpoints", f"loftr_{name}.ckpt"))
        except Exception:  # noqa: BLE001
            pass
        for c in cands:
            if c and os.path.exists(c):
                sd = torch.load(c, map_location="cpu", weights_only=True)
                return sd.get("state_dict", sd)
        return None

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GnError("gisnav_amd.LoFTR runs on an MI355X only (no CPU path)")
        if self._sd is None:
            raise _lib.GnError("no LoFTR weights: kornia would download loftr_outdoor.ckpt here; offline, put the checkpoint into torch.hub's "
                               "checkpoints directory, set GISNAV_AMD_LOFTR_WEIGHTS, or pass state_dict=")
        self._device = device
        self.lib = _lib.load()
        return self

    def eval(self):
        return self

    def __del__(self):
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx and self.lib is not None:
            self.lib.gn_loftr_destroy(ctx)

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            msg = self.lib.gn_loftr_last_error(self._ctx).decode() if self._ctx else self.lib.gn_loftr_last_error(None).decode()
            raise _lib.GnError(f"{what} failed ({rc}): {msg}")

    def _cap(self, H: int, W: int) -> int:
        L = (H // 8) * (W // 8)
        return min(L if self._max is None else min(self._max, L), 131072)     # (gn_loftr_create's own bound)

    def _ensure(self, H: int, W: int, B: int = 1) -> None:
        """One context per image shape, sized for the largest batch seen: re-created only when the shape changes or B exceeds its max_pairs."""
        if self._ctx is not None and self._shape == (H, W) and B <= self._pairs:
            return
        if self._ctx is not None:
            self.lib.gn_loftr_destroy(self._ctx)
            self._ctx = None
        ctx = C.c_void_p()
        pairs = max(B, self._pairs if self._shape == (H, W) else 1)
        rc = self.lib.gn_loftr_create_batch(self._device.index or 0, pairs, H, W, self._cap(H, W), int(self._fine), C.byref(ctx))
        if rc < 0:
            raise _lib.GnError(f"gn_loftr_create_batch failed ({rc}): {self.lib.gn_loftr_last_error(None).decode()}")
        self._ctx, self._shape, self._pairs = ctx, (H, W), pairs
        self.lib.gn_loftr_set_graph(ctx, int(self._graph))
        self.lib.gn_loftr_set_arithmetic(ctx, self._arith)
        for which, value in self._knobs.items():
            self._check(self.lib.gn_loftr_debug_set_variant(ctx, which, value), f"gn_loftr_debug_set_variant({which}, {value})")
        for name, arr in self._sd.items():
            if hasattr(arr, "detach"):
                arr = arr.detach().cpu().numpy()
            if name.startswith("matcher."):            # kornia's checkpoint nests the model under `matcher.`
                name = name[len("matcher."):]
            if name.endswith("num_batches_tracked") or name == "pos_encoding.pe" or (not self._fine and (name.startswith("loftr_fine") or name.startswith("fine_preprocess"))):
                continue
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*(arr.shape if arr.ndim else (1,)))
            self._check(self.lib.gn_loftr_load_tensor(ctx, name.encode(), arr.ctypes.data_as(C.c_void_p), shape, max(arr.ndim, 1)), f"gn_loftr_load_tensor({name})")
        missing = self.lib.gn_loftr_missing_tensors(ctx)
        if missing:
            raise _lib.GnError(f"{missing} required LoFTR tensors missing from the state dict")
        eps = self._eps.get((H, W), self._eps_all)
        if self._certify and eps is not None:          # (a shape without an eps is refused by match_segments)
            self._check(self.lib.gn_loftr_set_certify(ctx, self._certify, eps), "gn_loftr_set_certify")

    def calibrate_certify(self, image0, image1, safety: float = 4.0, floor_eps: float = 1e-5) -> Dict[str, float]:
        """Measure the certificate's eps for this image shape on a sample of pairs (gn_loftr_calibrate_certify): the sample runs in split-fp16
        and in exact-f32 arithmetic, d_max = the largest entry-wise difference of the two dual-softmax confidence matrices over the sample,
        eps = max(floor_eps, safety x d_max).  The eps is kept for (H, W) and used by every later call on that shape.  Returns {"d_max", "eps"}."""
        B, H, W = self._batch_shape(image0, image1)
        if self._device is None:
            raise _lib.GnError("call .to(device) first")
        f = lambda t: t.to(device=self._device, dtype=torch.float32).reshape(B, H, W).contiguous()  # noqa: E731
        a, b = f(image0), f(image1)
        self._ensure(H, W, B)
        out = (C.c_float * 2)()
        stream = C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
        self._check(self.lib.gn_loftr_calibrate_certify(self._ctx, B, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), float(safety), float(floor_eps), out, stream),
                    "gn_loftr_calibrate_certify")
        self._eps[(H, W)] = float(out[1])
        if self._certify:
            self._check(self.lib.gn_loftr_set_certify(self._ctx, self._certify, -1.0), "gn_loftr_set_certify")     # eps < 0: the calibrated one
        return {"d_max": float(out[0]), "eps": float(out[1])}

    def set_certify_eps(self, eps: float) -> None:
        """State the certificate's eps for every image shape from now on (replaces `certify_eps` and any calibrated value)."""
        if not 0.0 <= float(eps) < 1.0:
            raise _lib.GnError(f"certify_eps must lie in [0, 1), got {eps!r}")
        self._eps_all, self._eps = float(eps), {}
        if self._ctx is not None and self._certify:
            self._check(self.lib.gn_loftr_set_certify(self._ctx, self._certify, self._eps_all), "gn_loftr_set_certify")

    def certify_stats(self) -> Dict[str, int]:
        """Counters of the current context since it was created: pairs seen by certified calls, pairs the certificate flagged, pairs repeated
        in exact f32 because of a flag, pairs repeated because the fp16-range guard tripped."""
        keys = ("pairs", "flagged", "rerun_certificate", "rerun_guard")
        if self._ctx is None:
            return dict.fromkeys(keys, 0)
        out = (C.c_int64 * 4)()
        self._check(self.lib.gn_loftr_get_certify_stats(self._ctx, out), "gn_loftr_get_certify_stats")
        return {k: int(v) for k, v in zip(keys, out)}

    @staticmethod
    def _batch_shape(i0, i1):
        """(B, H, W) of the two inputs, which must agree in all three -- checked on the shapes alone, before anything touches the device."""
        def one(t, name):
            sh = tuple(int(v) for v in t.shape)
            if len(sh) == 2:
                return (1,) + sh
            if len(sh) == 3:
                return sh
            if len(sh) == 4 and sh[1] == 1:
                return (sh[0], sh[2], sh[3])
            raise _lib.GnError(f"{name}: expected (B, 1, H, W), (B, H, W) or (H, W), got {sh}")
        s0, s1 = one(i0, "image0"), one(i1, "image1")
        if s0 != s1:
            raise _lib.GnError(f"image0 {s0} and image1 {s1} must have one batch size and one image size (the published model pads / masks otherwise; not built)")
        if s0[0] < 1:
            raise _lib.GnError("empty batch")
        return s0

    @torch.inference_mode()
    def match_segments(self, image0, image1, host_counts: bool = True):
        """The library's own output layout for B pairs (one gn_loftr_match_batch): {"keypoints0" / "keypoints1" (B, cap, 2), "confidence" (B, cap),
        "ij" (B, cap, 2) int32, "n" (B,) int32} on the matcher's device -- pair b's matches are the first n[b] rows of its segment, which is what
        gn_gather_points / gn_pnp_ransac take -- and "n_host" (list of B ints, or None with host_counts=False: in exact-f32 arithmetic the call
        then does not synchronise the stream)."""
        B, H, W = self._batch_shape(image0, image1)
        if self._device is None:
            raise _lib.GnError("call .to(device) first")
        f = lambda t: t.to(device=self._device, dtype=torch.float32).reshape(B, H, W).contiguous()  # noqa: E731
        a, b = f(image0), f(image1)
        self._ensure(H, W, B)
        if self._certify and self._eps.get((H, W), self._eps_all) is None:
            raise _lib.GnError(f"certify is on but no eps is known for {H}x{W} images: pass certify_eps= or call calibrate_certify on a sample of that shape")
        M = self._cap(H, W)
        k0 = torch.empty((B, M, 2), dtype=torch.float32, device=self._device); k1 = torch.empty_like(k0)
        conf = torch.empty((B, M), dtype=torch.float32, device=self._device)
        ij = torch.empty((B, M, 2), dtype=torch.int32, device=self._device)
        n_dev = torch.empty((B,), dtype=torch.int32, device=self._device)
        n = (C.c_int32 * B)() if host_counts else None
        stream = C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        self._check(self.lib.gn_loftr_match_batch(self._ctx, B, p(a), p(b), p(k0), p(k1), p(conf), p(ij), p(n_dev), n, stream), "gn_loftr_match_batch")
        out = {"keypoints0": k0, "keypoints1": k1, "confidence": conf, "ij": ij, "n": n_dev, "n_host": [int(v) for v in n] if host_counts else None}
        if self._certify:
            flags = (C.c_int32 * B)()
            self._check(self.lib.gn_loftr_get_uncertain(self._ctx, B, flags), "gn_loftr_get_uncertain")
            out["uncertain"] = torch.tensor([bool(v) for v in flags], dtype=torch.bool)
        return out

    @torch.inference_mode()
    def __call__(self, data: Dict[str, torch.Tensor], with_ids: bool = False) -> Dict[str, torch.Tensor]:
        i0, i1 = data["image0"], data["image1"]
        self._batch_shape(i0, i1)                      # (refused on the shapes alone, before any device call)
        if self._device is None:
            raise _lib.GnError("call .to(device) first")
        in_dev = i0.device
        seg = self.match_segments(i0, i1)
        ns = seg["n_host"]
        cat = lambda t: (t[0, :ns[0]] if len(ns) == 1 else torch.cat([t[b, :m] for b, m in enumerate(ns)], 0)).to(in_dev)  # noqa: E731
        out = {"keypoints0": cat(seg["keypoints0"]), "keypoints1": cat(seg["keypoints1"]), "confidence": cat(seg["confidence"]),
               "batch_indexes": torch.zeros(ns[0], dtype=torch.int64, device=in_dev) if len(ns) == 1 else
               torch.repeat_interleave(torch.arange(len(ns), dtype=torch.int64, device=self._device), seg["n"].long(), output_size=sum(ns)).to(in_dev)}
        if with_ids:
            ij = cat(seg["ij"])
            out["i_ids"], out["j_ids"] = ij[:, 0].long(), ij[:, 1].long()
        return out

    forward = __call__

    def debug_variant(self, which: int, value: int) -> None:
        """Developer knob `which` (41, 42 or 44: gn_loftr_debug_set_variant) of THIS matcher, whatever image shapes it goes on to see; no other
        context in the process is touched.  A knob the library refuses raises and is not kept (before the first call there is no context to ask:
        the knob is then checked when one is created)."""
        if self._ctx is not None:
            self._check(self.lib.gn_loftr_debug_set_variant(self._ctx, int(which), int(value)), f"gn_loftr_debug_set_variant({which}, {value})")
        self._knobs[int(which)] = int(value)

    def debug_read(self, name: str, count: int) -> np.ndarray:
        buf = np.empty(count, dtype=np.float32)
        n = self.lib.gn_loftr_debug_read(self._ctx, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream))
        if n < 0:
            raise _lib.GnError(f"gn_loftr_debug_read({name}) failed ({n})")
        return buf[: int(n)]


@contextlib.contextmanager
def _dem_format(engine, dem_scale, dem_offset, dem_nodata):
    """PoseEngine.set_dem_format for one call (nothing is touched while all three are the defaults)."""
    if (dem_scale, dem_offset, dem_nodata) == (1.0, 0.0, None):
        yield
        return
    before = engine.dem_format()
    engine.set_dem_format(dem_scale, dem_offset, dem_nodata)
    try:
        yield
    finally:
        engine.set_dem_format(*before)


def _dem_tensor(dem, dev) -> torch.Tensor:
    """An elevation raster (or a stack of them) on the device in its own element type: uint8, uint16, int16 or float32 (ValueError otherwise)."""
    from .engine import dem_dtype_name
    if not isinstance(dem, torch.Tensor):
        dem = torch.from_numpy(np.ascontiguousarray(dem))
    dem_dtype_name(dem.dtype)
    return dem.to(dev).contiguous()


def loftr_pose(matcher: "LoFTR", engine, frame01: torch.Tensor, tile01: torch.Tensor, dem, K, min_matches: int = 15, conf_threshold: float = 0.0,
               return_covariance: bool = False, dist=None, ransac_iterations=None, return_inliers: bool = False,
               dem_scale: float = 1.0, dem_offset: float = 0.0, dem_nodata=None):
    """Camera frame <-> map tile pose with the detector-free matcher in front of the SAME solver as the SIFT / LightGlue path: LoFTR matches
    (`keypoints0` in the frame, `keypoints1` in the tile) -> DEM lift of the tile points (`_shared.py:95-102`) -> solvePnPRansac + Rodrigues
    (`gn_gather_points`, `gn_pnp_ransac`; seam B2).  Everything stays on the device.  frame01 / tile01: (H, W) float in [0, 1];
    dem: (H, W) uint8, uint16, int16 or float32 (the raster keeps its dtype), or None; dem_scale / dem_offset / dem_nodata: z = raw * dem_scale +
    dem_offset, and matches on a cell equal to dem_nodata are dropped before PnP (PoseEngine.set_dem_format, for this call) -- n_matches and
    the inlier indices then describe the shorter list.  Returns (R (3,3), t (3,1), n_matches) or None below `min_matches` / when RANSAC finds no model;
    with return_covariance also the 6x6 covariance of (rvec, tvec) from the inliers (None when it is not defined) as a fourth entry.
    dist: distCoeffs of the frame's camera for the solver (PoseEngine.set_distortion for this call; None = the engine's state).
    ransac_iterations: cv2.solvePnPRansac's iterationsCount for this call, 1 .. 4096 (None = the reference's 10).
    return_inliers: append cv2.solvePnPRansac's `inliers`, (n_inliers, 1) int32, indexing the matches that passed `conf_threshold` in their order
    (`gn_pnp_ransac_report`)."""
    out = matcher({"image0": frame01, "image1": tile01})
    keep = out["confidence"] > conf_threshold
    k0, k1 = out["keypoints0"][keep], out["keypoints1"][keep]
    n = int(k0.shape[0])
    if n < min_matches or n > engine.kmax:
        if n > engine.kmax:
            engine.grow(((n + 1023) // 1024) * 1024)
        if n < min_matches:
            return None
    dev = engine.device
    pad = lambda k: torch.cat([k.to(dev), torch.zeros((n, 2), dtype=torch.float32, device=dev)], 1).reshape(1, n, 4).contiguous()  # noqa: E731  GN_KPT_XYSA rows
    idx = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(2).reshape(1, n, 2)
    idx_full = torch.zeros((1, engine.kmax, 2), dtype=torch.int64, device=dev)
    idx_full[0, :n] = idx[0]
    nm = torch.tensor([n], dtype=torch.int32, device=dev)
    d = None if dem is None else _dem_tensor(dem, dev)[None]
    with _dem_format(engine, dem_scale, dem_offset, dem_nodata):
        mkp, obj = engine.gather_points(pad(k0), pad(k1), idx_full, nm, d, _lib.GN_KPT_XYSA)
    if dem_nodata is not None and d is not None:
        n = int(nm.cpu()[0])      # the matches left on valid cells
    res = _pnp_with_dist(engine, dist, obj, mkp, nm, np.asarray(K, np.float64).reshape(3, 3), min_pts=min_matches, covariance=return_covariance,
                         **_iterations_kw(ransac_iterations), **_report_kw(return_inliers))
    R, t, ok = res[0], res[1], res[3]
    if not bool(ok.cpu()[0]):
        return None
    tail = (res[-2][0, :int(res[2].cpu()[0])].cpu().numpy().reshape(-1, 1),) if return_inliers else ()
    if return_covariance:
        return (R[0].cpu().numpy(), t[0].cpu().numpy(), n, (res[4][0].cpu().numpy() if bool(res[6].cpu()[0]) else None)) + tail
    return (R[0].cpu().numpy(), t[0].cpu().numpy(), n) + tail


def _iterations_kw(ransac_iterations) -> dict:
    """The `iterations` keyword of engine.pnp_ransac for a per-call count (none at all when unset: the engine's default argument stays in charge)."""
    if ransac_iterations is None:
        return {}
    from .engine import check_ransac_iterations
    return {"iterations": check_ransac_iterations(ransac_iterations)}


def _report_kw(return_inliers: bool) -> dict:
    """The `report` keyword of engine.pnp_ransac (none at all when off: the call is then the one it always was)."""
    return {"report": True} if return_inliers else {}


def _pnp_with_dist(engine, dist, *args, **kwargs):
    """engine.pnp_ransac under the distCoeffs `dist` (None: the engine's own state), the engine's state restored afterwards."""
    if dist is None:
        return engine.pnp_ransac(*args, **kwargs)
    keep = engine.distortion()
    engine.set_distortion(dist)
    try:
        return engine.pnp_ransac(*args, **kwargs)
    finally:
        engine.set_distortion(keep)


def loftr_pose_batch(matcher: "LoFTR", engine, frames01, tiles01, dems, K, min_matches: int = 15, conf_threshold: float = 0.0, return_covariance: bool = False,
                     dist=None, ransac_iterations=None, return_inliers: bool = False, dem_scale: float = 1.0, dem_offset: float = 0.0, dem_nodata=None):
    """`loftr_pose` for B pairs at once: frames01 / tiles01 (B, H, W) (or sequences of B (H, W) images), dems (B, H, W) uint8, uint16, int16 or
    float32 (or a sequence of B) or None; dem_scale / dem_offset / dem_nodata as for `loftr_pose`.  ONE batched match (the counts stay on the device), the confidence filter as a stable per-pair compaction on the device, ONE
    gn_gather_points, ONE gn_pnp_ransac over the B pairs and ONE read-back.  Returns a list of B entries, each what `loftr_pose` returns for that
    pair (None below `min_matches` / without a model).  The engine must have been created with max_batch >= B; it is grown to the matcher's
    per-pair cap when that exceeds its keypoint capacity.  dist, ransac_iterations, return_inliers: as for `loftr_pose` (the inlier indices
    ride in the one read-back).  K (B, 3, 3) with dist None or (B, 4 | 5): one camera per pair (PoseEngine.pair_cameras; with dist every pair
    runs the plumb-bob kernels, a row of zeros being a pinhole camera run through them); K (3, 3) / dist (4 | 5,): one camera for all."""
    stack = lambda x: x if isinstance(x, torch.Tensor) else torch.stack([torch.as_tensor(v) for v in x])  # noqa: E731
    frames01, tiles01 = stack(frames01), stack(tiles01)
    B, H, W = matcher._batch_shape(frames01, tiles01)
    if B > engine.max_batch:
        raise _lib.GnError(f"{B} pairs exceed the engine's max_batch {engine.max_batch}")
    seg = matcher.match_segments(frames01, tiles01, host_counts=False)
    dev = engine.device
    k0, k1, conf, n = (seg[k].to(dev) for k in ("keypoints0", "keypoints1", "confidence", "n"))
    cap = int(k0.shape[1])
    # stable per-pair compaction of the rows that pass the confidence filter (plumbing): kept rows first, in their order
    keep = (torch.arange(cap, device=dev)[None, :] < n[:, None]) & (conf > conf_threshold)
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
    cnt = keep.sum(1).to(torch.int32)
    g = lambda k: torch.cat([torch.gather(k, 1, order[:, :, None].expand(B, cap, 2)), torch.zeros((B, cap, 2), dtype=torch.float32, device=dev)], 2).contiguous()  # noqa: E731  GN_KPT_XYSA rows
    if cap > engine.kmax:
        engine.grow(((cap + 1023) // 1024) * 1024)
    idx = torch.arange(engine.kmax, dtype=torch.int64, device=dev).repeat_interleave(2).reshape(1, engine.kmax, 2).repeat(B, 1, 1)
    idx = torch.where(torch.arange(engine.kmax, device=dev)[None, :, None] < cnt[:, None, None], idx, torch.zeros_like(idx)).contiguous()
    d = None
    if dems is not None:
        d = _dem_tensor(dems if isinstance(dems, torch.Tensor) else np.stack([np.asarray(v) for v in dems]), dev)
    with _dem_format(engine, dem_scale, dem_offset, dem_nodata):
        mkp, obj = engine.gather_points(g(k0), g(k1), idx, cnt, d, _lib.GN_KPT_XYSA)
    K = np.asarray(K, np.float64)
    if K.ndim == 3:
        # one camera per pair: the one PnP call runs with a per-pair table (K (B, 3, 3), dist None or (B, 4 | 5)); checked on the host first
        if K.shape[0] != B:
            raise ValueError(f"K has {K.shape[0]} matrices for {B} pairs")
        cams, model = engine.pair_cameras(K, dist)
        res = engine.pnp_ransac(obj, mkp, cnt, None, min_pts=min_matches, covariance=return_covariance, cameras=cams, camera_model=model,
                                **_iterations_kw(ransac_iterations), **_report_kw(return_inliers))
    else:
        res = _pnp_with_dist(engine, dist, obj, mkp, cnt, K.reshape(3, 3), min_pts=min_matches, covariance=return_covariance,
                             **_iterations_kw(ransac_iterations), **_report_kw(return_inliers))
    back = [res[0], res[1], res[3], cnt] + ([res[4], res[6]] if return_covariance else []) + ([res[2], res[-2]] if return_inliers else [])
    host = engine.to_host(*back)
    R, t, ok, cn = host[:4]
    out = []
    for b in range(B):
        nb = int(cn[b])
        tail = (np.array(host[-1][b][:int(host[-2][b])], np.int32).reshape(-1, 1),) if return_inliers else ()
        if nb < min_matches or not bool(ok[b]):
            out.append(None)
        elif return_covariance:
            out.append((np.array(R[b]), np.array(t[b]), nb, np.array(host[4][b]) if bool(host[5][b]) else None) + tail)
        else:
            out.append((np.array(R[b]), np.array(t[b]), nb) + tail)
    return out

"""Device-side engine: one `PoseEngine` per GPU wraps a `gn_ctx` of libgisnav_amd.so.

PyTorch is used here only for device memory, streams and (in `dist.py`) the RCCL process
group; every numeric step of the hot path runs in the hand-written gfx950 kernels behind the
C ABI.  The engine mirrors the state PoseNode builds in its constructor
(ros/gisnav/gisnav/core/pose_node.py:81-122): a device, a LightGlue("sift") matcher with 9
layers / threshold 0.5 / no early exit, and the solvePnPRansac settings of
core/_shared.py:109-116.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import struct
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .weights import canonical_state_dict

MIN_MATCHES = 15          # PoseNode.MIN_MATCHES, pose_node.py:63
FILTER_THRESHOLD = 0.5    # PoseNode.CONFIDENCE_THRESHOLD, pose_node.py:60
RANSAC_ITERATIONS = 10    # _shared.py:115
RANSAC_REPROJ_PX = 8.0    # cv2.solvePnPRansac default
RANSAC_CONFIDENCE = 0.99  # cv2.solvePnPRansac default



def check_ransac_iterations(iterations) -> int:
    """iterationsCount as the library takes it: an integer in 1 .. GN_RANSAC_MAX_ITERATIONS (ValueError / TypeError otherwise, before any GPU call)."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)):
        raise TypeError(f"ransac iterations must be an integer, got {type(iterations).__name__}")
    if not 1 <= int(iterations) <= _lib.GN_RANSAC_MAX_ITERATIONS:
        raise ValueError(f"ransac iterations must be in 1..{_lib.GN_RANSAC_MAX_ITERATIONS}, got {int(iterations)}")
    return int(iterations)


def check_width_pruning(width_confidence, min_kpts=None) -> None:
    """The library's argument rules for gn_set_width_pruning, before any GPU call: width_confidence finite and < 1 (<= 0 = off), min_kpts None or
    an integer >= 0 (ValueError / TypeError otherwise)."""
    if isinstance(width_confidence, bool) or not isinstance(width_confidence, (int, float, np.integer, np.floating)):
        raise TypeError(f"width_confidence must be a number, got {type(width_confidence).__name__}")
    if not np.isfinite(width_confidence) or float(width_confidence) >= 1.0:
        raise ValueError(f"width_confidence must be finite and < 1 (<= 0 switches pruning off), got {width_confidence}")
    if min_kpts is not None:
        if isinstance(min_kpts, bool) or not isinstance(min_kpts, (int, np.integer)):
            raise TypeError(f"pruning min_kpts must be an integer or None, got {type(min_kpts).__name__}")
        if int(min_kpts) < 0:
            raise ValueError(f"pruning min_kpts must be >= 0 (None = the default 1536), got {int(min_kpts)}")


def check_pair_cameras(K, d=None) -> np.ndarray:
    """The rows of a per-pair camera table from B intrinsic matrices K (B, 3, 3) and B plumb-bob coefficient sets d (B, 4 | 5) or None:
    (B, GN_PAIR_CAMERA_DOUBLES) f64 = fx, fy, cx, cy, k1, k2, p1, p2, k3.  ValueError for a wrong shape, non-finite values, a last row other than
    (0, 0, 1) or a non-zero skew K[b, 0, 1] -- on the host, before any GPU call (the library cannot validate device memory)."""
    K = np.asarray(K, np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3) or K.shape[0] < 1:
        raise ValueError(f"pair_cameras: K must be (B, 3, 3), got {K.shape}")
    B = K.shape[0]
    rows = np.zeros((B, _lib.GN_PAIR_CAMERA_DOUBLES), np.float64)
    if d is not None:
        d = np.asarray(d, np.float64)
        if d.ndim != 2 or d.shape[0] != B or d.shape[1] not in (4, 5):
            raise ValueError(f"pair_cameras: d must be ({B}, 4) or ({B}, 5) plumb-bob coefficients, got {d.shape}")
        rows[:, 4:4 + d.shape[1]] = d
    if not np.isfinite(K).all() or not np.isfinite(rows).all():
        raise ValueError("pair_cameras: non-finite value")
    if (K[:, 2] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError("pair_cameras: the last row of every K must be (0, 0, 1)")
    if (K[:, 0, 1] != 0.0).any():
        raise ValueError("pair_cameras: a skew K[b, 0, 1] is not supported by the PnP stage")
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    return rows


def check_camera_table(cameras, camera_model, B: int) -> None:
    """A `cameras` argument as the calls take it: a (B, GN_PAIR_CAMERA_DOUBLES) f64 contiguous tensor (PoseEngine.pair_cameras makes one) with
    one row per pair of the call, camera_model 0 or 1.  ValueError otherwise, before any GPU call."""
    if not isinstance(cameras, torch.Tensor) or cameras.dtype != torch.float64 or cameras.dim() != 2 or cameras.shape[1] != _lib.GN_PAIR_CAMERA_DOUBLES:
        raise ValueError(f"cameras must be a (B, {_lib.GN_PAIR_CAMERA_DOUBLES}) float64 tensor (PoseEngine.pair_cameras)")
    if cameras.shape[0] != B:
        raise ValueError(f"cameras has {cameras.shape[0]} rows for a call of {B} pairs")
    if not cameras.is_contiguous():
        raise ValueError("cameras must be contiguous")
    if isinstance(camera_model, bool) or camera_model not in (0, 1):
        raise ValueError(f"camera_model must be 0 (pinhole) or 1 (plumb-bob), got {camera_model!r}")


# element types of an elevation raster (gn_set_dem_format): numpy dtype name -> (GN_DEM_* constant, lowest, highest representable value)
_DEM_TYPES = {"uint8": (_lib.GN_DEM_U8, 0, 255), "uint16": (_lib.GN_DEM_U16, 0, 65535), "int16": (_lib.GN_DEM_I16, -32768, 32767),
              "float32": (_lib.GN_DEM_F32, None, None)}


def dem_dtype_name(dtype) -> str:
    """'uint8' / 'uint16' / 'int16' / 'float32' for a torch or numpy dtype of an elevation raster; ValueError for any other."""
    name = str(dtype).replace("torch.", "") if isinstance(dtype, torch.dtype) else np.dtype(dtype).name
    if name not in _DEM_TYPES:
        raise ValueError(f"an elevation raster must be uint8, uint16, int16 or float32, got {name}")
    return name


def check_dem_format(dtype, scale=1.0, offset=0.0, nodata=None) -> Tuple[int, float, float, int, float]:
    """The library's argument rules for gn_set_dem_format, before any GPU call: (type, scale, offset, has_nodata, nodata) for a raster of
    `dtype`.  ValueError for another dtype, a scale that is zero or not finite, an offset that is not finite, or -- for the integer types -- a
    nodata that is not an integer within the type's range.  nodata None = no void value; NaN (float32 only) = the non-finite cells alone."""
    typ, lo, hi = _DEM_TYPES[dem_dtype_name(dtype)]
    for name, v in (("dem_scale", scale), ("dem_offset", offset)) + ((("dem_nodata", nodata),) if nodata is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    scale, offset = float(scale), float(offset)
    if not np.isfinite(scale) or scale == 0.0:
        raise ValueError(f"dem_scale must be finite and not zero, got {scale}")
    if not np.isfinite(offset):
        raise ValueError(f"dem_offset must be finite, got {offset}")
    if nodata is None:
        return typ, scale, offset, 0, 0.0
    nodata = float(nodata)
    if lo is not None and not (lo <= nodata <= hi and nodata == np.floor(nodata)):
        raise ValueError(f"dem_nodata {nodata} is not representable in {dem_dtype_name(dtype)} (an integer in {lo}..{hi})")
    return typ, scale, offset, 1, nodata


def _k9_ptr(K):
    """K9_host of the C calls: None (NULL) when the call runs with a per-pair table and no matrix was given."""
    return None if K is None else np.ascontiguousarray(np.asarray(K, np.float64).reshape(9)).ctypes.data_as(_lib.c_f64p)


_PRECISIONS = {"f32": _lib.GN_PREC_F32, "bf16_attn": _lib.GN_PREC_BF16_ATTN, "f32x3_bf16_attn": _lib.GN_PREC_F32X3_BF16_ATTN,
               "f16x2_bf16_attn": _lib.GN_PREC_F16X2_BF16_ATTN, "f16x2_f16_attn": _lib.GN_PREC_F16X2_F16_ATTN,
               "f16x2_f16x2_attn": _lib.GN_PREC_F16X2_F16X2_ATTN}


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dev_tensor(t, dtype, device) -> torch.Tensor:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.to(device=device, dtype=dtype, non_blocking=True) if dtype is not None else t.to(device=device, non_blocking=True)
    return t.contiguous()


def numa_cpus(node: int):
    """CPU ids of NUMA node `node` (/sys/devices/system/node/node<N>/cpulist, e.g. "0-31,128-159"), or None."""
    try:
        with open(f"/sys/devices/system/node/node{int(node)}/cpulist") as f:
            return parse_cpulist(f.read())
    except (OSError, ValueError):
        return None


def parse_cpulist(text: str):
    cpus = set()
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus or None


class RecordStager:
    """Input side of a STREAM of new frame<->tile pairs (pose_node.py:207-213, 254-265): the raw `query_sift` / reference keypoint payloads
    (532-byte KEYPOINT_DTYPE records) and the DEM rasters of a batch are copied -- bytes, no unpacking -- into pinned host buffers and
    uploaded on a copy stream into one of `depth` device slots, while the engine works on the previous batch; `k_prep` reads the records
    as they are (GN_KPT_RECORD).  The reference builds per message: np.frombuffer + np.column_stack + six torch.tensor(...).to(device)
    calls from pageable memory.

        nxt = stager.stage(msgs)          # host memcpy into pinned memory + async H2D (any thread)
        stager.wait(cur); eng.estimate(cur, K, out=out); stager.release(cur)

    Contract: every staged batch is release()d on the compute stream after the last kernel that reads it and BEFORE the stage() call that
    re-uses its slot is issued (with `depth` slots: before the depth-th following stage()); a slot whose batch was never released is
    overwritten without waiting.
    """

    def __init__(self, engine: "PoseEngine", max_batch: int, max_kpts: int, dem_hw: Tuple[int, int], depth: int = 3, copy_threads: int = 4,
                 numa: Optional[str] = "auto", dem_dtype=torch.uint8):
        import os
        from concurrent.futures import ThreadPoolExecutor
        # one rank per GPU: the copy threads of a rank stay on the cores of its GPU's NUMA node (host staging is ~6 ms of memcpy
        # per 5.8 ms step and rank; eight unpinned pools wander over both sockets).  "auto": gn_device_numa_node; None: leave the threads alone.
        self.numa_node, cpus = -1, None
        if numa == "auto":
            self.numa_node = int(engine.lib.gn_device_numa_node(engine.device.index or 0))
            cpus = numa_cpus(self.numa_node) if self.numa_node >= 0 else None
            if cpus:
                cpus = (cpus & os.sched_getaffinity(0)) or None      # never outside what the launcher allowed this process

        def _pin():
            if cpus:
                try:
                    os.sched_setaffinity(0, cpus)
                except OSError:
                    pass
        self._pin = _pin
        self.eng, self.B, self.K, self.depth = engine, int(max_batch), int(max_kpts), int(depth)
        # the pinned-memory copies of a batch (35 MB at 32 x 1024 keypoints per side) run on a few host threads: one thread's memcpy
        # (~6 GB/s) would be slower than the GPU's step; numpy releases the GIL inside the copies
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(copy_threads)), initializer=_pin) if copy_threads > 1 else None
        dev, (H, W) = engine.device, dem_hw
        self.dem_dtype = getattr(torch, dem_dtype_name(dem_dtype))      # the rasters' element type (set_dem_format): the pinned and device buffers hold it
        self.copy_stream = torch.cuda.Stream(device=dev)
        mk = lambda shape, dt, **kw: torch.empty(shape, dtype=dt, **kw)  # noqa: E731
        self.slots = []
        for _ in range(self.depth):
            host = dict(rec_q=mk((self.B, self.K, 133), torch.float32, pin_memory=True), rec_r=mk((self.B, self.K, 133), torch.float32, pin_memory=True),
                        dem=mk((self.B, H, W), self.dem_dtype, pin_memory=True), n=mk((2, self.B), torch.int32, pin_memory=True))
            devb = {k: torch.empty_like(v, device=dev) for k, v in host.items()}
            self.slots.append(dict(host=host, host_np={k: v.numpy() for k, v in host.items()}, dev=devb,
                                   uploaded=torch.cuda.Event(), consumed=torch.cuda.Event(), used=False))
        self._next = 0

    def stage(self, msgs) -> dict:
        """msgs: up to max_batch tuples (query_sift bytes, reference-keypoint bytes, dem (H, W) of the stager's dem_dtype).  Returns the inputs dict of
        `PoseEngine.estimate`; call wait() on the compute stream before using it and release() after the last kernel that reads it."""
        slot = self.slots[self._next]
        h = slot["host_np"]
        B = len(msgs)
        if B < 1 or B > self.B:
            raise _lib.GnError(f"{B} pairs staged, the stager holds 1..{self.B}")
        for b, (q, r, dem) in enumerate(msgs):      # validated BEFORE anything is copied: a refused batch leaves the slot as it was
            if len(q) % 532 or len(r) % 532:
                raise _lib.GnError(f"pair {b}: keypoint payloads must be whole 532-byte KEYPOINT_DTYPE records (got {len(q)} and {len(r)} bytes)")
            if max(len(q), len(r)) // 532 > self.K:
                raise _lib.GnError(f"pair {b}: {max(len(q), len(r)) // 532} keypoints exceed the stager's max_kpts {self.K}")
            if tuple(np.shape(dem)) != tuple(h["dem"].shape[1:]):
                raise _lib.GnError(f"pair {b}: DEM raster {tuple(np.shape(dem))}, the stager was built for {tuple(h['dem'].shape[1:])}")
            if np.asarray(dem).dtype != h["dem"].dtype:
                raise _lib.GnError(f"pair {b}: DEM raster of {np.asarray(dem).dtype}, the stager was built for {h['dem'].dtype} (dem_dtype)")

        self._next = (self._next + 1) % self.depth
        if slot["used"]:
            slot["uploaded"].synchronize()           # the pinned host buffer is free again: its H2D copy has finished
            if slot.get("released", False):
                slot["consumed"].synchronize()       # the batch that last used this slot has been read by its kernels
            else:
                torch.cuda.synchronize(self.eng.device)   # release() was never called for it: wait for everything rather than overwrite a batch in use
        slot["released"] = False

        def copy_pair(b):
            q, r, dem = msgs[b]
            nq, nr = len(q) // 532, len(r) // 532
            h["rec_q"][b, :nq] = np.frombuffer(q, dtype=np.float32).reshape(nq, 133)      # one memcpy: the wire bytes ARE the device layout
            h["rec_r"][b, :nr] = np.frombuffer(r, dtype=np.float32).reshape(nr, 133)
            h["dem"][b] = dem
            h["n"][0, b], h["n"][1, b] = nq, nr

        if self._pool is not None and B > 1:
            list(self._pool.map(copy_pair, range(B)))
        else:
            for b in range(B):
                copy_pair(b)
        d = slot["dev"]
        with torch.cuda.stream(self.copy_stream):
            for k in ("rec_q", "rec_r", "dem", "n"):
                d[k].copy_(slot["host"][k], non_blocking=True)
            slot["uploaded"].record(self.copy_stream)
        slot["used"] = True
        return dict(kpt_q=d["rec_q"][:B], kpt_r=d["rec_r"][:B], n_q=d["n"][0, :B], n_r=d["n"][1, :B], dem=d["dem"][:B],
                    desc_q=None, desc_r=None, kpt_format=_lib.GN_KPT_RECORD, _slot=slot)

    def wait(self, inputs: dict) -> None:
        torch.cuda.current_stream(self.eng.device).wait_event(inputs["_slot"]["uploaded"])

    def release(self, inputs: dict) -> None:
        inputs["_slot"]["consumed"].record(torch.cuda.current_stream(self.eng.device))
        inputs["_slot"]["released"] = True

    def close(self) -> None:
        """Stop the copy threads (the pinned buffers and device slots go with the object)."""
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class PoseEngine:
    """Batched frame<->tile matcher + PnP solver on one MI355X."""

    def __init__(self, device: int = 0, max_batch: int = 32, max_kpts: int = 1024,
                 precision: str = "f32", state_dict: Optional[Dict[str, np.ndarray]] = None,
                 n_layers: int = 9, filter_threshold: float = FILTER_THRESHOLD, guard: str = "flag", feature: str = "sift"):
        if not torch.cuda.is_available():
            raise _lib.GnError("PoseEngine needs a HIP device; the product path has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device)
        self.max_batch, self.precision = max_batch, precision
        self._n_layers, self._filter_threshold, self._state_dict = n_layers, filter_threshold, None
        self._guard = {"off": 0, "flag": 1, "sync": 2}[guard]
        self.feature = feature
        self._feature = {"sift": _lib.GN_FEATURE_SIFT, "superpoint": _lib.GN_FEATURE_SUPERPOINT}[feature]
        self.desc_dim = 128 if feature == "sift" else 256
        ctx = C.c_void_p()
        _lib.check(None, self.lib.gn_create_ex(device, max_batch, max_kpts, _PRECISIONS[precision], self._feature, C.byref(ctx)), "gn_create_ex")
        self.ctx = ctx
        self.kmax = self.lib.gn_kmax(ctx)
        _lib.check(ctx, self.lib.gn_set_num_layers(ctx, n_layers), "gn_set_num_layers")
        _lib.check(ctx, self.lib.gn_set_filter_threshold(ctx, filter_threshold), "gn_set_filter_threshold")
        _lib.check(ctx, self.lib.gn_set_guard(ctx, self._guard), "gn_set_guard")
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def guard_status(self):
        """(last matcher call left the fp16 range of the f16x2 mode, number of such calls so far) -- synchronises the stream."""
        last, total = C.c_int32(0), C.c_int64(0)
        _lib.check(self.ctx, self.lib.gn_get_guard_status(self.ctx, self._stream(), C.byref(last), C.byref(total)), "gn_get_guard_status")
        return bool(last.value), int(total.value)

    # ------------------------------------------------------------------ margin certificate (gn_set_certify)
    def set_certify(self, mode, eps: Optional[float] = None, eps_f32: Optional[float] = None) -> None:
        """"off" | "flag" | "rerun" (0 / 1 / 2).  "rerun": every match() / estimate() call synchronises once, and the pairs in which a decision
        lies within `eps` of flipping (or whose activations left the fp16 range) are run again on the exact-f32 kernels before the call
        returns -- correspondence indices are then the exact arithmetic's (pose_node.py:285-297 consumes them as exact integers).
        "deferred" (3; estimate() with sub-batch streams): the flags of call n are read -- and its flagged pairs re-run -- after call n + 1 has been
        enqueued, so the host never waits for an idle GPU.  Contract: the inputs AND outputs of call n stay alive and untouched until call n + 1 has
        returned or flush() was called (alternate two output dicts); results of call n are final from then on."""
        m = {"off": 0, "flag": 1, "rerun": 2, "deferred": 3}.get(mode, mode)
        self._certify_mode, self._last_out_ptr = int(m), None
        _lib.check(self.ctx, self.lib.gn_set_certify(self.ctx, int(m), -1.0 if eps is None else float(eps), -1.0 if eps_f32 is None else float(eps_f32)),
                   "gn_set_certify")

    def fused_projection_status(self) -> int:
        """gn_fused_projection_status: 1 the projection fused behind the block tail was checked bitwise equal to the separate launches on this context's
        weights, 0 it differed and was switched off, -1 not run yet / not applicable."""
        return int(self.lib.gn_fused_projection_status(self.ctx))

    def set_ffn_products(self, products) -> None:
        """gn_set_ffn_products: 3 (default, f32-accurate), 2 (activations' fp16 high term only; run it under set_certify), 1 (weights' high term only as
        well: W_h X_h), or "auto" (0): the level follows the certificate -- calibrate_certify then measures eps for all three levels (and for the rung below level 1, set_qkv_products), and under
        set_certify("rerun" / "deferred") the context runs on two products only while that flags (at most 1 pair in 64) no more pairs than three products
        would, and on one after two consecutive such windows for level 1.  Indices do not depend on the level."""
        p = 0 if products in ("auto", 0) else int(products)
        self._ffn_auto = p == 0
        _lib.check(self.ctx, self.lib.gn_set_ffn_products(self.ctx, p), "gn_set_ffn_products")

    def set_qkv_products(self, products) -> None:
        """gn_set_qkv_products: partial products of the attention input projections on bulk grids.  2: two (W_m X_h + W_h X_h), as before; 1: one (W_h X_h)
        wherever the block tail runs on level 1 and the bulk kernels are selected; "auto" (0, the default): a rung of the automatic ladder
        (set_ffn_products("auto")) below level 1 -- calibrate_certify measures its eps as a fourth arithmetic and a context on level 1 steps onto it after one
        clean window of 64 pairs.  set_ffn_products(1) alone never selects it."""
        p = 0 if products in ("auto", 0) else int(products)
        _lib.check(self.ctx, self.lib.gn_set_qkv_products(self.ctx, p), "gn_set_qkv_products")

    def set_qkv_level_eps(self, eps_projection: float) -> None:
        """gn_set_qkv_level_eps: the rung's eps as an earlier calibrate_certify measured it (after set_ffn_level_eps)."""
        _lib.check(self.ctx, self.lib.gn_set_qkv_level_eps(self.ctx, float(eps_projection)), "gn_set_qkv_level_eps")

    def set_ffn_level_eps(self, eps_two: float, eps_three: float, level: int = 3, eps_one: Optional[float] = None) -> None:
        """gn_set_ffn_level_eps (and gn_set_ffn_level_eps1): the levels' eps as an earlier calibrate_certify (same weights, same batch size) measured them, and
        the level to start on.  Without eps_one the one-product level keeps whatever eps it has; level=1 without any starts on two products."""
        if eps_one is not None:
            _lib.check(self.ctx, self.lib.gn_set_ffn_level_eps1(self.ctx, float(eps_one)), "gn_set_ffn_level_eps1")
        _lib.check(self.ctx, self.lib.gn_set_ffn_level_eps(self.ctx, float(eps_two), float(eps_three), int(level)), "gn_set_ffn_level_eps")

    def ffn_level(self) -> Dict[str, float]:
        """gn_get_ffn_level / gn_get_ffn_level1: the level the next call runs on, the calibrated eps of the three levels, and how many certified calls ran on each."""
        lvl, e2, e3, buf = C.c_int32(0), C.c_float(0.0), C.c_float(0.0), (C.c_int64 * 4)()
        _lib.check(self.ctx, self.lib.gn_get_ffn_level(self.ctx, C.byref(lvl), C.byref(e2), C.byref(e3), buf), "gn_get_ffn_level")
        e1, c1 = C.c_float(0.0), C.c_int64(0)
        _lib.check(self.ctx, self.lib.gn_get_ffn_level1(self.ctx, C.byref(e1), C.byref(c1)), "gn_get_ffn_level1")
        qs, qr, e0, c0 = C.c_int32(0), C.c_int32(0), C.c_float(0.0), C.c_int64(0)
        _lib.check(self.ctx, self.lib.gn_get_qkv_level(self.ctx, C.byref(qs), C.byref(qr), C.byref(e0), C.byref(c0)), "gn_get_qkv_level")
        # (the rung below level 1 -- one-product attention input projections -- keeps level == 1: "projection_one_product" says whether the next call runs on it;
        # calls_one_product counts the rung's calls too)
        return {"level": int(lvl.value), "eps_two_products": float(e2.value), "eps_three_products": float(e3.value), "eps_one_product": float(e1.value),
                "calls_two_products": int(buf[0]), "calls_three_products": int(buf[1]), "calls_one_product": int(c1.value),
                "switches": int(buf[2]), "automatic": bool(buf[3]),
                "eps_one_product_projection": float(e0.value), "calls_projection_one_product": int(c0.value), "projection_one_product": bool(qr.value),
                "qkv_products_setting": int(qs.value)}

    def calibrate_certify(self, inputs: dict, safety: float = 4.0, floor_eps: float = 1.0e-5) -> Dict[str, float]:
        """gn_calibrate_certify on staged inputs (the dict of stage_inputs / RecordStager.stage): measures max |P_mode - P_f32| over the deciding
        entries of the sample and sets eps = max(floor_eps, safety * that).  Returns {"measured": ..., "eps": ...}."""
        B = inputs["kpt_q"].shape[0]
        m, e = C.c_float(0.0), C.c_float(0.0)
        rc = self.lib.gn_calibrate_certify(self.ctx, B, inputs["kpt_format"],
                                           _ptr(inputs.get("desc_q")), _ptr(inputs["kpt_q"]), _ptr(inputs["n_q"]), inputs["kpt_q"].shape[1],
                                           _ptr(inputs.get("desc_r")), _ptr(inputs["kpt_r"]), _ptr(inputs["n_r"]), inputs["kpt_r"].shape[1],
                                           float(safety), float(floor_eps), C.byref(m), C.byref(e), self._stream())
        _lib.check(self.ctx, rc, "gn_calibrate_certify")
        lv = self.ffn_level()
        d = {"measured": float(m.value), "eps": float(e.value), "safety": float(safety)}
        if getattr(self, "_certify_ladder", False):      # set_certify_ladder(True): the middle level was measured too
            d["eps_mid"] = self.certify_ladder_stats()["eps_mid"]
        if getattr(self, "_ffn_auto", False):      # set_ffn_products("auto"): all three levels were measured; measured / eps are the three-product level's
            d["eps_two_products"], d["eps_three_products"] = lv["eps_two_products"], lv["eps_three_products"]
            d["eps_one_product"] = lv["eps_one_product"]
            d["eps_one_product_projection"] = lv["eps_one_product_projection"]      # (< 0: not measured -- set_qkv_products(2), or another precision mode)
        return d

    def set_certify_ladder(self, enable: bool, eps_mid: Optional[float] = None) -> None:
        """gn_set_certify_ladder: with the ladder on, set_certify("rerun" / "deferred") re-runs the pairs flagged for margin first in the
        "f16x2_f16x2_attn" arithmetic, certified there against eps_mid (measured by calibrate_certify while the ladder is on), and only the pairs still
        flagged in exact f32.  Contexts of "f16x2_bf16_attn" / "f16x2_f16_attn" only.  eps_mid=None keeps the current value."""
        _lib.check(self.ctx, self.lib.gn_set_certify_ladder(self.ctx, int(bool(enable)), -1.0 if eps_mid is None else float(eps_mid)),
                   "gn_set_certify_ladder")
        self._certify_ladder = bool(enable)

    def certify_ladder_stats(self) -> Dict[str, float]:
        """gn_get_certify_ladder_stats: pairs re-run on the middle level, of those certified there, of those passed on to exact f32 (since the last
        certify_stats(reset=True)), and eps_mid (None when not calibrated)."""
        buf = (C.c_int64 * 4)()
        _lib.check(self.ctx, self.lib.gn_get_certify_ladder_stats(self.ctx, buf), "gn_get_certify_ladder_stats")
        eps = None if buf[3] < 0 else struct.unpack("<f", struct.pack("<I", int(buf[3])))[0]
        return {"mid_rerun": int(buf[0]), "mid_certified": int(buf[1]), "passed_to_f32": int(buf[2]), "eps_mid": eps}

    def certify_stats(self, reset: bool = False) -> Dict[str, int]:
        buf = (C.c_int64 * 8)()
        _lib.check(self.ctx, self.lib.gn_get_certify_stats(self.ctx, buf), "gn_get_certify_stats")
        if reset:
            _lib.check(self.ctx, self.lib.gn_reset_certify_stats(self.ctx), "gn_reset_certify_stats")
        keys = ("calls", "pairs", "flagged_margin", "flagged_fp16_range", "rerun_pairs", "f32_marginal_pairs", "mode")
        d = {k: int(buf[i]) for i, k in enumerate(keys)}
        # where the eps in effect comes from; "discarded": measured on weights a load has since replaced (every pair goes to exact f32)
        d["eps_source"] = {0: "default", 1: "stated", 2: "calibrated", 3: "discarded"}.get(int(buf[7]), str(int(buf[7])))
        d["rerun_fraction"] = (d["rerun_pairs"] / d["pairs"]) if d["pairs"] else 0.0
        return d

    def uncertain(self, B: int) -> np.ndarray:
        """Per-pair flags of the most recent matcher call (0 certified, 1 margin, 2 fp16 range); synchronises the stream."""
        out = np.zeros(B, np.int32)
        _lib.check(self.ctx, self.lib.gn_get_uncertain(self.ctx, int(B), out.ctypes.data_as(_lib.c_i32p), self._stream()), "gn_get_uncertain")
        return out

    def __del__(self):
        ctx, self.ctx = getattr(self, "ctx", None), None
        if ctx:
            self.lib.gn_destroy(ctx)

    # ------------------------------------------------------------------ weights
    def grow(self, max_kpts: int) -> None:
        """Re-size the context for more keypoints per side (`gn_resize`: the workspaces are replaced, every weight, SuperPoint tensor and
        setting stays).  The reference accepts any keypoint count (cv2.SIFT_create() is unbounded, pose_node.py:122); the mirrors call this
        instead of failing on a larger cloud.  Costs a device synchronisation and a few allocations -- no weight reload (round 2 re-created
        the whole context: a multi-100 ms stall on the first large tile)."""
        if max_kpts <= self.kmax:
            return
        _lib.check(self.ctx, self.lib.gn_resize(self.ctx, int(max_kpts)), "gn_resize")
        self.kmax = self.lib.gn_kmax(self.ctx)
        self._sift = None

    # SuperPoint weights / arithmetic live in the context (gn_sp_*) and survive gn_resize
    def sp_set_arithmetic(self, mode: int) -> None:
        _lib.check(self.ctx, self.lib.gn_sp_set_arithmetic(self.ctx, int(mode)), "gn_sp_set_arithmetic")

    def sp_split_trips(self) -> int:
        """Passes of this context's SuperPoint extractor that the split-fp16 guard repeated on the exact f32 convolutions (an activation left fp16's
        range); read-only (gn_debug_read("sp_split_trips"))."""
        return int(self.debug_read("sp_split_trips", 1, dtype=np.int64)[0])

    def sp_load_state_dict(self, sd) -> None:
        for name, arr in sd.items():
            if hasattr(arr, "detach"):
                arr = arr.detach().cpu().numpy()
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*(arr.shape if arr.ndim else (1,)))
            rc = self.lib.gn_sp_load_tensor(self.ctx, name.encode(), arr.ctypes.data_as(C.c_void_p), shape, max(arr.ndim, 1))
            _lib.check(self.ctx, rc, f"gn_sp_load_tensor({name})")

    def load_state_dict(self, sd) -> None:
        self._state_dict = sd
        for name, arr in canonical_state_dict(sd).items():
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*(arr.shape if arr.ndim else (1,)))
            rc = self.lib.gn_load_tensor(self.ctx, name.encode(), arr.ctypes.data_as(C.c_void_p), shape, max(arr.ndim, 1))
            _lib.check(self.ctx, rc, f"gn_load_tensor({name})")
        missing = self.lib.gn_missing_tensors(self.ctx)
        if missing:
            raise _lib.GnError(f"{missing} required LightGlue tensors missing from the state dict")

    def set_image_size(self, wh_q=None, wh_r=None) -> None:
        """kornia LightGlueMatcher's hw1 / hw2 as (w, h): image sizes for the keypoint normalisation; None = keypoint extent (what
        PoseNode gets, pose_node.py:285-287)."""
        q, r = wh_q or (0.0, 0.0), wh_r or (0.0, 0.0)
        _lib.check(self.ctx, self.lib.gn_set_image_size(self.ctx, float(q[0]), float(q[1]), float(r[0]), float(r[1])), "gn_set_image_size")

    def set_distortion(self, d) -> None:
        """cv2.solvePnPRansac's distCoeffs for the PnP stage of pnp_ransac / estimate / vo_estimate (gn_set_distortion): 4 or 5 plumb-bob
        coefficients (k1, k2, p1, p2[, k3]); None, an empty sequence or all zeros switch it off (the default).  Sticky, captured per call."""
        a = np.zeros(0, np.float64) if d is None else np.ascontiguousarray(np.asarray(d, np.float64).reshape(-1))
        rc = self.lib.gn_set_distortion(self.ctx, a.ctypes.data_as(_lib.c_f64p) if a.size else None, int(a.size))
        _lib.check(self.ctx, rc, "gn_set_distortion")

    def distortion(self) -> Optional[np.ndarray]:
        """The five coefficients in effect (gn_get_distortion), or None when distortion is off."""
        d = np.zeros(5, np.float64)
        rc = self.lib.gn_get_distortion(self.ctx, d.ctypes.data_as(_lib.c_f64p))
        _lib.check(self.ctx, rc, "gn_get_distortion")
        return d if rc == 1 else None

    def pair_cameras(self, K, d=None) -> Tuple[torch.Tensor, int]:
        """A per-pair camera table for estimate / vo_estimate / pnp_ransac / undistort_points (`cameras=`, `camera_model=`; gn_set_pair_cameras):
        K (B, 3, 3), d None or (B, 4 | 5) plumb-bob coefficients -> (cams (B, 9) f64 on the device, model); model = 1 iff d is given.  Checked on
        the host first (check_pair_cameras), uploaded through the pinned staging, and the caller's own tensor (a later table does not alias it)."""
        rows = check_pair_cameras(K, d)
        return self.to_device("pair_cameras", rows, torch.float64).clone(), (0 if d is None else 1)

    @contextlib.contextmanager
    def _camera_table(self, cameras, camera_model, B: int, K):
        """The table in charge for the C call inside (host-side state only: set before, off after).  None: nothing is touched."""
        if cameras is None:
            if K is None:
                raise ValueError("K is required without a cameras table")
            yield
            return
        check_camera_table(cameras, camera_model, B)
        _lib.check(self.ctx, self.lib.gn_set_pair_cameras(self.ctx, _ptr(cameras), int(B), int(camera_model)), "gn_set_pair_cameras")
        try:
            yield
        finally:
            self.lib.gn_set_pair_cameras(self.ctx, None, 0, 0)

    def set_ransac(self, iterations: int = RANSAC_ITERATIONS, reproj_px: float = RANSAC_REPROJ_PX, confidence: float = RANSAC_CONFIDENCE) -> None:
        """cv2.solvePnPRansac's iterationsCount / reprojectionError / confidence for the PnP stage inside estimate / vo_estimate and the
        certificate's re-runs (gn_set_ransac): 1 .. 4096 hypotheses.  Sticky, captured per call; the default is the reference's (10, 8.0, 0.99).
        pnp_ransac / pnp_ransac_host take theirs as arguments."""
        iterations = check_ransac_iterations(iterations)
        _lib.check(self.ctx, self.lib.gn_set_ransac(self.ctx, iterations, float(reproj_px), float(confidence)), "gn_set_ransac")

    def ransac(self) -> Tuple[int, float, float]:
        """(iterations, reproj_px, confidence) in effect (gn_get_ransac)."""
        it, px, conf = C.c_int(0), C.c_float(0.0), C.c_double(0.0)
        _lib.check(self.ctx, self.lib.gn_get_ransac(self.ctx, C.byref(it), C.byref(px), C.byref(conf)), "gn_get_ransac")
        return int(it.value), float(px.value), float(conf.value)

    # set_dem_format: (scale, offset, nodata) for the calls to come -- the element type is each call's dem.dtype -- and what the context
    # holds right now (gn_set_dem_format's default until a call needs another)
    _dem_fmt = (1.0, 0.0, None)
    _dem_applied = (_lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0)

    def set_dem_format(self, scale: float = 1.0, offset: float = 0.0, nodata=None) -> None:
        """Elevation rasters beyond 8 bits (gn_set_dem_format): z = (float)(raw * scale + offset) for the `dem` of estimate / estimate_bucketed /
        estimate_images / gather_points, and `nodata` = the raw value of a void cell (None: no voids; NaN: the non-finite cells of a float32
        raster alone).  A match on a void cell is removed before PnP and the outputs describe the shorter list.  The element type is taken from
        the dtype of each call's `dem` tensor (uint8 / uint16 / int16 / float32; ValueError otherwise, and for a nodata the type cannot hold).
        Sticky, captured per call; the default (1, 0, None) with a uint8 raster computes bit for bit what it always did."""
        check_dem_format(np.float32, scale, offset, None if nodata is None else float("nan"))      # (nodata against the type: per call)
        if nodata is not None and (isinstance(nodata, bool) or not isinstance(nodata, (int, float, np.integer, np.floating))):
            raise TypeError(f"dem_nodata must be a number or None, got {type(nodata).__name__}")
        self._dem_fmt = (float(scale), float(offset), None if nodata is None else float(nodata))

    def dem_format(self) -> Tuple[float, float, Optional[float]]:
        """(scale, offset, nodata) in effect (set_dem_format)."""
        return self._dem_fmt

    def _apply_dem_format(self, dem) -> None:
        """The context's DEM format for a call with raster `dem` (None: nothing to lift)."""
        if dem is None:
            return
        fmt = check_dem_format(dem.dtype, *self._dem_fmt)
        same = fmt[:4] == self._dem_applied[:4] and (fmt[4] == self._dem_applied[4] or (fmt[4] != fmt[4] and self._dem_applied[4] != self._dem_applied[4]))
        if not same:
            _lib.check(self.ctx, self.lib.gn_set_dem_format(self.ctx, *fmt), "gn_set_dem_format")
            self._dem_applied = fmt

    def dem_last_dropped(self, B: int) -> np.ndarray:
        """Matches removed as void from pairs 0 .. B-1 of the most recent call that ran with a void value (gn_dem_last_dropped); [B] int32.
        Synchronises the device."""
        dropped = np.zeros(int(B), np.int32)
        rc = self.lib.gn_dem_last_dropped(self.ctx, int(B), dropped.ctypes.data_as(_lib.c_i32p), self._stream())
        _lib.check(self.ctx, rc, "gn_dem_last_dropped")
        return dropped

    def ransac_last_counts(self, B: int) -> Tuple[np.ndarray, np.ndarray]:
        """Per pair of the most recent PnP stage: (final adapted iteration count, hypotheses actually evaluated), int32 [B] each
        (gn_ransac_last_counts).  Synchronises the device."""
        niters, evaluated = np.zeros(B, np.int32), np.zeros(B, np.int32)
        rc = self.lib.gn_ransac_last_counts(self.ctx, int(B), niters.ctypes.data_as(_lib.c_i32p), evaluated.ctypes.data_as(_lib.c_i32p), self._stream())
        _lib.check(self.ctx, rc, "gn_ransac_last_counts")
        return niters, evaluated

    def undistort_points(self, img, n_pts, K: Optional[np.ndarray] = None, to_pixels: bool = False, out: Optional[torch.Tensor] = None,
                         cameras: Optional[torch.Tensor] = None, camera_model: int = 0) -> torch.Tensor:
        """cv2.undistortPoints with this engine's coefficients (gn_undistort_points).  img [B,S,2] f32 pixels, n_pts [B] i32 (device) ->
        [B,S,2] f32: normalised coordinates, or pixels again with to_pixels (cv2's P = K).  Slots past n_pts keep what `out` held (zeros
        when it is allocated here).  cameras / camera_model (pair_cameras): row b for point list b instead of K and the engine's coefficients."""
        B, S = img.shape[0], img.shape[1]
        with self._camera_table(cameras, camera_model, B, K):
            if out is None:
                out = torch.zeros((B, S, 2), dtype=torch.float32, device=self.device)
            rc = self.lib.gn_undistort_points(self.ctx, B, _ptr(img), _ptr(n_pts), S, _k9_ptr(K), int(bool(to_pixels)),
                                              _ptr(out), self._stream())
            _lib.check(self.ctx, rc, "gn_undistort_points")
        return out

    def set_num_layers(self, n: int) -> None:
        self._n_layers = n
        _lib.check(self.ctx, self.lib.gn_set_num_layers(self.ctx, n), "gn_set_num_layers")

    # ------------------------------------------------------------------ point pruning (gn_set_width_pruning)
    def set_width_pruning(self, width_confidence: float, min_kpts: Optional[int] = None) -> None:
        """kornia's width_confidence with early exit off: after every layer but the last, a side that still holds more than `min_kpts` keypoints
        (None: 1536, recalled from kornia's pruning_keypoint_thresholds) keeps those with sigmoid(matchability) > 1 - width_confidence; the rest of
        the call runs on what is left and the match indices stay ORIGINAL keypoint indices.  <= 0 switches it off (the default).  Refused (GnError)
        while the margin certificate is on, and for width_confidence >= 1 or not finite."""
        check_width_pruning(width_confidence, min_kpts)
        rc = self.lib.gn_set_width_pruning(self.ctx, float(width_confidence), -1 if min_kpts is None else int(min_kpts))
        _lib.check(self.ctx, rc, "gn_set_width_pruning")

    def width_pruning(self) -> Tuple[float, int]:
        """(width_confidence, min_kpts) in effect; width_confidence is -1.0 when pruning is off."""
        w, m = C.c_float(0.0), C.c_int(0)
        _lib.check(self.ctx, self.lib.gn_get_width_pruning(self.ctx, C.byref(w), C.byref(m)), "gn_get_width_pruning")
        return float(w.value), int(m.value)

    def last_prune(self, B: int) -> Tuple[np.ndarray, np.ndarray]:
        """kornia's (prune0, prune1) of the most recent matcher call, int32 [B, kmax] each (gn_get_prune): the number of layers every original
        keypoint took part in -- n_layers everywhere with pruning off, 1 where pruning is on and never fired, 0 past a side's count.
        Synchronises the device."""
        p0, p1 = np.zeros((B, self.kmax), np.int32), np.zeros((B, self.kmax), np.int32)
        _lib.check(self.ctx, self.lib.gn_get_prune(self.ctx, int(B), p0.ctypes.data_as(_lib.c_i32p), p1.ctypes.data_as(_lib.c_i32p)), "gn_get_prune")
        return p0, p1

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def stage_inputs(self, pairs, kpt_format: int = _lib.GN_KPT_XYSA):
        """Pack a list of `synthetic.Pair`-like objects into device tensors (host -> HBM once)."""
        B = len(pairs)
        nq = max(len(p.kp_q) for p in pairs)
        nr = max(len(p.kp_r) for p in pairs)
        D = self.desc_dim
        dq = np.zeros((B, nq, D), np.float32); kq = np.zeros((B, nq, 4), np.float32)
        dr = np.zeros((B, nr, D), np.float32); kr = np.zeros((B, nr, 4), np.float32)
        n_q = np.zeros(B, np.int32); n_r = np.zeros(B, np.int32)
        h, w = pairs[0].dem.shape
        dem = np.zeros((B, h, w), np.dtype(dem_dtype_name(pairs[0].dem.dtype)))
        for b, p in enumerate(pairs):
            a, c = len(p.kp_q), len(p.kp_r)
            n_q[b], n_r[b] = a, c
            dq[b, :a], dr[b, :c] = p.desc_q, p.desc_r
            kq[b, :a] = np.column_stack([p.kp_q, p.size_q, p.angle_q])
            kr[b, :c] = np.column_stack([p.kp_r, p.size_r, p.angle_r])
            dem[b] = p.dem
        f = lambda a, dt: _dev_tensor(a, dt, self.device)  # noqa: E731
        return dict(desc_q=f(dq, torch.float32), kpt_q=f(kq, torch.float32), n_q=f(n_q, torch.int32),
                    desc_r=f(dr, torch.float32), kpt_r=f(kr, torch.float32), n_r=f(n_r, torch.int32),
                    dem=f(dem, None), kpt_format=kpt_format)

    # ------------------------------------------------------------------ hot path
    def match(self, desc_q, kpt_q, n_q, desc_r, kpt_r, n_r, kpt_format: int = _lib.GN_KPT_XYSA,
              out: Optional[tuple] = None):
        """gn_match.  Tensors are device tensors: desc [B,S,128] f32, kpt [B,S,4|6] f32, n [B] i32.
        Returns (idx [B,kmax,2] i64, score [B,kmax] f32, n_match [B] i32) on the device."""
        B = kpt_q.shape[0]
        if out is None:
            idx = torch.empty((B, self.kmax, 2), dtype=torch.int64, device=self.device)
            score = torch.empty((B, self.kmax), dtype=torch.float32, device=self.device)
            n_match = torch.empty((B,), dtype=torch.int32, device=self.device)
        else:
            idx, score, n_match = out
        rc = self.lib.gn_match(self.ctx, B, kpt_format, _ptr(desc_q), _ptr(kpt_q), _ptr(n_q), kpt_q.shape[1],
                               _ptr(desc_r), _ptr(kpt_r), _ptr(n_r), kpt_r.shape[1],
                               _ptr(idx), _ptr(score), _ptr(n_match), self._stream())
        _lib.check(self.ctx, rc, "gn_match")
        return idx, score, n_match

    def gather_points(self, kpt_q, kpt_r, idx, n_match, dem, kpt_format: int = _lib.GN_KPT_XYSA, score=None):
        """gn_gather_points: (mkp_q [B,kmax,2], obj [B,kmax,3]) of the match list idx / n_match, the reference side lifted with `dem` under
        set_dem_format.  With a void value set, idx, n_match and `score` (optional [B,kmax] f32: gn_gather_points_scored) are compacted in
        place to the matches on valid cells."""
        B = kpt_q.shape[0]
        self._apply_dem_format(dem)
        mkp_q = torch.zeros((B, self.kmax, 2), dtype=torch.float32, device=self.device)
        obj = torch.zeros((B, self.kmax, 3), dtype=torch.float32, device=self.device)
        H, W = (dem.shape[1], dem.shape[2]) if dem is not None else (0, 0)
        if score is not None:
            rc = self.lib.gn_gather_points_scored(self.ctx, B, kpt_format, _ptr(kpt_q), kpt_q.shape[1], _ptr(kpt_r), kpt_r.shape[1],
                                                  _ptr(idx), _ptr(score), _ptr(n_match), _ptr(dem), H, W, _ptr(mkp_q), _ptr(obj), self._stream())
        else:
            rc = self.lib.gn_gather_points(self.ctx, B, kpt_format, _ptr(kpt_q), kpt_q.shape[1], _ptr(kpt_r), kpt_r.shape[1],
                                           _ptr(idx), _ptr(n_match), _ptr(dem), H, W, _ptr(mkp_q), _ptr(obj), self._stream())
        _lib.check(self.ctx, rc, "gn_gather_points_scored" if score is not None else "gn_gather_points")
        return mkp_q, obj

    def _alloc_cov(self, B: int) -> dict:
        d = self.device
        return dict(cov=torch.empty((B, 6, 6), dtype=torch.float64, device=d), sigma=torch.empty((B,), dtype=torch.float64, device=d),
                    cov_ok=torch.empty((B,), dtype=torch.uint8, device=d))

    def _alloc_report(self, B: int, stride: int, matches: bool = False) -> dict:
        d = self.device
        out = dict(inlier_mask=torch.empty((B, stride), dtype=torch.uint8, device=d), inlier_idx=torch.empty((B, stride), dtype=torch.int32, device=d),
                   reproj_err=torch.empty((B, stride), dtype=torch.float32, device=d))
        if matches:
            out.update(idx=torch.empty((B, stride, 2), dtype=torch.int64, device=d), score=torch.empty((B, stride), dtype=torch.float32, device=d))
        return out

    def pnp_ransac(self, obj, img, n_pts, K: np.ndarray, iterations: int = RANSAC_ITERATIONS,
                   reproj_px: float = RANSAC_REPROJ_PX, confidence: float = RANSAC_CONFIDENCE, min_pts: int = 5,
                   covariance: bool = False, sigma_px: float = 0.0, report: bool = False, report_out: Optional[dict] = None,
                   cameras: Optional[torch.Tensor] = None, camera_model: int = 0):
        """gn_pnp_ransac.  obj [B,S,3] f32, img [B,S,2] f32, n_pts [B] i32 (device).  Returns (R, t, n_inliers, ok); with covariance=True
        (gn_pnp_ransac_cov) also cov [B,6,6] f64 of (rvec, tvec), sigma [B] f64 (a-posteriori pixel sigma) and cov_ok [B] u8.  sigma_px > 0
        states the pixel noise; 0 scales the covariance with the residuals' own sigma.  report=True (gn_pnp_ransac_report) appends
        inlier_mask [B,S] u8, inlier_idx [B,S] i32 (cv2's `inliers`: the first n_inliers entries, then -1) and reproj_err [B,S] f32 (pixels at
        the returned pose, -1 past n_pts and where ok = 0); report_out: a dict of those three to write into instead of fresh tensors.
        cameras / camera_model (pair_cameras): pair b is solved with row b instead of K (which may then be None) and the engine's coefficients."""
        B = obj.shape[0]
        with self._camera_table(cameras, camera_model, B, K):
            return self._pnp_ransac(obj, img, n_pts, K, iterations, reproj_px, confidence, min_pts, covariance, sigma_px, report, report_out)

    def _pnp_ransac(self, obj, img, n_pts, K, iterations, reproj_px, confidence, min_pts, covariance, sigma_px, report, report_out):
        B = obj.shape[0]
        if report:
            R = torch.empty((B, 3, 3), dtype=torch.float64, device=self.device)
            t = torch.empty((B, 3, 1), dtype=torch.float64, device=self.device)
            n_inl = torch.empty((B,), dtype=torch.int32, device=self.device)
            ok = torch.empty((B,), dtype=torch.uint8, device=self.device)
            K9 = _k9_ptr(K)
            c = self._alloc_cov(B) if covariance else {}
            r = report_out if report_out is not None else self._alloc_report(B, obj.shape[1])
            rc = self.lib.gn_pnp_ransac_report(self.ctx, B, _ptr(obj), _ptr(img), _ptr(n_pts), obj.shape[1],
                                               K9, iterations, reproj_px, confidence, min_pts,
                                               _ptr(R), _ptr(t), _ptr(n_inl), _ptr(ok), float(sigma_px), _ptr(c.get("cov")), _ptr(c.get("sigma")), _ptr(c.get("cov_ok")),
                                               _ptr(r.get("inlier_mask")), _ptr(r.get("inlier_idx")), _ptr(r.get("reproj_err")), self._stream())
            _lib.check(self.ctx, rc, "gn_pnp_ransac_report")
            res = (R, t, n_inl, ok) + ((c["cov"], c["sigma"], c["cov_ok"]) if covariance else ())
            return res + (r.get("inlier_mask"), r.get("inlier_idx"), r.get("reproj_err"))
        R = torch.empty((B, 3, 3), dtype=torch.float64, device=self.device)
        t = torch.empty((B, 3, 1), dtype=torch.float64, device=self.device)
        n_inl = torch.empty((B,), dtype=torch.int32, device=self.device)
        ok = torch.empty((B,), dtype=torch.uint8, device=self.device)
        K9 = _k9_ptr(K)
        if covariance:
            c = self._alloc_cov(B)
            rc = self.lib.gn_pnp_ransac_cov(self.ctx, B, _ptr(obj), _ptr(img), _ptr(n_pts), obj.shape[1],
                                            K9, iterations, reproj_px, confidence, min_pts,
                                            _ptr(R), _ptr(t), _ptr(n_inl), _ptr(ok), float(sigma_px), _ptr(c["cov"]), _ptr(c["sigma"]), _ptr(c["cov_ok"]),
                                            self._stream())
            _lib.check(self.ctx, rc, "gn_pnp_ransac_cov")
            return R, t, n_inl, ok, c["cov"], c["sigma"], c["cov_ok"]
        rc = self.lib.gn_pnp_ransac(self.ctx, B, _ptr(obj), _ptr(img), _ptr(n_pts), obj.shape[1],
                                    K9, iterations, reproj_px, confidence, min_pts,
                                    _ptr(R), _ptr(t), _ptr(n_inl), _ptr(ok), self._stream())
        _lib.check(self.ctx, rc, "gn_pnp_ransac")
        return R, t, n_inl, ok

    def to_device(self, name: str, array, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """Host array -> device tensor through this engine's pinned staging (gisnav_amd.upload.PinnedUploader); a device tensor passes through."""
        if isinstance(array, torch.Tensor):
            return array
        if getattr(self, "_uploader", None) is None:
            from .upload import PinnedUploader
            self._uploader = PinnedUploader(self.device)
        return self._uploader(name, array, dtype)

    def to_host(self, *tensors: torch.Tensor):
        """Small device tensors -> numpy copies through one pinned block and one synchronisation (gisnav_amd.upload.PinnedDownloader)."""
        if getattr(self, "_downloader", None) is None:
            from .upload import PinnedDownloader
            self._downloader = PinnedDownloader(self.device)
        return self._downloader(*tensors)

    def pnp_ransac_host(self, obj: np.ndarray, img: np.ndarray, K: np.ndarray, iterations: int = RANSAC_ITERATIONS,
                        reproj_px: float = RANSAC_REPROJ_PX, confidence: float = RANSAC_CONFIDENCE, min_pts: int = 5,
                        covariance: bool = False, sigma_px: float = 0.0, dist=None, report: bool = False):
        """gn_pnp_ransac for ONE correspondence list given as host arrays (seam B2): obj (n, 3), img (n, 2) -> (R (3,3) f64, t (3,1) f64, n_inliers, ok)
        as host values.  One pinned staging block in ([n | pad | obj | img], one asynchronous copy), one 416-byte block out: pageable transfers of
        this size were measured to stall for ~90 ms every few dozen calls on the MI355X boxes (tools/bench_seams.py), pinned ones never.
        covariance=True (gn_pnp_ransac_cov) appends (cov (6,6) f64, sigma, cov_ok) to the result.  dist: distCoeffs for this call alone
        (set_distortion around it, the engine's own state restored afterwards); None leaves the engine's state in charge.  report=True
        (gn_pnp_ransac_report) appends (inliers (n_inliers, 1) int32 as cv2 returns them, reproj_err (n,) f32) -- the output block grows by 8 n
        bytes, and only then."""
        if dist is not None:
            keep = self.distortion()
            self.set_distortion(dist)
            try:
                return self.pnp_ransac_host(obj, img, K, iterations, reproj_px, confidence, min_pts, covariance, sigma_px, report=report)
            finally:
                self.set_distortion(keep)
        n = int(len(obj))
        if n > self.kmax:
            raise _lib.GnError(f"{n} correspondences exceed this context's max_kpts {self.kmax}")
        io = getattr(self, "_pnp_io", None)
        if io is None or io["cap"] != self.kmax:
            cap = self.kmax
            pin = torch.empty(8 + 5 * cap, dtype=torch.float32, pin_memory=True)
            # R 72 | t 24 | pad 4 | n_inliers 4 | ok 1 | pad 7 | cov 288 | sigma 8 | cov_ok 1 (+ pad) | report: inlier_idx 4 n | reproj_err 4 n
            out = torch.zeros(416 + 8 * cap, dtype=torch.uint8, device=self.device)
            io = self._pnp_io = dict(cap=cap, pin=pin, pin_np=pin.numpy(), dev=torch.empty(8 + 5 * cap, dtype=torch.float32, device=self.device), out=out,
                                     host=torch.empty(416 + 8 * cap, dtype=torch.uint8, pin_memory=True))
            io["host_np"] = io["host"].numpy()
        h = io["pin_np"]
        h[:1].view(np.int32)[0] = n
        i0 = 4 + (3 * n + 3) // 4 * 4                       # the image points start on a 16-byte boundary, like the object points
        h[4:4 + 3 * n] = np.asarray(obj, np.float32).reshape(-1)
        h[i0:i0 + 2 * n] = np.asarray(img, np.float32).reshape(-1)
        d, o = io["dev"], io["out"]
        d[:i0 + 2 * n].copy_(io["pin"][:i0 + 2 * n], non_blocking=True)
        K9 = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        args = (self.ctx, 1, _ptr(d[4:4 + 3 * n]), _ptr(d[i0:i0 + 2 * n]), _ptr(d[:1].view(torch.int32)), n,
                K9.ctypes.data_as(_lib.c_f64p), iterations, reproj_px, confidence, min_pts,
                _ptr(o[0:72]), _ptr(o[72:96]), _ptr(o[100:104]), _ptr(o[104:105]))
        cov3 = (_ptr(o[112:400]), _ptr(o[400:408]), _ptr(o[408:409])) if covariance else (None, None, None)
        if report:
            rc = self.lib.gn_pnp_ransac_report(*args, float(sigma_px), *cov3, None, _ptr(o[416:416 + 4 * n]), _ptr(o[416 + 4 * n:416 + 8 * n]), self._stream())
        elif covariance:
            rc = self.lib.gn_pnp_ransac_cov(*args, float(sigma_px), *cov3, self._stream())
        else:
            rc = self.lib.gn_pnp_ransac(*args, self._stream())
        _lib.check(self.ctx, rc, "gn_pnp_ransac_report" if report else "gn_pnp_ransac_cov" if covariance else "gn_pnp_ransac")
        nb = 416 + 8 * n if report else 416 if covariance else 112
        io["host"][:nb].copy_(o[:nb], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        r = io["host_np"]
        res = (r[0:72].view(np.float64).reshape(3, 3).copy(), r[72:96].view(np.float64).reshape(3, 1).copy(), int(r[100:104].view(np.int32)[0]), bool(r[104]))
        if covariance:
            res += (r[112:400].view(np.float64).reshape(6, 6).copy(), float(r[400:408].view(np.float64)[0]), bool(r[408]))
        if report:
            ninl = res[2] if res[3] else 0
            res += (r[416:416 + 4 * n].view(np.int32)[:ninl].reshape(-1, 1).copy(), r[416 + 4 * n:416 + 8 * n].view(np.float32).copy())
        return res

    def set_ragged(self, ragged: Optional[bool]) -> None:
        """Override of a choice the library makes by itself.  The big kernels skip tiles that hold only padding either way; the block tail has two
        forms (one workgroup per tile, or one per CU walking the list of non-empty tiles: ~20 % faster on batches whose keypoint counts differ a lot --
        an unbounded cv2.SIFT_create(), pose_node.py:122 --, 3 % slower per launch on batches without padding; identical bits).  By default
        (`None`) the library picks the form per call from the fraction of padding-only tiles its previous call saw; True / False force one."""
        _lib.check(self.ctx, self.lib.gn_debug_set_variant(self.ctx, 31, 1 if ragged is None else 2 if ragged else 3), "gn_debug_set_variant(31)")

    def set_overlap(self, enable: bool) -> None:
        """Batch-serving option: PnP of call n overlaps the matcher of call n+1 (see gn_set_overlap); call flush()
        before reading R / t / n_inliers / ok."""
        _lib.check(self.ctx, self.lib.gn_set_overlap(self.ctx, int(enable)), "gn_set_overlap")

    def set_substreams(self, n: int, deferred_join: bool = False) -> None:
        """Throughput option: every estimate() call runs its pairs as n groups on internal streams (gn_set_substreams).  With
        deferred_join the groups are only joined by flush(): keep the input tensors of a call alive until then."""
        _lib.check(self.ctx, self.lib.gn_set_substreams(self.ctx, int(n)), "gn_set_substreams")
        _lib.check(self.ctx, self.lib.gn_set_deferred_join(self.ctx, int(bool(deferred_join))), "gn_set_deferred_join")

    def set_active_kpts(self, max_kpts_per_side: int) -> int:
        """Padded keypoint count the following match()/estimate() calls run at (gn_set_active_kpts): pass the largest keypoint
        count of the batch when it is well below max_kpts.  Returns the padded size in effect."""
        rc = self.lib.gn_set_active_kpts(self.ctx, int(max_kpts_per_side))
        if rc < 0:
            _lib.check(self.ctx, rc, "gn_set_active_kpts")
        return rc

    def flush(self) -> None:
        _lib.check(self.ctx, self.lib.gn_flush(self.ctx, self._stream()), "gn_flush")
        self._last_out_ptr = None

    def _report_ptrs(self, out: dict):
        return tuple(_ptr(out.get(k)) for k in ("idx", "score", "inlier_mask", "inlier_idx", "reproj_err"))

    def estimate(self, inputs: dict, K: np.ndarray, min_matches: int = MIN_MATCHES, out: Optional[dict] = None,
                 covariance: bool = False, sigma_px: float = 0.0, report: bool = False):
        """gn_estimate on staged inputs: PoseNode._pose lines 246-308 for the whole batch.  covariance=True (gn_estimate_cov): `out` also
        carries cov [B,6,6], sigma [B], cov_ok [B] (alloc_outputs(B, covariance=True)), complete when R / t / ok are.  report=True
        (gn_estimate_report): `out` also carries the match list idx [B,kmax,2], score [B,kmax] and inlier_mask / inlier_idx / reproj_err
        [B,kmax] of its rows (alloc_outputs(B, report=True)), complete when R / t / ok are.
        inputs["cameras"] / inputs["camera_model"] (pair_cameras): pair b's PnP runs with row b instead of K (which may then be None) and
        the engine's coefficients; the table is an input like the others (keep it alive as long as them)."""
        B = inputs["kpt_q"].shape[0]
        with self._camera_table(inputs.get("cameras"), inputs.get("camera_model", 0), B, K):
            return self._estimate(inputs, K, min_matches, out, covariance, sigma_px, report)

    def _estimate(self, inputs, K, min_matches, out, covariance, sigma_px, report):
        B = inputs["kpt_q"].shape[0]
        if out is None:
            out = self.alloc_outputs(B, covariance, report)
        if getattr(self, "_certify_mode", 0) == 3:
            if self._last_out_ptr == out["R"].data_ptr():
                raise _lib.GnError("deferred certificate: this call would write the outputs of the previous call, whose flagged pairs may still be re-run -- "
                                   "alternate two output dicts, or flush() between the calls")
            self._last_out_ptr = out["R"].data_ptr()
        dem = inputs.get("dem")
        self._apply_dem_format(dem)
        H, W = (dem.shape[1], dem.shape[2]) if dem is not None else (0, 0)
        K9 = _k9_ptr(K)
        # (GN_KPT_RECORD inputs carry the descriptors inside the keypoint records: desc_q / desc_r are None)
        args = (self.ctx, B, inputs["kpt_format"],
                _ptr(inputs.get("desc_q")), _ptr(inputs["kpt_q"]), _ptr(inputs["n_q"]), inputs["kpt_q"].shape[1],
                _ptr(inputs.get("desc_r")), _ptr(inputs["kpt_r"]), _ptr(inputs["n_r"]), inputs["kpt_r"].shape[1],
                _ptr(dem), H, W, K9, min_matches,
                _ptr(out["R"]), _ptr(out["t"]), _ptr(out["n_match"]), _ptr(out["n_inliers"]), _ptr(out["ok"]))
        if report:
            cov3 = (_ptr(out["cov"]), _ptr(out["sigma"]), _ptr(out["cov_ok"])) if covariance else (None, None, None)
            rc = self.lib.gn_estimate_report(*args, float(sigma_px), *cov3, *self._report_ptrs(out), self._stream())
        elif covariance:
            rc = self.lib.gn_estimate_cov(*args, float(sigma_px), _ptr(out["cov"]), _ptr(out["sigma"]), _ptr(out["cov_ok"]), self._stream())
        else:
            rc = self.lib.gn_estimate(*args, self._stream())
        _lib.check(self.ctx, rc, "gn_estimate_report" if report else "gn_estimate_cov" if covariance else "gn_estimate")
        return out

    def estimate_bucketed(self, inputs: dict, K: np.ndarray, n_q_host, n_r_host, bucket_pairs: int = 8, min_matches: int = MIN_MATCHES,
                          out: Optional[dict] = None, report: bool = False):
        """Length-bucketing scheduler for ragged batches: `cv2.SIFT_create()` is unbounded (pose_node.py:122), so the keypoint counts of a
        batch of messages spread widely, and one gn_estimate call pads every pair to the batch maximum (attention cost grows with the
        SQUARE of the padded length).  The pairs are sorted by max(n_q, n_r) (host-side counts: no device read), run as groups of
        `bucket_pairs` consecutive pairs each padded to ITS maximum (gn_set_active_kpts), and the results are returned in the caller's
        order.  Padding slots are never read, and within one kernel family results are the same bits whatever the padding; calls of one or two
        pairs choose their family by pair count alone, so they never depend on it.  A call of more pairs chooses by its number of 128-token tiles
        and workgroups (k_qkv from 128 tiles, k_ffn128 from 256, k_attn_pw at multiples of 256 slots): there the padded size can change the family,
        and with it the result at rounding level -- within the mode's fp64 budgets, not the same bits (tests/test_gpu_fp64_padded_sizes.py,
        DESIGN 11.7).  Results depend in the same way on the number of pairs per call: calls of one or
        two pairs (and sub-stream groups of that size) run the small-grid kernel family, whose summation order differs from the bulk kernels' -- a
        remainder bucket of one or two pairs therefore gives the same matches and poses up to rounding, not the same bits, as one padded call
        (tests/test_gpu_round6.py).  With the certificate on (set_certify) the correspondence indices are the exact arithmetic's either
        way.  report=True: every bucket runs gn_estimate_report, and the match lists and reports come back in the caller's order with the rest.
        Returns (out, stats)."""
        n_q_host = np.asarray(n_q_host).astype(np.int64)
        n_r_host = np.asarray(n_r_host).astype(np.int64)
        B = len(n_q_host)
        if out is None:
            out = self.alloc_outputs(B, report=report)
        need = np.maximum(np.maximum(n_q_host, n_r_host), 1)
        order = np.argsort(-need, kind="stable")
        perm = torch.as_tensor(order, device=self.device)
        # (a uint16 raster is permuted through its int16 view: the same bytes, and an index kernel every torch build has)
        pick = lambda v: v.view(torch.int16).index_select(0, perm).view(torch.uint16) if v.dtype == torch.uint16 else v.index_select(0, perm)  # noqa: E731
        srt = {k: (pick(v) if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}
        tmp = self.alloc_outputs(B, report=report)
        pad_tokens = 0
        try:
            for a in range(0, B, bucket_pairs):
                b = min(B, a + bucket_pairs)
                pad = self.set_active_kpts(int(need[order[a:b]].max()))
                pad_tokens += 2 * pad * (b - a)
                grp = {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in srt.items()}
                self.estimate(grp, K, min_matches, out={k: v[a:b] for k, v in tmp.items()}, report=report)
        finally:
            self.set_active_kpts(self.kmax)
        # with set_overlap / set_substreams(deferred_join=True) the PnP stage or the groups may still run on the library's internal streams:
        # join them before `tmp` is read on the caller's stream and before the index_select'ed copies in `srt` are released
        self.flush()
        for k in out:
            out[k].index_copy_(0, perm, tmp[k])
        real = int((n_q_host + n_r_host).sum())
        one_call_pad = 2 * B * (((int(need.max()) + 127) // 128) * 128)
        return out, {"real_tokens": real, "padded_tokens_bucketed": int(pad_tokens), "padded_tokens_one_call": int(one_call_pad),
                     "groups": (B + bucket_pairs - 1) // bucket_pairs}

    def estimate_images(self, frames, tiles, K: np.ndarray, dem=None, sift=None, min_matches: int = MIN_MATCHES, out: Optional[dict] = None,
                        report: bool = False, cameras: Optional[torch.Tensor] = None, camera_model: int = 0):
        """Frames -> pose from pixels for B pairs, everything in HBM: one batched SIFT pass over the B camera frames and the
        B map tiles (`gn_sift_detect_and_compute_batch`), the matcher padded to what the batch needs (`gn_set_active_kpts`),
        then `gn_estimate`.  frames / tiles: (B, H, W) uint8 (numpy or device tensors, one size); dem: (B, H, W) uint8, uint16, int16 or
        float32 (set_dem_format), or None (flat).  report=True: as estimate; `kpt_q` / `kpt_r` [B,S,4] of the extraction are then added to the outputs, so that idx can be
        resolved to pixel coordinates.  cameras / camera_model (pair_cameras): one camera per frame, as estimate.  Returns (estimate outputs, n_keypoints [2B] int32 on the host: frames first)."""
        from .sift import SIFT
        if sift is None:
            if getattr(self, "_sift", None) is None:
                self._sift = SIFT(engine=self, max_keypoints=self.kmax)
            sift = self._sift
        to_dev = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, np.uint8), device=self.device)  # noqa: E731
        f, t = to_dev(frames), to_dev(tiles)
        assert f.shape == t.shape and f.dim() == 3, "expected two (B, H, W) uint8 stacks of one size"
        B = int(f.shape[0])
        kpt, _, _, desc, n = sift.detect_and_compute_batch_device(torch.cat([f, t], 0))
        totals = sift.last_totals(2 * B)
        if int(totals.max()) > sift._max:
            # cv2.SIFT_create() is unbounded (pose_node.py:122); the extractor kept the strongest max_keypoints by response.  Say so
            # instead of silently matching a truncated cloud; a caller that wants them all passes a larger SIFT / engine.
            import warnings
            warnings.warn(f"SIFT found up to {int(totals.max())} keypoints per image, kept the {sift._max} strongest (max_keypoints); "
                          "create the PoseEngine / SIFT with a larger max_kpts to match them all", RuntimeWarning, stacklevel=2)
        nd = torch.as_tensor(n, device=self.device)
        if dem is None:
            dem = torch.zeros((B, int(f.shape[1]), int(f.shape[2])), dtype=torch.uint8, device=self.device)
        inputs = dict(desc_q=desc[:B], kpt_q=kpt[:B], n_q=nd[:B], desc_r=desc[B:], kpt_r=kpt[B:], n_r=nd[B:], dem=dem if isinstance(dem, torch.Tensor) else _dev_tensor(np.asarray(dem), None, self.device), kpt_format=_lib.GN_KPT_XYSA)
        if cameras is not None:
            inputs.update(cameras=cameras, camera_model=camera_model)
        self.set_active_kpts(max(int(n.max()), 1))
        try:
            res = self.estimate(inputs, K, min_matches, out=out, report=report)
            if report:
                res = dict(res, kpt_q=inputs["kpt_q"], kpt_r=inputs["kpt_r"])
            self.flush()                                       # sub-stream groups read the temporaries above: join before they are released
        finally:
            self.set_active_kpts(self.kmax)                    # the active size is sticky context state: do not leak it to later calls
        return res, n

    # ------------------------------------------------------------------ visual-odometry path (TwistNode)
    def vo_match(self, desc_q, n_q, desc_r, n_r, ratio: float = 0.7, want_knn: bool = False):
        """gn_vo_match: BFMatcher(L2).knnMatch(k=2) + ratio test.  desc [B,S,128] f32, n [B] i32 (device).
        Returns (idx [B,kmax,2] i64, dist [B,kmax] f32, n_good [B] i32[, nn_idx [B,kmax,2] i32, nn_dist [B,kmax,2] f32])."""
        B = desc_q.shape[0]
        idx = torch.empty((B, self.kmax, 2), dtype=torch.int64, device=self.device)
        dist = torch.empty((B, self.kmax), dtype=torch.float32, device=self.device)
        n_good = torch.empty((B,), dtype=torch.int32, device=self.device)
        nn_idx = torch.empty((B, self.kmax, 2), dtype=torch.int32, device=self.device) if want_knn else None
        nn_dist = torch.empty((B, self.kmax, 2), dtype=torch.float32, device=self.device) if want_knn else None
        rc = self.lib.gn_vo_match(self.ctx, B, _ptr(desc_q), _ptr(n_q), desc_q.shape[1], _ptr(desc_r), _ptr(n_r), desc_r.shape[1],
                                  float(ratio), _ptr(idx), _ptr(dist), _ptr(n_good), _ptr(nn_idx), _ptr(nn_dist), self._stream())
        _lib.check(self.ctx, rc, "gn_vo_match")
        return (idx, dist, n_good, nn_idx, nn_dist) if want_knn else (idx, dist, n_good)

    def vo_estimate(self, inputs: dict, K: np.ndarray, ratio: float = 0.7, min_matches: int = 30, out: Optional[dict] = None,
                    covariance: bool = False, sigma_px: float = 0.0, report: bool = False):
        """gn_vo_estimate on staged inputs: TwistNode._pose lines 227-289 for the whole batch (covariance=True: gn_vo_estimate_cov, report=True:
        gn_vo_estimate_report, both as estimate; `score` is then the matches' distance).  inputs["cameras"] / inputs["camera_model"]: as estimate."""
        B = inputs["desc_q"].shape[0]
        with self._camera_table(inputs.get("cameras"), inputs.get("camera_model", 0), B, K):
            return self._vo_estimate(inputs, K, ratio, min_matches, out, covariance, sigma_px, report)

    def _vo_estimate(self, inputs, K, ratio, min_matches, out, covariance, sigma_px, report):
        B = inputs["desc_q"].shape[0]
        if out is None:
            out = self.alloc_outputs(B, covariance, report)
        K9 = _k9_ptr(K)
        args = (self.ctx, B, inputs["kpt_format"],
                _ptr(inputs["desc_q"]), _ptr(inputs["kpt_q"]), _ptr(inputs["n_q"]), inputs["desc_q"].shape[1],
                _ptr(inputs["desc_r"]), _ptr(inputs["kpt_r"]), _ptr(inputs["n_r"]), inputs["desc_r"].shape[1],
                K9, float(ratio), min_matches,
                _ptr(out["R"]), _ptr(out["t"]), _ptr(out["n_match"]), _ptr(out["n_inliers"]), _ptr(out["ok"]))
        if report:
            cov3 = (_ptr(out["cov"]), _ptr(out["sigma"]), _ptr(out["cov_ok"])) if covariance else (None, None, None)
            rc = self.lib.gn_vo_estimate_report(*args, float(sigma_px), *cov3, *self._report_ptrs(out), self._stream())
        elif covariance:
            rc = self.lib.gn_vo_estimate_cov(*args, float(sigma_px), _ptr(out["cov"]), _ptr(out["sigma"]), _ptr(out["cov_ok"]), self._stream())
        else:
            rc = self.lib.gn_vo_estimate(*args, self._stream())
        _lib.check(self.ctx, rc, "gn_vo_estimate_report" if report else "gn_vo_estimate_cov" if covariance else "gn_vo_estimate")
        return out

    def vo_estimate_images(self, frames_q, frames_r, K: np.ndarray, sift=None, ratio: float = 0.7, min_matches: int = 30, out: Optional[dict] = None,
                           report: bool = False):
        """TwistNode._pose from pixels for B frame pairs (twist_node.py:227-289), everything in HBM: one batched SIFT pass over
        the B query frames and the B reference (previous) frames, then brute-force 2-NN + ratio test + planar PnP
        (`gn_vo_estimate`).  report=True: as estimate_images.  Returns (outputs, n_keypoints [2B] int32 on the host: query frames first)."""
        from .sift import SIFT
        if sift is None:
            if getattr(self, "_sift", None) is None:
                self._sift = SIFT(engine=self, max_keypoints=self.kmax)
            sift = self._sift
        to_dev = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, np.uint8), device=self.device)  # noqa: E731
        q, r = to_dev(frames_q), to_dev(frames_r)
        assert q.shape == r.shape and q.dim() == 3, "expected two (B, H, W) uint8 stacks of one size"
        B = int(q.shape[0])
        kpt, _, _, desc, n = sift.detect_and_compute_batch_device(torch.cat([q, r], 0))
        nd = torch.as_tensor(n, device=self.device)
        inputs = dict(desc_q=desc[:B], kpt_q=kpt[:B], n_q=nd[:B], desc_r=desc[B:], kpt_r=kpt[B:], n_r=nd[B:], kpt_format=_lib.GN_KPT_XYSA)
        res = self.vo_estimate(inputs, K, ratio, min_matches, out=out, report=report)
        if report:
            res = dict(res, kpt_q=inputs["kpt_q"], kpt_r=inputs["kpt_r"])
        return res, n

    def alloc_outputs(self, B: int, covariance: bool = False, report: bool = False) -> dict:
        d = self.device
        out = dict(R=torch.empty((B, 3, 3), dtype=torch.float64, device=d), t=torch.empty((B, 3, 1), dtype=torch.float64, device=d),
                   n_match=torch.empty((B,), dtype=torch.int32, device=d), n_inliers=torch.empty((B,), dtype=torch.int32, device=d),
                   ok=torch.empty((B,), dtype=torch.uint8, device=d))
        if covariance:
            out.update(self._alloc_cov(B))
        if report:
            out.update(self._alloc_report(B, self.kmax, matches=True))
        return out

    # ------------------------------------------------------------------ test hooks
    def debug_read(self, name: str, count: int, dtype=np.float32) -> np.ndarray:
        buf = np.empty(count, dtype=dtype)
        n = self.lib.gn_debug_read(self.ctx, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.nbytes, self._stream())
        _lib.check(self.ctx, int(n), f"gn_debug_read({name})")
        return buf[: int(n)]

    def set_stage_timing(self, enable: bool) -> None:
        _lib.check(self.ctx, self.lib.gn_set_stage_timing(self.ctx, int(enable)), "gn_set_stage_timing")

    def stage_ms(self) -> Dict[str, float]:
        buf = (C.c_float * 16)()
        n = self.lib.gn_get_stage_ms(self.ctx, buf, 16)
        _lib.check(self.ctx, n, "gn_get_stage_ms")
        return {name: float(buf[i]) for i, name in enumerate(_lib.STAGE_NAMES[:n])}

    def set_kernel_timing(self, max_launches: int) -> None:
        _lib.check(self.ctx, self.lib.gn_set_kernel_timing(self.ctx, max_launches), "gn_set_kernel_timing")

    def kernel_stats(self, kernel_class: int = 0) -> Dict[str, float]:
        """HIP-event totals of the recorded launches; kernel_class 0 = GEMMs, 1 = attention."""
        buf = (C.c_double * 3)()
        _lib.check(self.ctx, self.lib.gn_get_kernel_stats(self.ctx, kernel_class, buf), "gn_get_kernel_stats")
        by = C.c_double(0.0)
        _lib.check(self.ctx, self.lib.gn_get_kernel_bytes(self.ctx, kernel_class, C.byref(by)), "gn_get_kernel_bytes")
        return {"launches": buf[0], "ms": buf[1], "flops": buf[2], "bytes": by.value}

    def kernel_table(self):
        """[{name, launches, ms, flops, bytes}] of the launches recorded since set_kernel_timing (HIP events on the launch stream)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        n = self.lib.gn_get_kernel_table(self.ctx, buf, len(buf))
        _lib.check(self.ctx, n, "gn_get_kernel_table")
        return json.loads(buf.value.decode())

    def debug_gemm(self, A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
        M, K = A.shape
        N = W.shape[0]
        Y = torch.empty((M, N), dtype=torch.float32, device=self.device)
        rc = self.lib.gn_debug_gemm(self.ctx, M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(Y), self._stream())
        _lib.check(self.ctx, rc, "gn_debug_gemm")
        return Y

    def debug_attention(self, q, k, v, nkv, cross: bool, qscale: float) -> torch.Tensor:
        """q,k,v [BS, npad, 256] f32 (4 heads x 64 concatenated); nkv [BS] i32."""
        BS, npad, _ = q.shape
        out = torch.empty_like(q)
        rc = self.lib.gn_debug_attention(self.ctx, BS, npad, int(cross), qscale, _ptr(q), 256, _ptr(k), 256, _ptr(v), 256,
                                         _ptr(nkv), _ptr(out), 256, self._stream())
        _lib.check(self.ctx, rc, "gn_debug_attention")
        return out

    def debug_match_head(self, md: torch.Tensor, ls: torch.Tensor, nvalid: torch.Tensor):
        """gn_debug_match_head: the match head alone.  md [B, 2, np, 256] f32, ls [B, 2, np] f32, nvalid [B, 2] i32 (device tensors).
        Returns (idx [B,kmax,2] i64, score [B,kmax] f32, n_match [B] i32) on the device; the per-row / per-column vectors through debug_read."""
        B, _, npad, _ = md.shape
        idx = torch.empty((B, self.kmax, 2), dtype=torch.int64, device=self.device)
        score = torch.empty((B, self.kmax), dtype=torch.float32, device=self.device)
        n_match = torch.empty((B,), dtype=torch.int32, device=self.device)
        rc = self.lib.gn_debug_match_head(self.ctx, B, npad, _ptr(md), _ptr(ls), _ptr(nvalid), _ptr(idx), _ptr(score), _ptr(n_match), self._stream())
        _lib.check(self.ctx, rc, "gn_debug_match_head")
        return idx, score, n_match

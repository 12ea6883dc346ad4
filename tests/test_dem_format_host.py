"""Elevation rasters beyond 8 bits, the parts that need no GPU (DESIGN.md "Elevation rasters: element types, scale, offset, voids"; the GPU side
is tests/test_gpu_dem_format.py):

  1. known answers of the numpy restatements (tests/dem_format_ref.py), worked by hand: the lift and the void compaction on a 3 x 4 raster, a .5
     tie of the float warp rounding to even, int16 saturation, angle 0 equal to a plain crop with voids included;
  2. ros2_node.image_to_dem: each encoding, a step larger than the row, big-endian data, a refused encoding;
  3. the mirrors' argument rules (check_dem_format, stereo_reference, PoseNode's parameters) raise before any device work;
  4. compute_pose's host-side lift (pose.lift_points) applies scale and offset and drops void rows;
  5. gn_set_dem_format / gn_get_dem_format / gn_dem_last_dropped / gn_stereo_reference_dem are declared in the header, exported by the built
     library and bound in _lib.SIGNATURES; gn_estimate / gn_gather_points are still declared verbatim;
  6. the scenes of tests/dem_format_common.py: every re-encoding lifts back to the uint8 raster; the tall scene is solved by the oracle's PnP and
     reading it through the low byte moves t by more than 1e-3 (the precondition of the GPU test).
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import dem_format_common as dc
import dem_format_ref as ref
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

HERE = os.path.dirname(os.path.abspath(__file__))
VP, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


# ------------------------------------------------------------------------------------------------------------------ 1
RASTER = np.array([[[10, 300, 40000, 7], [65535, 0, 256, 9], [1, 2, 3, 65535]]], np.uint16)      # 3 x 4


def test_lift_and_compaction_by_hand():
    # reference keypoints: (1.9, 0.2) -> cell (0, 1) = 300; (3.99, 2.5) -> (2, 3) = 65535 (void); (-4, 1.5) -> clamped (1, 0) = 65535 (void);
    # (4.0, 9.0) -> clamped (2, 3) = void; (2.0, 0.0) -> (0, 2) = 40000; (0.5, 2.7) -> (2, 0) = 1
    kr = np.array([[[1.9, 0.2, 0, 0], [3.99, 2.5, 0, 0], [-4.0, 1.5, 0, 0], [4.0, 9.0, 0, 0], [2.0, 0.0, 0, 0], [0.5, 2.7, 0, 0]]], np.float32)
    kq = np.arange(24, dtype=np.float32).reshape(1, 6, 4)
    idx = np.zeros((1, 8, 2), np.int64)
    idx[0, :6] = [[5, 0], [4, 1], [3, 2], [2, 3], [1, 4], [0, 5]]
    score = np.arange(8, dtype=np.float32)[None] / 8
    n = np.array([6], np.int32)
    plain = ref.gather(kq, kr, idx, n, RASTER, 0.03125, -15.625)
    assert plain["n_match"][0] == 6 and plain["dropped"][0] == 0
    assert plain["obj"][0, :6, 2].tolist() == [300 / 32 - 15.625, 65535 / 32 - 15.625, 65535 / 32 - 15.625, 65535 / 32 - 15.625, 40000 / 32 - 15.625, 1 / 32 - 15.625]
    assert plain["mkp_q"][0, 0].tolist() == [20.0, 21.0] and plain["obj"][0, 2, :2].tolist() == [-4.0, 1.5]      # coordinates stay, only the cell is clamped
    got = ref.gather(kq, kr, idx, n, RASTER, 0.03125, -15.625, nodata=65535, score=score)
    assert got["n_match"][0] == 3 and got["dropped"][0] == 3
    assert got["idx"][0, :3].tolist() == [[5, 0], [1, 4], [0, 5]] and got["score"][0, :3].tolist() == [0.0, 0.5, 0.625]
    assert got["obj"][0, :3, 2].tolist() == [300 / 32 - 15.625, 40000 / 32 - 15.625, 1 / 32 - 15.625]
    assert got["mkp_q"][0, :3].tolist() == [[20.0, 21.0], [4.0, 5.0], [0.0, 1.0]]
    # the same bits read as int16: 40000 is -25536, 65535 is -1
    assert ref.gather(kq, kr, idx, n, RASTER.view(np.int16))["obj"][0, :6, 2].tolist() == [300.0, -1.0, -1.0, -1.0, -25536.0, 1.0]
    # a scale that is no power of two: one rounding of the product, one of the sum, one to f32
    z = ref.lift(np.array([3300], np.uint16), 0.03, 0.1)[0]
    assert z == np.float32(np.float64(3300) * np.float64(0.03) + np.float64(0.1)) and z.dtype == np.float32
    # float rasters: non-finite cells are void whatever nodata is, NaN as nodata means those alone
    f = np.array([1.0, np.nan, -9999.0, np.inf], np.float32)
    assert ref.is_void(f, np.nan).tolist() == [False, True, False, True] and ref.is_void(f, -9999.0).tolist() == [False, True, True, True]
    assert not ref.is_void(f, None).any()


def test_float_warp_tie_rounds_to_even_and_saturates():
    # a 90 degree turn keeps the fractions at 0; half-cell fractions need a hand-made check of the blend itself: weights 1/4 each at fx = fy = 16
    H = W = 8
    sy, sx, fy, fx = ref.warp_coords(H, W, 0.0, (4, 4))
    assert not fy.any() and not fx.any() and np.array_equal(sy[:, 0], np.arange(2, 6)) and np.array_equal(sx[0], np.arange(2, 6))
    # 45 degrees on an 8 x 8 raster: find an output cell with fx = fy = 16 is not guaranteed, so the tie is checked on the rounding step directly
    assert np.rint(np.float32(2.5)) == 2 and np.rint(np.float32(3.5)) == 4 and np.rint(np.float32(-2.5)) == -2
    # int16 saturation through the whole restatement: a raster of 32767 rotated by 37.3 degrees never exceeds the type, and one of -32768 never
    # falls below it, although f32 sums of four products may round a hair past the ends
    for v in (32767, -32768):
        out = ref.warp_dem(np.full((61, 83), v, np.int16), 37.3, (40, 56))
        assert out.dtype == np.int16 and out.max() <= 32767 and out.min() >= -32768 and (out == v).sum() > 1000
    out = ref.warp_dem(np.full((61, 83), 65535, np.uint16), 37.3, (40, 56))
    assert out.max() == 65535
    # a tie by construction: source values (1, 2, 1, 2) under weights 1/4 give 1.5 -> 2, (2, 3, 2, 3) give 2.5 -> 2
    f32 = np.float32
    for taps, want in (((1, 2, 1, 2), 2), ((2, 3, 2, 3), 2), ((3, 4, 3, 4), 4)):
        w = f32(16 * 16) / f32(1024)
        v = f32(f32(f32(f32(taps[0]) * w + f32(taps[1]) * w) + f32(taps[2]) * w) + f32(taps[3]) * w)
        assert np.rint(v) == want


@pytest.mark.parametrize("name", ["uint8", "uint16", "int16", "float32"])
def test_angle_zero_is_a_plain_crop_voids_included(name):
    dem = dc.warp_raster(name)
    crop_shape = (40, 56)
    warp = ref.warp_dem_u8 if name == "uint8" else ref.warp_dem
    assert np.array_equal(warp(dem, 0.0, crop_shape), ref.crop(dem, crop_shape))
    for block in (False, True):
        d, nd = dc.with_voids(dem, crop_shape, block)
        out = warp(d, 0.0, crop_shape, nodata=nd)
        assert np.array_equal(out, ref.crop(d, crop_shape))                      # voids neither dilate nor vanish
        assert (out == nd).sum() == (1 if not block else 54)
    # a full-size crop: the last row and column have their right / lower taps outside the source at weight zero -- still an exact copy
    d, nd = dc.with_voids(dem, dem.shape, False)
    assert np.array_equal(warp(d, 0.0, dem.shape, nodata=nd), d)
    # at 37.3 degrees the corners of the crop lie outside the source and are void; a single void cell adds the few output cells whose live taps
    # touch it (a cell of the source is a tap of at most 4 output cells of a rigid turn, give or take the rounding of the fractions)
    d, nd = dc.with_voids(dem, crop_shape, False)
    clean = d.copy()
    clean[d == nd] = 7
    corners = (warp(clean, 37.3, crop_shape, nodata=nd) == nd)
    out = warp(d, 37.3, crop_shape, nodata=nd) == nd
    assert corners.sum() > 0 and not corners[10:30, 15:40].any() and (out | corners).sum() == out.sum()
    assert 1 <= out.sum() - corners.sum() <= 6


# ------------------------------------------------------------------------------------------------------------------ 2
def _img(arr, encoding, pad=0, big=False):
    a = np.asarray(arr)
    wire = a.astype(a.dtype.newbyteorder(">")) if big else a
    rows = [wire[r].tobytes() + b"\xee" * pad for r in range(a.shape[0])]
    return types.SimpleNamespace(height=a.shape[0], width=a.shape[1], encoding=encoding, is_bigendian=int(big),
                                 step=a.shape[1] * a.dtype.itemsize + pad, data=b"".join(rows))


@pytest.mark.parametrize("encoding, dtype", [("mono8", np.uint8), ("8UC1", np.uint8), ("mono16", np.uint16), ("16UC1", np.uint16),
                                             ("16SC1", np.int16), ("32FC1", np.float32)])
def test_image_to_dem_decodes_every_encoding(encoding, dtype):
    from gisnav_amd.ros2_node import image_to_dem
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((5, 7)) * 3000).astype(dtype) if dtype != np.uint8 else rng.integers(0, 256, (5, 7), dtype=np.uint8)
    for pad in (0, 6):
        for big in (False, True):
            got = image_to_dem(_img(a, encoding, pad, big))
            assert got.dtype == np.dtype(dtype) and got.dtype.isnative and np.array_equal(got, a), (pad, big)


def test_image_to_dem_refuses_other_encodings_by_name():
    from gisnav_amd.ros2_node import image_to_dem, ortho_stereo_image_from_ros
    a = np.zeros((4, 4), np.uint8)
    for enc in ("bgr8", "32SC1", "64FC1"):
        with pytest.raises(ValueError, match=enc):
            image_to_dem(_img(a, enc))
    with pytest.raises(ValueError, match="step"):
        image_to_dem(types.SimpleNamespace(height=4, width=4, encoding="mono16", is_bigendian=0, step=6, data=bytes(64)))
    with pytest.raises(ValueError, match="shorter"):
        image_to_dem(types.SimpleNamespace(height=4, width=4, encoding="mono16", is_bigendian=0, step=8, data=bytes(31)))
    # the message conversion decodes msg.dem with it, and msg.reference stays mono8
    hdr = types.SimpleNamespace(stamp=types.SimpleNamespace(sec=5, nanosec=6))
    dem16 = np.arange(16, dtype=np.int16).reshape(4, 4) - 8
    mk = lambda im: types.SimpleNamespace(header=hdr, **vars(im))  # noqa: E731
    msg = types.SimpleNamespace(query_sift=types.SimpleNamespace(data=b"", header=hdr), query=types.SimpleNamespace(header=hdr),
                                reference=mk(_img(a, "mono8")), dem=mk(_img(dem16, "16SC1")), crs=types.SimpleNamespace(data="x"))
    wire = ortho_stereo_image_from_ros(msg)
    assert wire.dem.data.dtype == np.int16 and np.array_equal(wire.dem.data, dem16) and wire.reference.data.dtype == np.uint8
    msg.reference = mk(_img(dem16, "16SC1"))
    with pytest.raises(ValueError, match="mono8"):
        ortho_stereo_image_from_ros(msg)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_argument_rules_raise_before_any_device_work():
    import torch
    from gisnav_amd import _lib
    from gisnav_amd.engine import check_dem_format, dem_dtype_name
    assert check_dem_format(np.uint8) == (_lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0)
    assert check_dem_format(torch.uint16, 0.03, -2.0, 65535) == (_lib.GN_DEM_U16, 0.03, -2.0, 1, 65535.0)
    assert check_dem_format(np.dtype("int16"), 1, 0, -32768) == (_lib.GN_DEM_I16, 1.0, 0.0, 1, -32768.0)
    typ, _, _, has, nd = check_dem_format(torch.float32, 4.0, -402.0, float("nan"))
    assert (typ, has) == (_lib.GN_DEM_F32, 1) and nd != nd
    assert (_lib.GN_DEM_U8, _lib.GN_DEM_U16, _lib.GN_DEM_I16, _lib.GN_DEM_F32) == (0, 1, 2, 3)
    for dt in (np.float64, np.int32, torch.int64, np.uint32, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16, int16 or float32"):
            dem_dtype_name(dt)
    for kw in (dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(offset=float("inf")), dict(offset=float("nan"))):
        with pytest.raises(ValueError):
            check_dem_format(np.uint16, **kw)
    for dt, nd in ((np.uint8, 256), (np.uint8, -1), (np.uint16, 65536), (np.uint16, 0.5), (np.int16, -32769), (np.int16, 32768), (np.int16, float("nan")),
                   (np.uint16, float("inf"))):
        with pytest.raises(ValueError, match="not representable"):
            check_dem_format(dt, 1.0, 0.0, nd)
    with pytest.raises(TypeError):
        check_dem_format(np.uint16, "1.0")
    # the mirrors: PoseEngine.set_dem_format / stereo_reference / PoseNode never reach the library with a refused argument
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.stereo import stereo_reference

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"device work ({name}) before the arguments were checked")
    eng = PoseEngine.__new__(PoseEngine)
    eng.lib, eng.ctx, eng._dem_fmt, eng._dem_applied = Boom(), None, (1.0, 0.0, None), (0, 1.0, 0.0, 0, 0.0)
    for args in ((0.0,), (float("nan"),), (1.0, float("inf")), (1.0, 0.0, "x")):
        with pytest.raises((ValueError, TypeError)):
            eng.set_dem_format(*args)
    assert eng.dem_format() == (1.0, 0.0, None)
    eng.set_dem_format(0.03, 1.5, -32768)
    assert eng.dem_format() == (0.03, 1.5, -32768.0)
    with pytest.raises(ValueError, match="not representable"):      # the nodata of the format against the raster of the call
        eng._apply_dem_format(torch.zeros((1, 2, 2), dtype=torch.uint16))
    with pytest.raises(ValueError, match="uint8, uint16, int16 or float32"):
        eng._apply_dem_format(torch.zeros((1, 2, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        stereo_reference(Boom(), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float64), 0.0, (2, 2))
    with pytest.raises(ValueError, match="not representable"):
        stereo_reference(Boom(), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint16), 0.0, (2, 2), nodata=-1)
    from gisnav_amd.pose_node import PoseNode
    with pytest.raises(ValueError, match="dem_scale"):
        PoseNode({}, dem_scale=0.0)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_compute_pose_lift_scales_and_drops_void_rows():
    from gisnav_amd.pose import compute_pose, lift_points
    dem = RASTER[0].view(np.int16)
    mkp_ref = np.array([[1.9, 0.2], [3.99, 2.5], [2.0, 0.0], [0.5, 2.7], [0.0, 1.0]], np.float32)      # cells 300, -1, -25536, 1, -1
    mkp_qry = np.arange(10, dtype=np.float64).reshape(5, 2)
    obj, img = lift_points(mkp_qry, mkp_ref, dem, 0.5, 2.0, -1)
    assert obj.dtype == np.float32 and img.dtype == np.float32
    assert obj.tolist() == [[np.float32(1.9), np.float32(0.2), 152.0], [2.0, 0.0, -12766.0], [0.5, np.float32(2.7), 2.5]]
    assert img.tolist() == [[0.0, 1.0], [4.0, 5.0], [6.0, 7.0]]
    obj, _ = lift_points(mkp_qry, mkp_ref, dem, 0.5, 2.0)
    assert len(obj) == 5 and obj[1, 2] == 1.5
    # nothing set: the raster is read as always, whatever its dtype
    obj, _ = lift_points(mkp_qry, mkp_ref, dem.astype(np.float64))
    assert obj[:, 2].tolist() == [300.0, -1.0, -25536.0, 1.0, -1.0]
    with pytest.raises(ValueError, match="not representable"):
        lift_points(mkp_qry, mkp_ref, dem, 1.0, 0.0, 0.5)
    # fewer than four rows left after the voids: no pose, and no engine is built for it
    cam = types.SimpleNamespace(k=K_MATRIX.reshape(9), d=None, distortion_model="")
    assert compute_pose(cam, mkp_qry, mkp_ref, dem, dem_nodata=-1) is None


# ------------------------------------------------------------------------------------------------------------------ 5
def test_symbols_are_declared_exported_and_bound():
    from gisnav_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(HERE, "..", "include", "gisnav_amd.h")).read())
    assert "enum { GN_DEM_U8 = 0, GN_DEM_U16 = 1, GN_DEM_I16 = 2, GN_DEM_F32 = 3 };" in header
    assert "int gn_set_dem_format(gn_ctx* ctx, int type, double scale, double offset, int has_nodata, double nodata);" in header
    assert "int gn_get_dem_format(const gn_ctx* ctx, int* type, double* scale, double* offset, int* has_nodata, double* nodata);" in header
    assert "int gn_dem_last_dropped(gn_ctx* ctx, int B, int32_t* dropped_host, void* stream);" in header
    assert ("int gn_stereo_reference_dem(gn_ctx* ctx, const uint8_t* bgr, const void* dem, int dem_type, int has_nodata, double nodata, int H, int W, "
            "double angle_degrees, int crop_h, int crop_w, uint8_t* out_ref, void* out_dem, double* back9_host, void* stream);") in header
    # the existing entry points keep their signatures
    assert ("int gn_gather_points(gn_ctx* ctx, int B, int kpt_format, const float* kpt_q, int stride_q, const float* kpt_r, int stride_r, "
            "const int64_t* idx, const int32_t* n_match, const uint8_t* dem, int H, int W, float* mkp_q, float* obj, void* stream);") in header
    assert ("int gn_estimate(gn_ctx* ctx, int B, int kpt_format, const float* desc_q, const float* kpt_q, const int32_t* n_q, int stride_q, "
            "const float* desc_r, const float* kpt_r, const int32_t* n_r, int stride_r, const uint8_t* dem, int H, int W, const double* K9_host, "
            "int min_matches, double* R, double* t, int32_t* n_match, int32_t* n_inliers, uint8_t* ok, void* stream);") in header
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    PI, PD = ctypes.POINTER(I), ctypes.POINTER(D)
    want = {"gn_set_dem_format": [VP, I, D, D, I, D],
            "gn_get_dem_format": [VP, PI, PD, PD, PI, PD],
            "gn_dem_last_dropped": [VP, I, ctypes.POINTER(ctypes.c_int32), VP],
            "gn_stereo_reference_dem": [VP, VP, VP, I, I, D, I, I, D, I, I, VP, VP, PD, VP]}
    lib = _lib.load()
    for name, args in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args
    err_arg = lib.gn_set_distortion(None, None, 0)                       # GN_ERR_ARG
    assert err_arg < 0
    assert lib.gn_set_dem_format(None, 0, 1.0, 0.0, 0, 0.0) == err_arg
    assert lib.gn_get_dem_format(None, None, None, None, None, None) == err_arg
    assert lib.gn_dem_last_dropped(None, 1, None, None) == err_arg
    assert lib.gn_stereo_reference_dem(None, None, None, 1, 0, 0.0, 4, 4, 0.0, 2, 2, None, None, None, None) == err_arg


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", ["uint16", "int16", "float32"])
def test_reencoded_rasters_lift_back_to_the_uint8_raster(name):
    p = make_pair(3, 300, 300)
    q, scale, offset = dc.reencode(p, name)
    assert q.dem.dtype.name == name and q.dem.shape == p.dem.shape
    assert np.array_equal(ref.lift(q.dem, scale, offset), p.dem.astype(np.float32))
    if name == "uint16":
        assert q.dem.max() > 255


def test_tall_scene_is_solved_and_discriminates():
    """The preconditions of the GPU test E: the oracle solves the tall scene from its true matches, and the same scene read through the low byte
    of the raster (what a uint8 cast of the uint16 cells gives) moves t by more than 1e-3."""
    for i in (0, 1):
        p = dc.tall_scene(i)
        assert p.dem.dtype == np.uint16 and p.dem.max() > 3000
        obj, img = dc.gt_points(p, p.dem, dc.TALL_SCALE)
        assert obj[:, 2].max() > 60.0
        ok, r, t, inl = pr.solve_pnp_ransac(obj, img, K_MATRIX)
        assert ok and len(inl) >= 0.9 * len(obj)
        assert np.linalg.norm(pr.rodrigues_vec2mat(r) - p.R_gt) < 1e-3 and np.linalg.norm(t - p.t_gt) / np.linalg.norm(p.t_gt) < 1e-3
        wrapped, _ = dc.gt_points(p, (p.dem & 0xff).astype(np.uint16), dc.TALL_SCALE)
        ok2, _, t2, _ = pr.solve_pnp_ransac(wrapped, img, K_MATRIX)
        moved = float(np.linalg.norm(t2 - t)) if ok2 else float("inf")
        print(f"tall scene {i}: low-byte read moves t by {moved:.3g}")
        assert moved > 1e-3

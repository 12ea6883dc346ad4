"""Elevation rasters beyond 8 bits on the GPU (DESIGN.md "Elevation rasters: element types, scale, offset, voids"): gn_set_dem_format through
gather_points and estimate, gn_dem_last_dropped, gn_stereo_reference_dem.  Expected values are the numpy restatements of tests/dem_format_ref.py;
everything is compared exactly unless stated.

  A. the lift of all four element types on an odd-width raster, two pairs with different rasters;
  B. off is off: the default format set explicitly, or another one set and reset, gives the bits of a fresh context; uint8 with a void value
     that no cell holds gives the bits of the plain gather;
  C. the void compaction at every chunk and wave boundary of a 2048-slot list;
  D. one scene in four encodings returns the uint8 call's pose bit for bit: single stream, sub-batch groups, the certificate's re-run (every pair
     flagged: the run of flagged pairs is re-run in place, in exact f32);
  E. tall terrain (raw relief 0 .. 3300 at scale 0.03) against the oracle's PnP;
  F. voids end to end under sub-batch groups, with the report;
  G. the reference-raster warp for uint16 / int16 / float32 rasters and for uint8 with voids;
  H. the refusals of the C ABI.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import dem_format_common as dc
import dem_format_ref as ref
from gisnav_amd import _lib
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu

H_A, W_A = 37, 53
DTYPES = ("uint8", "uint16", "int16", "float32")


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=4, max_kpts=2048)
    yield e
    del e


def _gather(e, kq, kr, idx, n, dem, score=None):
    """gather_points on copies of the match list; everything back on the host."""
    d = e.device
    idx_t, n_t = _dev(idx, d), _dev(n, d)
    score_t = None if score is None else _dev(score, d)
    mkp, obj = e.gather_points(_dev(kq, d), _dev(kr, d), idx_t, n_t, _dev(dem, d), score=score_t)
    torch.cuda.synchronize()
    return dict(mkp_q=mkp.cpu().numpy(), obj=obj.cpu().numpy(), idx=idx_t.cpu().numpy(), n_match=n_t.cpu().numpy(),
                score=None if score is None else score_t.cpu().numpy())


def _same_rows(got, want, keys):
    for b in range(len(want["n_match"])):
        m = int(want["n_match"][b])
        for k in keys:
            assert got[k][b, :m].tobytes() == want[k][b, :m].tobytes(), (k, b)


# ------------------------------------------------------------------------------------------------------------------ A
def _scene_a():
    rng = np.random.default_rng(11)
    S, n = 96, np.array([90, 61], np.int32)
    kr = np.zeros((2, S, 4), np.float32)
    kr[:, :, 0], kr[:, :, 1] = rng.uniform(-3, W_A + 3, (2, S)), rng.uniform(-3, H_A + 3, (2, S))      # some outside the raster on every side
    kr[0, :6, :2] = [[W_A - 0.5, H_A - 0.5], [W_A, 3.2], [-0.25, -7.0], [5.5, H_A], [W_A - 1, 0.0], [0.0, H_A - 1]]
    kq = rng.uniform(0, 500, (2, S, 4)).astype(np.float32)
    idx = np.zeros((2, 2048, 2), np.int64)
    for b in range(2):
        idx[b, :n[b], 0], idx[b, :n[b], 1] = rng.permutation(S)[:n[b]], rng.permutation(S)[:n[b]]
    return kq, kr, idx, n


def _raster_a(name):
    rng = np.random.default_rng(12)
    if name == "uint8":
        return rng.integers(0, 256, (2, H_A, W_A), dtype=np.uint8)
    if name == "float32":
        return (rng.standard_normal((2, H_A, W_A)) * 2500.0).astype(np.float32)
    d = rng.integers(0, 65536, (2, H_A, W_A)).astype(np.uint16)      # above 255 and above 32767
    return d if name == "uint16" else d.view(np.int16)


@pytest.mark.parametrize("scale, offset", [(1.0, 0.0), (0.03125, -15.625), (0.03, 0.1)])
@pytest.mark.parametrize("name", DTYPES)
def test_a_lift(eng, name, scale, offset):
    kq, kr, idx, n = _scene_a()
    dem = _raster_a(name)
    if name in ("uint16", "int16"):
        assert (dem.view(np.uint16) > 32767).any() and (dem.view(np.uint16) > 255).any()
    eng.set_dem_format(scale, offset)
    try:
        got = _gather(eng, kq, kr, idx, n, dem)
    finally:
        eng.set_dem_format()
    want = ref.gather(kq, kr, idx, n, dem, scale, offset)
    _same_rows(got, want, ("mkp_q", "obj"))
    assert np.array_equal(got["idx"], idx) and np.array_equal(got["n_match"], n)      # nothing is written without a void value
    if name == "int16":      # the same bits read as uint16 in a second call give other heights
        other = _gather(eng, kq, kr, idx, n, dem.view(np.uint16))
        assert not np.array_equal(other["obj"][0, :n[0], 2], got["obj"][0, :n[0], 2])
        _same_rows(other, ref.gather(kq, kr, idx, n, dem.view(np.uint16)), ("obj",))


# ------------------------------------------------------------------------------------------------------------------ B
def test_b_off_is_off(eng):
    from gisnav_amd.engine import PoseEngine
    kq, kr, idx, n = _scene_a()
    dem = _raster_a("uint8")
    fresh = PoseEngine(0, max_batch=4, max_kpts=2048)
    base = _gather(fresh, kq, kr, idx, n, dem)
    del fresh
    lib, ctx = eng.lib, eng.ctx
    assert lib.gn_set_dem_format(ctx, _lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0) == 0           # the default, set explicitly
    eng._dem_applied = (_lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0)
    explicit = _gather(eng, kq, kr, idx, n, dem)
    eng.set_dem_format(0.5, 3.0, 17)
    moved = _gather(eng, kq, kr, idx, n, dem)                                             # another format ...
    eng.set_dem_format()
    back = _gather(eng, kq, kr, idx, n, dem)                                              # ... and reset
    for got in (explicit, back):
        for k in ("mkp_q", "obj", "idx", "n_match"):
            assert got[k].tobytes() == base[k].tobytes(), k
    assert moved["obj"].tobytes() != base["obj"].tobytes()
    # uint8 with a void value that no cell holds: the compaction kernel runs and changes nothing
    clean = dem.copy()
    clean[clean == 255] = 254
    plain = _gather(eng, kq, kr, idx, n, clean)
    eng.set_dem_format(nodata=255)
    try:
        voided = _gather(eng, kq, kr, idx, n, clean)
        assert not eng.dem_last_dropped(2).any()
    finally:
        eng.set_dem_format()
    assert np.array_equal(voided["n_match"], n) and np.array_equal(voided["idx"], idx)
    _same_rows(voided, dict(plain, n_match=n), ("mkp_q", "obj"))


# ------------------------------------------------------------------------------------------------------------------ C
KMAX_C, SIDE_C = 2048, 64


def _void_pattern(kind, n, rng):
    v = np.zeros(n, bool)
    if kind == "edges":      # the first and the last row, and both sides of every multiple of 64 (so of 1024 too)
        for k in range(0, n + 1, 64):
            for j in (k - 1, k):
                if 0 <= j < n:
                    v[j] = True
        v[0] = v[n - 1] = True
    elif kind == "all":
        v[:] = True
    elif kind == "random":
        v = rng.random(n) < 0.3
    return v


@pytest.mark.parametrize("n_match", [1, 255, 256, 257, 1023, 1024, 1025, 2048])
def test_c_void_compaction(eng, n_match):
    rng = np.random.default_rng(100 + n_match)
    for kinds in (("edges", "none", "all"), ("random", "all", "edges")):
        B = 3
        kq = rng.uniform(0, 500, (B, KMAX_C, 4)).astype(np.float32)
        kr = np.zeros((B, KMAX_C, 4), np.float32)
        idx = np.zeros((B, KMAX_C, 2), np.int64)
        dem = rng.integers(0, 30000, (B, SIDE_C, SIDE_C)).astype(np.int16)
        score = (rng.permutation(B * KMAX_C).reshape(B, KMAX_C) + 1).astype(np.float32)      # distinct per row
        n = np.array([n_match, max(n_match - 1, 1), n_match], np.int32)
        for b, kind in enumerate(kinds):
            pq, pr_ = rng.permutation(KMAX_C), rng.permutation(KMAX_C)
            idx[b, :, 0], idx[b, :, 1] = pq, pr_
            rows = np.arange(KMAX_C)
            cell = rows * 2                                                  # row k owns a cell of its own
            kr[b, pr_, 0], kr[b, pr_, 1] = cell % SIDE_C + 0.5, cell // SIDE_C + 0.25
            v = _void_pattern(kind, int(n[b]), rng)
            dem[b].reshape(-1)[cell[:n[b]][v]] = -32768
        eng.set_dem_format(0.25, -3.0, -32768)
        try:
            got = _gather(eng, kq, kr, idx, n, dem, score=score)
            got["dropped"] = eng.dem_last_dropped(B)
        finally:
            eng.set_dem_format()
        want = ref.gather(kq, kr, idx, n, dem, 0.25, -3.0, -32768, score=score)
        assert np.array_equal(got["n_match"], want["n_match"]) and np.array_equal(got["dropped"], want["dropped"]), (kinds, got["n_match"], want["n_match"])
        assert want["n_match"][kinds.index("all")] == 0 and (want["dropped"] > 0).any()
        _same_rows(got, want, ("idx", "score", "mkp_q", "obj"))


# ------------------------------------------------------------------------------------------------------------------ D
def _estimate(e, pairs, report=False):
    out = e.estimate(e.stage_inputs(pairs), K_MATRIX, report=report)
    e.flush()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


POSE_KEYS = ("R", "t", "n_match", "n_inliers", "ok")


def _four_encodings(e, pairs):
    base = _estimate(e, pairs)
    assert base["ok"].all()
    for name in ("uint16", "int16", "float32"):
        enc = [dc.reencode(p, name) for p in pairs]
        e.set_dem_format(enc[0][1], enc[0][2])
        try:
            got = _estimate(e, [q for q, _, _ in enc])
        finally:
            e.set_dem_format()
        for k in POSE_KEYS:
            assert got[k].tobytes() == base[k].tobytes(), (name, k)


@pytest.fixture(scope="module")
def eng_f32(state_dict_np):
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=4, max_kpts=384, state_dict=state_dict_np)
    yield e
    del e


def test_d_one_scene_four_encodings(eng_f32):
    pairs = [make_pair(i, 300, 300) for i in (0, 1, 2)]
    _four_encodings(eng_f32, pairs)
    eng_f32.set_substreams(2)      # B = 4: group 1's rasters start 2 H W ELEMENTS in; every group's PnP runs on the PnP stream
    try:
        _four_encodings(eng_f32, pairs + [make_pair(3, 300, 300)])
    finally:
        eng_f32.flush()
        eng_f32.set_substreams(1)


def test_d_through_the_certificate_rerun(state_dict_np):
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=4, max_kpts=384, precision="f16x2_f16_attn", state_dict=state_dict_np)
    e.set_certify("rerun", eps=float("inf"))      # every pair is flagged and goes through the certificate's re-run in exact f32
    _four_encodings(e, [make_pair(i, 300, 300) for i in (0, 1, 2)])
    assert e.certify_stats()["rerun_pairs"] >= 12      # four calls of three pairs, every pair re-run
    del e


# ------------------------------------------------------------------------------------------------------------------ E
def test_e_tall_terrain(eng_f32):
    pairs = [dc.tall_scene(0), dc.tall_scene(1)]
    eng_f32.set_dem_format(dc.TALL_SCALE)
    try:
        got = _estimate(eng_f32, pairs, report=True)
    finally:
        eng_f32.set_dem_format()
    for b, p in enumerate(pairs):
        m = int(got["n_match"][b])
        assert got["ok"][b] and m >= 100
        idx = got["idx"][b, :m]
        yi, xi = ref.cells(p.kp_r[idx[:, 1]], *p.dem.shape)
        obj = np.column_stack([p.kp_r[idx[:, 1]], ref.lift(p.dem[yi, xi], dc.TALL_SCALE)]).astype(np.float32)
        assert obj[:, 2].max() > 60.0
        ok, r, t, _ = pr.solve_pnp_ransac(obj, p.kp_q[idx[:, 0]], K_MATRIX)
        assert ok
        dR, dt = np.linalg.norm(got["R"][b].reshape(3, 3) - pr.rodrigues_vec2mat(r)), np.linalg.norm(got["t"][b].reshape(3, 1) - t) / np.linalg.norm(t)
        print(f"tall scene {b}: dR {dR:.2e} dt {dt:.2e}")
        assert dR < 1e-8 and dt < 1e-8, (b, dR, dt)


# ------------------------------------------------------------------------------------------------------------------ F
def test_f_voids_end_to_end(eng_f32):
    e = eng_f32
    tall = [dc.tall_scene(0), dc.tall_scene(1), dc.tall_scene(2)]
    pairs = [dc.void_cells(tall[0], 0.10, 7), dc.void_cells(tall[1], 1.0, 8, every=True), dataclasses.replace(tall[2], dem=tall[2].dem.astype(np.int16))]
    e.set_substreams(2)
    try:
        e.set_dem_format(dc.TALL_SCALE)
        full = _estimate(e, pairs, report=True)                    # the void value read as a height: the whole match list
        e.set_dem_format(dc.TALL_SCALE, 0.0, -32768)
        got = _estimate(e, pairs, report=True)
        dropped = e.dem_last_dropped(3)
    finally:
        e.set_dem_format()
        e.flush()
        e.set_substreams(1)
    inputs = e.stage_inputs(pairs)
    kq, kr = inputs["kpt_q"].cpu().numpy(), inputs["kpt_r"].cpu().numpy()
    dem = np.stack([p.dem for p in pairs])
    want = ref.gather(kq, kr, full["idx"], full["n_match"], dem, dc.TALL_SCALE, 0.0, -32768, score=full["score"])
    assert np.array_equal(got["n_match"], want["n_match"]) and np.array_equal(dropped, want["dropped"])
    assert 0 < want["dropped"][0] < full["n_match"][0] and want["dropped"][2] == 0
    _same_rows(got, want, ("idx", "score"))
    for b in range(3):
        m = int(got["n_match"][b])
        inl = got["inlier_idx"][b]
        assert (inl[inl >= 0] < m).all() and (inl >= 0).sum() == (got["n_inliers"][b] if got["ok"][b] else 0)
        assert not got["inlier_mask"][b, m:].any()
    # a pair whose matched cells are all void: no matches, no pose; its neighbour in the other group is untouched
    assert got["n_match"][1] == 0 and got["ok"][1] == 0 and full["n_match"][1] > 100
    for k in POSE_KEYS + ("idx", "score", "inlier_idx", "reproj_err"):
        assert got[k][2].tobytes() == full[k][2].tobytes(), k
    # the pose of pair 0 is the pose of a PnP call given the pre-filtered list
    assert got["ok"][0]
    d = e.device
    res = e.pnp_ransac(_dev(want["obj"][:1], d), _dev(want["mkp_q"][:1], d), _dev(want["n_match"][:1], d), K_MATRIX, min_pts=15)
    torch.cuda.synchronize()
    assert res[0].cpu().numpy().tobytes() == got["R"][0].tobytes() and res[1].cpu().numpy().tobytes() == got["t"][0].tobytes()
    assert int(res[2].cpu()[0]) == got["n_inliers"][0]


# ------------------------------------------------------------------------------------------------------------------ G
CROP_G = (40, 56)


@pytest.mark.parametrize("angle", [0.0, 90.0, 37.3, -123.45])
@pytest.mark.parametrize("name, voids", [("uint16", None), ("int16", None), ("float32", None), ("uint8", "cell"), ("uint8", "block"),
                                         ("uint16", "block"), ("int16", "cell"), ("float32", "block"), ("float32", "nan")])
def test_g_warp(eng, name, voids, angle):
    from gisnav_amd.stereo import stereo_reference
    dem = dc.warp_raster(name)
    bgr = np.random.default_rng(21).integers(0, 256, dem.shape + (3,), dtype=np.uint8)
    nodata = None
    if voids == "nan":
        dem = dem.copy()
        dem[30:33, 40:45], dem[10, 60], nodata = np.nan, np.inf, float("nan")
    elif voids is not None:
        dem, nodata = dc.with_voids(dem, CROP_G, voids == "block")
    out_ref, out_dem, back = stereo_reference(eng, bgr, dem, angle, CROP_G, nodata=nodata)
    base_ref, _, base_back = stereo_reference(eng, bgr, np.zeros(dem.shape, np.uint8), angle, CROP_G)      # gn_stereo_reference itself
    torch.cuda.synchronize()
    assert out_ref.cpu().numpy().tobytes() == base_ref.cpu().numpy().tobytes() and np.array_equal(back, base_back)
    got = out_dem.cpu().numpy()
    want = (ref.warp_dem_u8 if name == "uint8" else ref.warp_dem)(dem, angle, CROP_G, nodata=nodata)
    assert got.dtype == dem.dtype and np.array_equal(got, want, equal_nan=name == "float32")
    if angle == 0.0:
        plain = ref.crop(dem, CROP_G)
        if voids == "nan":      # a void cell stores the void value: the +Inf cell comes out as NaN like the NaN cells
            plain = np.where(np.isfinite(plain), plain, np.float32(np.nan))
        assert np.array_equal(got, plain, equal_nan=name == "float32")
    if voids is not None:
        void = np.isnan(got) if voids == "nan" else got == nodata
        assert not void.all()
        if voids != "block" or angle == 0.0:      # (the block touches the crop's edge at angle 0 and may turn out of the window elsewhere)
            assert void.any()


# ------------------------------------------------------------------------------------------------------------------ H
def test_h_refusals(eng):
    lib, ctx = eng.lib, eng.ctx
    err_arg = lib.gn_set_distortion(None, None, 0)
    assert lib.gn_set_dem_format(ctx, _lib.GN_DEM_I16, 0.03, 1.5, 1, -32768.0) == 0

    def state():
        t, h = C.c_int(-1), C.c_int(-1)
        s, o, nd = C.c_double(), C.c_double(), C.c_double()
        assert lib.gn_get_dem_format(ctx, C.byref(t), C.byref(s), C.byref(o), C.byref(h), C.byref(nd)) == 0
        return t.value, s.value, o.value, h.value, nd.value
    try:
        assert state() == (_lib.GN_DEM_I16, 0.03, 1.5, 1, -32768.0)
        nan, inf = float("nan"), float("inf")
        bad = [(4, 1.0, 0.0, 0, 0.0), (-1, 1.0, 0.0, 0, 0.0), (1, 0.0, 0.0, 0, 0.0), (1, nan, 0.0, 0, 0.0), (1, inf, 0.0, 0, 0.0), (1, 1.0, inf, 0, 0.0),
               (1, 1.0, nan, 0, 0.0), (0, 1.0, 0.0, 1, 256.0), (0, 1.0, 0.0, 1, -1.0), (1, 1.0, 0.0, 1, 65536.0), (1, 1.0, 0.0, 1, 0.5),
               (2, 1.0, 0.0, 1, -32769.0), (2, 1.0, 0.0, 1, 32768.0), (2, 1.0, 0.0, 1, nan), (1, 1.0, 0.0, 1, inf)]
        for args in bad:
            assert lib.gn_set_dem_format(ctx, *args) == err_arg, args
            assert b"gn_set_dem_format" in lib.gn_last_error(ctx), args
            assert state() == (_lib.GN_DEM_I16, 0.03, 1.5, 1, -32768.0), args
        # accepted: a float raster takes any void value, NaN included; a void value is not looked at while has_nodata is 0
        assert lib.gn_set_dem_format(ctx, _lib.GN_DEM_F32, 4.0, -402.0, 1, nan) == 0
        assert state()[:4] == (_lib.GN_DEM_F32, 4.0, -402.0, 1) and state()[4] != state()[4]
        assert lib.gn_set_dem_format(ctx, _lib.GN_DEM_U8, 2.0, 0.0, 0, 1e9) == 0
        dropped = np.zeros(8, np.int32)
        assert lib.gn_dem_last_dropped(ctx, 0, dropped.ctypes.data_as(_lib.c_i32p), None) == err_arg
        assert lib.gn_dem_last_dropped(ctx, 5, dropped.ctypes.data_as(_lib.c_i32p), None) == err_arg      # max_batch is 4
        assert lib.gn_dem_last_dropped(ctx, 2, None, None) == err_arg
        buf = torch.zeros(64, dtype=torch.uint8, device=eng.device)
        p = C.c_void_p(buf.data_ptr())
        for args in ((p, p, 4, 0, 0.0), (p, p, _lib.GN_DEM_U16, 1, -1.0), (p, p, _lib.GN_DEM_I16, 1, 0.5), (None, p, 1, 0, 0.0)):
            assert lib.gn_stereo_reference_dem(ctx, *args, 4, 4, 0.0, 2, 2, p, p, None, None) == err_arg, args
            assert b"gn_stereo_reference_dem" in lib.gn_last_error(ctx)
    finally:
        assert lib.gn_set_dem_format(ctx, _lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0) == 0
        eng._dem_applied = (_lib.GN_DEM_U8, 1.0, 0.0, 0, 0.0)


# ------------------------------------------------------------------------------------------------------------------ seams
def test_seams_carry_the_element_type(state_dict_np, eng_f32):
    """PoseNode's pinned raster, RecordStager(dem_dtype=), estimate_bucketed and compute_pose with a re-encoded raster return what the uint8
    raster returns: the same bits through one path, uint8 against uint16 / int16."""
    from gisnav_amd import wire
    from gisnav_amd.engine import RecordStager
    from gisnav_amd.pose import compute_pose
    from gisnav_amd.pose_node import PoseNode
    p = make_pair(86, n_q=300, n_r=280)
    q16, scale, offset = dc.reencode(p, "int16")
    extractor = lambda r: (p.kp_r, p.desc_r, p.size_r, p.angle_r)  # noqa: E731
    cam = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    mk = lambda dem: wire.OrthoStereoImage(query_sift=wire.pack_keypoints(p.kp_q, p.size_q, p.angle_q, p.desc_q),  # noqa: E731
                                           reference=wire.ImageMsg(p.ref, wire.Stamp(7, 0)), dem=wire.ImageMsg(dem, wire.Stamp(7, 0)))
    r8 = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32").estimate(cam, mk(p.dem))
    node = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32", dem_scale=scale, dem_offset=offset)
    r16 = node.estimate(cam, mk(q16.dem))
    assert r8 is not None and np.array_equal(r8[0], r16[0]) and np.array_equal(r8[1], r16[1])
    void = dc.void_cells(q16, 0.1, 3)
    node_v = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32", dem_scale=scale, dem_offset=offset, dem_nodata=-32768)
    rv = node_v.estimate(cam, mk(void.dem))
    assert rv is not None and 0 < node_v.last_num_matches < node.last_num_matches
    # (nine tenths of the same matches, 0.5 px of keypoint noise: the same pose to well under a percent)
    assert np.linalg.norm(rv[1] - r8[1]) / np.linalg.norm(r8[1]) < 1e-2
    # RecordStager with uint16 rasters against RecordStager with the uint8 ones
    e = eng_f32
    pairs = [make_pair(i, 300, 300) for i in (0, 1)]
    enc = [dc.reencode(x, "uint16") for x in pairs]
    recs = lambda ps: [(wire.pack_keypoints(x.kp_q, x.size_q, x.angle_q, x.desc_q), wire.pack_keypoints(x.kp_r, x.size_r, x.angle_r, x.desc_r), x.dem) for x in ps]  # noqa: E731
    st8 = RecordStager(e, 2, 384, pairs[0].dem.shape, depth=2, copy_threads=1, numa=None)
    inp8 = st8.stage(recs(pairs))
    st8.wait(inp8)
    base = {k: v.cpu().numpy() for k, v in e.estimate(inp8, K_MATRIX).items()}
    st8.release(inp8)
    st8.close()
    assert base["ok"].all()
    st = RecordStager(e, 2, 384, pairs[0].dem.shape, depth=2, copy_threads=1, numa=None, dem_dtype=torch.uint16)
    msgs = recs([x for x, _, _ in enc])
    with pytest.raises(_lib.GnError, match="dem_dtype"):
        st.stage([(m[0], m[1], pairs[0].dem) for m in msgs])
    inp = st.stage(msgs)
    st.wait(inp)
    e.set_dem_format(enc[0][1], enc[0][2])
    try:
        rec = {k: v.cpu().numpy() for k, v in e.estimate(inp, K_MATRIX).items()}
        bkt, _ = e.estimate_bucketed(e.stage_inputs([x for x, _, _ in enc]), K_MATRIX, [300, 300], [300, 300], bucket_pairs=1)
        bkt = {k: v.cpu().numpy() for k, v in bkt.items()}
    finally:
        e.set_dem_format()
        st.release(inp)
        st.close()
    bkt8, _ = e.estimate_bucketed(e.stage_inputs(pairs), K_MATRIX, [300, 300], [300, 300], bucket_pairs=1)
    for k in POSE_KEYS:
        assert rec[k].tobytes() == base[k].tobytes(), k
        assert bkt[k].tobytes() == bkt8[k].cpu().numpy().tobytes(), k
    # compute_pose's host-side lift
    ok8 = compute_pose(cam, p.kp_q[p.gt_q2r >= 0], p.kp_r[p.gt_q2r[p.gt_q2r >= 0]], p.dem, engine=e)
    ok16 = compute_pose(cam, p.kp_q[p.gt_q2r >= 0], p.kp_r[p.gt_q2r[p.gt_q2r >= 0]], q16.dem, engine=e, dem_scale=scale, dem_offset=offset)
    assert ok8 is not None and np.array_equal(ok8[0], ok16[0]) and np.array_equal(ok8[1], ok16[1])

"""Per-pair cameras, the parts that need no GPU (DESIGN.md "Per-pair cameras"; the GPU side is tests/test_gpu_pair_cameras.py):

  1. the precondition of the GPU tests: every scene of tests/pair_cameras_common.py solved by the fp64 restatement with its OWN camera returns
     the true inliers and the true pose (2e-4, the bound of DESIGN "Lens distortion"); with the NEXT pair's camera it finds no model or misses t
     by more than 1 -- a camera given to the wrong pair cannot pass;
  2. gn_set_pair_cameras / gn_get_pair_cameras are declared, exported and bound, and refuse a null context;
  3. PoseEngine.pair_cameras' ValueErrors (shape, non-finite values, skew, last row) and the rows it builds;
  4. estimate / vo_estimate / pnp_ransac / undistort_points: a row count other than B raises before any library call; with a table the library
     sees set -> call (K9 NULL) -> unset; without one, the call alone (a recording library);
  5. estimate_bucketed permutes and slices `cameras` with the other tensors and passes `camera_model` through;
  6. compute_pose_batch: an unsupported distortion_model raises through distortion_of, short messages yield None without a GPU call.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pair_cameras_common as pc
from gisnav_amd.synthetic import K_MATRIX

HERE = os.path.dirname(os.path.abspath(__file__))
VP, I = ctypes.c_void_p, ctypes.c_int


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("b", range(pc.NB))
def test_own_camera_solves_the_scene_and_the_neighbours_cannot(b):
    o, u, rv, tv, inl = pc.scenes()[b]
    assert len(o) == pc.POINTS[b] and int(inl.sum()) == pc.TRUE_INLIERS[b]
    ok, r, t, idx = pc.restated(b, b)
    assert ok and np.array_equal(idx, np.nonzero(inl)[0])
    gt = max(np.abs(r.reshape(3) - rv).max(), np.abs(t.reshape(3) - tv).max())
    ok2, _, t2, _ = pc.restated(b, (b + 1) % pc.NB)
    miss = float(np.linalg.norm(t2.reshape(3) - tv)) if ok2 else float("inf")
    print(f"scene {b}: own camera {gt:.2e} from truth; camera {(b + 1) % pc.NB}: ok {ok2}, |dt| {miss:.1f}")
    assert gt <= 2e-4
    assert (not ok2) or miss > 1.0


def test_table_rows_layout():
    rows = pc.table_rows()
    assert rows.shape == (5, 9) and rows.dtype == np.float64
    assert rows[1].tolist() == [410.9392, 395.0, 331.5, 236.0, -0.11, 0.03, -4e-4, 6e-4, -0.004]
    assert not rows[2, 4:].any()
    # pairwise different: a swap of two rows is a different table
    assert len({r.tobytes() for r in rows}) == 5


# ------------------------------------------------------------------------------------------------------------------ 2
def test_symbols_are_declared_exported_and_bound():
    from gisnav_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(HERE, "..", "include", "gisnav_amd.h")).read())
    assert re.search(r"#define GN_PAIR_CAMERA_DOUBLES 9\b", header)
    assert "int gn_set_pair_cameras(gn_ctx* ctx, const double* cams, int n, int model);" in header
    assert "int gn_get_pair_cameras(const gn_ctx* ctx, const double** cams, int* n, int* model);" in header
    assert _lib.GN_PAIR_CAMERA_DOUBLES == 9
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = {"gn_set_pair_cameras": [VP, VP, I, I],
            "gn_get_pair_cameras": [VP, ctypes.POINTER(VP), ctypes.POINTER(I), ctypes.POINTER(I)]}
    lib = _lib.load()
    for name, args in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args
    err_arg = lib.gn_set_distortion(None, None, 0)                       # GN_ERR_ARG
    assert err_arg < 0
    assert lib.gn_set_pair_cameras(None, None, 0, 0) == err_arg
    assert lib.gn_set_pair_cameras(None, None, 3, 1) == err_arg
    assert lib.gn_get_pair_cameras(None, None, None, None) == err_arg


# ------------------------------------------------------------------------------------------------------------------ 3
class _Recorder:
    """Stands in for the loaded library: records (entry point, arguments) and returns GN_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _stub_engine(kmax=128):
    from gisnav_amd.engine import PoseEngine
    e = object.__new__(PoseEngine)
    e.device, e.kmax, e.ctx, e.lib = torch.device("cpu"), kmax, None, _Recorder()
    e._stream = lambda: None
    e._last_out_ptr = None
    e.uploads = []
    e.to_device = lambda name, a, dtype=torch.float32: (e.uploads.append(name), torch.as_tensor(np.asarray(a)).to(dtype))[1]      # (no pinned memory here)
    return e


def test_pair_cameras_checks_on_the_host():
    e = _stub_engine()
    cams, model = e.pair_cameras(pc.KS, pc.DS)
    assert model == 1 and cams.dtype == torch.float64 and cams.shape == (5, 9) and e.uploads == ["pair_cameras"]
    assert np.array_equal(cams.numpy(), pc.table_rows())
    cams4, model4 = e.pair_cameras(pc.KS, pc.DS[:, :4])                    # four coefficients: k3 = 0
    assert model4 == 1 and np.array_equal(cams4.numpy()[:, :8], pc.table_rows()[:, :8]) and not cams4.numpy()[:, 8].any()
    cams0, model0 = e.pair_cameras(pc.KS)
    assert model0 == 0 and np.array_equal(cams0.numpy()[:, :4], pc.table_rows()[:, :4]) and not cams0.numpy()[:, 4:].any()
    n_up = len(e.uploads)

    def bad(K, d=None):
        with pytest.raises(ValueError):
            e.pair_cameras(K, d)

    bad(pc.KS[0])                                                          # (3, 3): the one-camera form belongs to the K argument
    bad(pc.KS.reshape(5, 9))
    bad(pc.KS, pc.DS[0])                                                   # d must be (B, 4 | 5)
    bad(pc.KS, pc.DS[:4])
    bad(pc.KS, np.zeros((5, 8)))                                           # plumb-bob only
    for val in (np.nan, np.inf):
        K = pc.KS.copy(); K[3, 1, 1] = val; bad(K)
        D = pc.DS.copy(); D[2, 4] = val; bad(pc.KS, D)
    K = pc.KS.copy(); K[1, 0, 1] = 1e-3; bad(K)                            # skew
    for r, c, v in ((2, 0, 1e-9), (2, 1, -1.0), (2, 2, 2.0)):              # last row != (0, 0, 1)
        K = pc.KS.copy(); K[4, r, c] = v; bad(K)
    assert len(e.uploads) == n_up and not e.lib.calls                      # nothing reached the device or the library


# ------------------------------------------------------------------------------------------------------------------ 4
def _inputs(B):
    from gisnav_amd import _lib
    return dict(desc_q=torch.zeros(B, 128, 128), kpt_q=torch.zeros(B, 128, 4), n_q=torch.zeros(B, dtype=torch.int32),
                desc_r=torch.zeros(B, 128, 128), kpt_r=torch.zeros(B, 128, 4), n_r=torch.zeros(B, dtype=torch.int32),
                dem=torch.zeros(B, 8, 8, dtype=torch.uint8), kpt_format=_lib.GN_KPT_XYSA)


def _addr(p):
    return None if p is None else (p.value if isinstance(p, ctypes.c_void_p) else p)


def test_row_count_mismatch_raises_before_any_call():
    e = _stub_engine()
    cams = torch.from_numpy(pc.table_rows())                               # five rows
    obj, img, n = torch.zeros(3, 64, 3), torch.zeros(3, 64, 2), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="5 rows for a call of 3"):
        e.estimate(dict(_inputs(3), cameras=cams, camera_model=1), None)
    with pytest.raises(ValueError, match="5 rows for a call of 3"):
        e.vo_estimate(dict(_inputs(3), cameras=cams, camera_model=1), None)
    with pytest.raises(ValueError, match="5 rows for a call of 3"):
        e.pnp_ransac(obj, img, n, None, cameras=cams, camera_model=1)
    with pytest.raises(ValueError, match="5 rows for a call of 3"):
        e.undistort_points(img, n, cameras=cams, camera_model=1)
    with pytest.raises(ValueError):
        e.pnp_ransac(obj, img, n, None, cameras=cams[:3].to(torch.float32), camera_model=1)      # not f64
    with pytest.raises(ValueError):
        e.pnp_ransac(obj, img, n, None, cameras=cams[:3, :8], camera_model=1)                     # not 9 columns
    with pytest.raises(ValueError):
        e.pnp_ransac(obj, img, n, None, cameras=cams[:3], camera_model=2)
    with pytest.raises(ValueError):
        e.pnp_ransac(obj, img, n, None)                                                           # neither K nor a table
    assert not e.lib.calls


def test_calls_set_the_table_around_the_c_call_and_only_then():
    e = _stub_engine()
    cams = torch.from_numpy(pc.table_rows()[:3].copy())
    obj, img, n = torch.zeros(3, 64, 3), torch.zeros(3, 64, 2), torch.zeros(3, dtype=torch.int32)
    e.estimate(dict(_inputs(3), cameras=cams, camera_model=1), None)
    e.vo_estimate(dict(_inputs(3), cameras=cams, camera_model=0), None)
    e.pnp_ransac(obj, img, n, None, cameras=cams, camera_model=1, covariance=True, report=True)
    e.undistort_points(img, n, cameras=cams, camera_model=1, to_pixels=True)
    names = [c[0] for c in e.lib.calls]
    assert names == ["gn_set_pair_cameras", "gn_estimate", "gn_set_pair_cameras",
                     "gn_set_pair_cameras", "gn_vo_estimate", "gn_set_pair_cameras",
                     "gn_set_pair_cameras", "gn_pnp_ransac_report", "gn_set_pair_cameras",
                     "gn_set_pair_cameras", "gn_undistort_points", "gn_set_pair_cameras"]
    for k, model in zip((0, 3, 6, 9), (1, 0, 1, 1)):
        on, off = e.lib.calls[k][1], e.lib.calls[k + 2][1]
        assert (_addr(on[1]), on[2], on[3]) == (cams.data_ptr(), 3, model)
        assert (_addr(off[1]), off[2], off[3]) == (None, 0, 0)
    assert e.lib.calls[1][1][14] is None and e.lib.calls[4][1][11] is None        # K9_host: NULL
    assert e.lib.calls[7][1][6] is None and e.lib.calls[10][1][5] is None
    # without a table: the call it always was, and nothing else
    e.lib.calls.clear()
    e.estimate(_inputs(3), K_MATRIX)
    e.pnp_ransac(obj, img, n, K_MATRIX)
    e.undistort_points(img, n, K_MATRIX)
    assert [c[0] for c in e.lib.calls] == ["gn_estimate", "gn_pnp_ransac", "gn_undistort_points"]
    assert e.lib.calls[0][1][14] is not None


def test_a_failing_call_still_unsets_the_table():
    e = _stub_engine()

    class Boom(Exception):
        pass

    def boom(*a):
        raise Boom()
    rec = e.lib
    rec.gn_pnp_ransac = boom
    cams = torch.from_numpy(pc.table_rows()[:2].copy())
    with pytest.raises(Boom):
        e.pnp_ransac(torch.zeros(2, 64, 3), torch.zeros(2, 64, 2), torch.zeros(2, dtype=torch.int32), None, cameras=cams, camera_model=1)
    assert [c[0] for c in rec.calls] == ["gn_set_pair_cameras", "gn_set_pair_cameras"] and rec.calls[-1][1][2] == 0


# ------------------------------------------------------------------------------------------------------------------ 5
def test_estimate_bucketed_carries_the_rows_with_their_pairs():
    e = _stub_engine()
    e.set_active_kpts = lambda k: ((int(k) + 127) // 128) * 128
    e.flush = lambda: None
    B = 8
    n_host = np.array([60, 250, 130, 200, 90, 256, 40, 180])
    rows = np.arange(B * 9, dtype=np.float64).reshape(B, 9)                # row b starts with 9 b
    inp = dict(_inputs(B), cameras=torch.from_numpy(rows), camera_model=1)
    seen = []
    e._estimate = lambda inputs, K, *a: seen.append((inputs["cameras"].clone(), inputs["camera_model"], inputs["cameras"].data_ptr()))
    e.estimate_bucketed(inp, None, n_host, n_host, bucket_pairs=3)
    order = np.argsort(-n_host, kind="stable")
    assert order.tolist() != list(range(B))
    assert [len(s[0]) for s in seen] == [3, 3, 2] and all(s[1] == 1 for s in seen)
    got = torch.cat([s[0] for s in seen]).numpy()
    assert np.array_equal(got, rows[order])                                # bucket k, slot j holds the camera of the pair that runs there
    sets = [c for c in e.lib.calls if c[0] == "gn_set_pair_cameras"]
    assert [c[1][2] for c in sets] == [3, 0, 3, 0, 2, 0]                   # set with the bucket's rows, unset, per bucket
    assert [_addr(c[1][1]) for c in sets[0::2]] == [s[2] for s in seen]


# ------------------------------------------------------------------------------------------------------------------ 6
def test_compute_pose_batch_refusals_need_no_gpu(monkeypatch):
    from gisnav_amd import pose, wire

    def no_engine(*a, **kw):
        raise AssertionError("no engine may be created for these calls")
    monkeypatch.setattr(pose, "PoseEngine", no_engine)
    monkeypatch.setattr(pose, "_batch_engine", None)
    k9 = pc.KS[0].reshape(9)
    good = wire.CameraInfo(k=k9, height=480, width=640, d=pc.DS[0], distortion_model="plumb_bob")
    fisheye = wire.CameraInfo(k=k9, height=480, width=640, d=np.zeros(4), distortion_model="equidistant")
    pts = [np.zeros((3, 2), np.float32), np.zeros((0, 2), np.float32)]
    with pytest.raises(ValueError, match="equidistant"):
        pose.compute_pose_batch([good, fisheye], pts, pts, [None, None], use_distortion=True)
    # the default ignores d and the model, as compute_pose does; messages below solvePnPRansac's minimum of 4 points: None in their slots
    assert pose.compute_pose_batch([good, fisheye], pts, pts, [None, None]) == [None, None]
    assert pose.compute_pose_batch([good, good], pts, pts, [None, None], use_distortion=True, return_inliers=True) == [None, None]
    with pytest.raises(ValueError):
        pose.compute_pose_batch([good], pts, pts, [None, None])             # one entry per message
    with pytest.raises(ValueError):
        pose.compute_pose_batch([good, good], pts, pts, [None, None], ransac_iterations=0)
    assert pose.compute_pose_batch([], [], [], []) == []

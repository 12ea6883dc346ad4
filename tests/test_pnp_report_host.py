"""Report of the pose stage, the parts that need no GPU (DESIGN.md "Report of the pose stage"; the GPU side is tests/test_gpu_pnp_report.py):

  1. the three entry points are declared, exported and bound, and refuse a null context;
  2. the engine's wrappers: alloc_outputs keys on and off, which entry point a call reaches and with which pointers (a recording library);
  3. compute_pose(return_inliers=True) against a stubbed engine: shape and dtype of cv2's `inliers`, the old call untouched when off;
  4. PoseNode(report=True) fills last_report from its one output block, whose read-back keeps its size when the flag is off (a stubbed engine);
  5. the fixed scenes of the GPU tests have STABLE inlier sets: the oracle returns the same set at reproj_error = 8 (1 - 1e-3), 8 and
     8 (1 + 1e-3).  A condition on the inputs, not a tolerance: a scene that fails it is replaced in tests/pnp_report_scenes.py.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import pnp_distorted_ref as ref
import pnp_report_scenes as S
from gisnav_amd.synthetic import K_MATRIX
from oracle import pnp_ransac as pr

HERE = os.path.dirname(os.path.abspath(__file__))
VP, I, D_, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float


# ------------------------------------------------------------------------------------------------------------------ 1
def test_symbols_are_declared_exported_and_bound():
    from gisnav_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(HERE, "..", "include", "gisnav_amd.h")).read())
    tail = r"double sigma_px, double\* cov_rt, double\* sigma_hat, uint8_t\* cov_ok, "
    rep = r"uint8_t\* inlier_mask, int32_t\* inlier_idx, float\* reproj_err, void\* stream\);"
    for name, decl in (("gn_pnp_ransac_report", tail + rep), ("gn_estimate_report", tail + r"int64_t\* idx, float\* score, " + rep),
                       ("gn_vo_estimate_report", tail + r"int64_t\* idx, float\* score, " + rep)):
        assert re.search(r"int " + name + r"\(gn_ctx\* ctx, int B,[^;]*" + decl, header), name
    assert "hypothesis model" in header and "refined" in header          # where the mask and the residual come from is documented
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    f64p = _lib.c_f64p
    want = {"gn_pnp_ransac_report": [VP, I, VP, VP, VP, I, f64p, I, F, D_, I, VP, VP, VP, VP, D_, VP, VP, VP, VP, VP, VP, VP],
            "gn_estimate_report": [VP, I, I, VP, VP, VP, I, VP, VP, VP, I, VP, I, I, f64p, I, VP, VP, VP, VP, VP, D_, VP, VP, VP, VP, VP, VP, VP, VP, VP],
            "gn_vo_estimate_report": [VP, I, I, VP, VP, VP, I, VP, VP, VP, I, f64p, D_, I, VP, VP, VP, VP, VP, D_, VP, VP, VP, VP, VP, VP, VP, VP, VP]}
    lib = _lib.load()
    for name, args in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args
        # the *_cov signature + the report pointers in front of the stream
        cov = _lib.SIGNATURES[name.replace("_report", "_cov")][1]
        assert args[:-1][:len(cov) - 1] == cov[:-1] and len(args) - len(cov) == (3 if name == "gn_pnp_ransac_report" else 5)
        nulls = [0 if a is I else 0.0 if a in (D_, F) else None for a in args]
        assert getattr(lib, name)(*nulls) < 0                            # null context: GN_ERR_ARG, nothing touched


# ------------------------------------------------------------------------------------------------------------------ 2
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
    return e


def _addr(p):
    return None if p is None else (p.value if isinstance(p, ctypes.c_void_p) else p)


def test_engine_wrappers_route_and_allocate():
    from gisnav_amd import _lib
    e = _stub_engine()
    old = ["R", "n_inliers", "n_match", "ok", "t"]
    new = ["idx", "inlier_idx", "inlier_mask", "reproj_err", "score"]
    assert sorted(e.alloc_outputs(3)) == old and sorted(e.alloc_outputs(3, covariance=True)) == sorted(old + ["cov", "cov_ok", "sigma"])
    out = e.alloc_outputs(3, report=True)
    assert sorted(out) == sorted(old + new)
    assert out["idx"].shape == (3, 128, 2) and out["idx"].dtype == torch.int64 and out["score"].dtype == torch.float32
    assert out["inlier_mask"].shape == (3, 128) and out["inlier_mask"].dtype == torch.uint8
    assert out["inlier_idx"].dtype == torch.int32 and out["reproj_err"].dtype == torch.float32 and out["reproj_err"].shape == (3, 128)
    inputs = dict(desc_q=torch.zeros(3, 128, 128), kpt_q=torch.zeros(3, 128, 4), n_q=torch.zeros(3, dtype=torch.int32),
                  desc_r=torch.zeros(3, 128, 128), kpt_r=torch.zeros(3, 128, 4), n_r=torch.zeros(3, dtype=torch.int32),
                  dem=torch.zeros(3, 8, 8, dtype=torch.uint8), kpt_format=_lib.GN_KPT_XYSA)
    # off: the call it always was
    e.estimate(inputs, K_MATRIX)
    e.vo_estimate(inputs, K_MATRIX)
    assert [(n, len(a)) for n, a in e.lib.calls] == [("gn_estimate", 22), ("gn_vo_estimate", 20)]
    e.lib.calls.clear()
    # on: the report entry point, covariance trio null, the five arrays of `out` in front of the stream
    got = e.estimate(inputs, K_MATRIX, out=out, report=True)
    name, a = e.lib.calls.pop()
    assert got is out and name == "gn_estimate_report" and len(a) == 31
    assert [_addr(p) for p in a[22:25]] == [None, None, None]
    assert [_addr(p) for p in a[25:30]] == [out[k].data_ptr() for k in ("idx", "score", "inlier_mask", "inlier_idx", "reproj_err")]
    both = e.estimate(inputs, K_MATRIX, report=True, covariance=True)
    name, a = e.lib.calls.pop()
    assert name == "gn_estimate_report" and [_addr(p) for p in a[22:25]] == [both[k].data_ptr() for k in ("cov", "sigma", "cov_ok")]
    vo = e.vo_estimate(inputs, K_MATRIX, report=True)
    name, a = e.lib.calls.pop()
    assert name == "gn_vo_estimate_report" and len(a) == 29 and _addr(a[23]) == vo["idx"].data_ptr() and _addr(a[27]) == vo["reproj_err"].data_ptr()
    # the PnP stage alone
    obj, img, n = torch.zeros(2, 96, 3), torch.zeros(2, 96, 2), torch.zeros(2, dtype=torch.int32)
    assert len(e.pnp_ransac(obj, img, n, K_MATRIX)) == 4 and e.lib.calls.pop()[0] == "gn_pnp_ransac"
    res = e.pnp_ransac(obj, img, n, K_MATRIX, report=True)
    name, a = e.lib.calls.pop()
    assert name == "gn_pnp_ransac_report" and len(a) == 23 and len(res) == 7
    assert [tuple(x.shape) for x in res[4:]] == [(2, 96)] * 3 and [x.dtype for x in res[4:]] == [torch.uint8, torch.int32, torch.float32]
    assert [_addr(p) for p in a[19:22]] == [x.data_ptr() for x in res[4:]] and a[5] == 96
    only = e.pnp_ransac(obj, img, n, K_MATRIX, report=True, report_out=dict(inlier_idx=res[5]), covariance=True)
    name, a = e.lib.calls.pop()
    assert len(only) == 10 and only[7] is None and only[8] is res[5] and only[9] is None
    assert [_addr(p) for p in a[19:22]] == [None, res[5].data_ptr(), None] and _addr(a[16]) == only[4].data_ptr()


# ------------------------------------------------------------------------------------------------------------------ 3
def test_compute_pose_returns_inliers_as_cv2_does():
    from gisnav_amd.pose import compute_pose
    calls = []
    R, t = np.eye(3), np.arange(3.0).reshape(3, 1)
    inl = np.array([[0], [2], [5]], np.int32)
    err = np.linspace(0, 1, 6).astype(np.float32)

    class Eng:
        kmax = 64

        def pnp_ransac_host(self, obj, img, K, iterations, **kw):
            calls.append(kw)
            res = (R, t, 3, True)
            if kw.get("covariance"):
                res += (np.eye(6), 0.5, True)
            if kw.get("report"):
                res += (inl, err)
            return res
    info = types.SimpleNamespace(k=K_MATRIX.reshape(9))
    pts = np.random.default_rng(0).uniform(10, 100, (6, 2)).astype(np.float32)
    assert len(compute_pose(info, pts, pts, None, engine=Eng())) == 2
    assert "report" not in calls[-1]                                      # off: the engine is called as it always was
    got = compute_pose(info, pts, pts, None, engine=Eng(), return_inliers=True)
    assert calls[-1]["report"] is True and len(got) == 3 and got[0] is R and got[1] is t
    assert got[2].shape == (3, 1) and got[2].dtype == np.int32 and np.array_equal(got[2], inl)
    got = compute_pose(info, pts, pts, None, engine=Eng(), return_covariance=True, return_inliers=True, return_residuals=True)
    assert len(got) == 5 and got[2].shape == (6, 6) and got[3] is inl and got[4] is err
    assert compute_pose(info, pts[:3], pts[:3], None, engine=Eng(), return_inliers=True) is None      # < 4 points: no pose, as before


def test_twist_and_loftr_helpers_keep_their_calls_when_off():
    import inspect
    from gisnav_amd import loftr, vo
    assert loftr._report_kw(False) == {} and loftr._report_kw(True) == {"report": True}
    for f in (vo.twist_pose, loftr.loftr_pose, loftr.loftr_pose_batch):
        assert inspect.signature(f).parameters["return_inliers"].default is False


# ------------------------------------------------------------------------------------------------------------------ 4
def _fake_engine_class(record):
    class FakeEngine:
        def __init__(self, *a, **kw):
            self.device, self.kmax = torch.device("cpu"), 512

        def set_active_kpts(self, n):
            return n

        def estimate(self, inputs, K, min_matches, out=None, covariance=False, sigma_px=0.0, report=False):
            record.append(dict(report=report, keys=sorted(out)))
            out["R"].copy_(torch.eye(3, dtype=torch.float64)[None]); out["t"].fill_(2.0)
            out["n_match"].fill_(40); out["n_inliers"].fill_(3); out["ok"].fill_(1)
            if report:
                out["idx"][0, :40, 0] = torch.arange(40); out["idx"][0, :40, 1] = torch.arange(40) + 5
                out["score"][0, :40] = 0.5
                out["inlier_idx"].fill_(-1); out["inlier_idx"][0, :3] = torch.tensor([1, 7, 39], dtype=torch.int32)
                out["reproj_err"].fill_(-1.0); out["reproj_err"][0, :40] = torch.arange(40, dtype=torch.float32)
            return out
    return FakeEngine


@pytest.mark.parametrize("report", [False, True])
def test_pose_node_fills_last_report_from_its_one_block(monkeypatch, report):
    from gisnav_amd import pose_node, wire
    record, sizes = [], []
    monkeypatch.setattr(pose_node, "PoseEngine", _fake_engine_class(record))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: real_empty(*a, **{k: v for k, v in kw.items() if k != "pin_memory"}))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(synchronize=lambda: None))
    real_bytes = pose_node.PoseNode.out_bytes
    monkeypatch.setattr(pose_node.PoseNode, "out_bytes", staticmethod(lambda *a: sizes.append(real_bytes(*a)) or sizes[-1]))
    rng = np.random.default_rng(0)
    kp_q, kp_r = rng.uniform(0, 400, (60, 2)).astype(np.float32), rng.uniform(0, 400, (50, 2)).astype(np.float32)
    extractor = lambda img: (kp_r, np.zeros((50, 128), np.float32), np.ones(50, np.float32), np.zeros(50, np.float32))  # noqa: E731
    node = pose_node.PoseNode({}, extractor, max_kpts=512, precision="f32", report=report)
    msg = wire.OrthoStereoImage(query_sift=wire.pack_keypoints(kp_q, np.ones(60, np.float32), np.zeros(60, np.float32), np.zeros((60, 128), np.float32)),
                                reference=wire.ImageMsg(np.zeros((8, 8), np.uint8), wire.Stamp(1, 0)), dem=wire.ImageMsg(np.zeros((8, 8), np.uint8), wire.Stamp(1, 0)))
    cam = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    r = node.estimate(cam, msg)
    assert r is not None and np.array_equal(r[0], np.eye(3)) and (r[1] == 2.0).all() and node.last_num_matches == 40
    assert record[-1]["report"] is report
    if not report:
        assert sizes[-1] == 112 and node.last_report is None              # the read-back is the 112 bytes it was
        assert "idx" not in record[-1]["keys"]
        return
    assert sizes[-1] == 416 + 28 * 512
    rep = node.last_report
    assert sorted(rep) == ["inliers", "mkp_qry", "mkp_ref", "reproj_err", "score"]
    assert np.array_equal(rep["mkp_qry"], kp_q[:40]) and np.array_equal(rep["mkp_ref"], kp_r[5:45])
    assert rep["inliers"].shape == (3, 1) and rep["inliers"].dtype == np.int32 and rep["inliers"][:, 0].tolist() == [1, 7, 39]
    assert np.array_equal(rep["reproj_err"], np.arange(40, dtype=np.float32)) and (rep["score"] == 0.5).all() and len(rep["score"]) == 40
    empty = wire.OrthoStereoImage(query_sift=b"", reference=msg.reference, dem=msg.dem)
    assert node.estimate(cam, empty) is None and node.last_report is None


def test_transfer_size_grows_only_with_the_flag():
    from gisnav_amd.pose_node import PoseNode
    assert PoseNode.out_bytes(False, False, 4096) == 112 and PoseNode.out_bytes(True, False, 4096) == 416
    assert PoseNode.out_bytes(False, True, 1024) == PoseNode.out_bytes(True, True, 1024) == 416 + 28 * 1024


# ------------------------------------------------------------------------------------------------------------------ 5
def _stable(solve):
    sets = [solve(S.REPROJ * s) for s in (1 - 1e-3, 1.0, 1 + 1e-3)]
    assert all(r[0] for r in sets)
    return all(np.array_equal(sets[1][3], r[3]) for r in sets), np.asarray(sets[1][3])


def test_one_call_scenes_have_stable_inlier_sets():
    scenes = S.one_call_scenes()
    assert [len(o) for o, _ in scenes] == [4, 5, 12, 63, 65, 130, 300] and S.KSTRIDE == 384 and S.MIN_PTS == 15
    assert sorted({planar for _, (_, _, planar) in S.ONE_CALL}) == [False, True]
    for (o, u), (n, (m, seed, planar)) in zip(scenes, S.ONE_CALL):
        ok, inl = _stable(lambda e, o=o, u=u: pr.solve_pnp_ransac(o, u, S.K, 10, e))
        assert ok, (n, seed)
        if n >= 12:                                                       # every fourth point is displaced by 40 - 120 px, and rejected
            assert np.array_equal(inl, np.nonzero(np.arange(n) % 4 != 3)[0]), n
            assert (planar and not o[:, 2].any()) or (not planar and len(np.unique(o[:, 2])) > 3)
        else:
            assert np.array_equal(inl, np.arange(n))


def test_round_scenes_have_stable_inlier_sets_and_match_the_golden_rows():
    scenes, K = S.round_scenes()
    g = np.load(S.GOLDEN)
    for s, (o, u) in zip(S.ROUND_SCENES, scenes):
        assert len(o) == 60
        ok, inl = _stable(lambda e, o=o, u=u: pr.solve_pnp_ransac(o, u, K, S.ROUND_COUNT, e))
        i = list(g[f"{s}_counts"]).index(S.ROUND_COUNT)
        assert ok and np.array_equal(np.nonzero(g[f"{s}_inl"][i])[0], inl), s


def test_distorted_scenes_have_stable_inlier_sets():
    assert len(S.DIST_SCENES) == 3 and np.array_equal(S.D, ref.D_TEST)
    for (o, u), key in zip(S.dist_scenes(), S.DIST_SCENES):
        ok, inl = _stable(lambda e, o=o, u=u: ref.solve_pnp_ransac_dist(o, u, S.K, S.D, 10, e))
        assert ok and len(inl) >= S.MIN_PTS, key

"""Lens distortion (distCoeffs) in the PnP stage on the GPU: gn_set_distortion / gn_get_distortion / gn_undistort_points (DESIGN.md "Lens distortion").

  1. gn_undistort_points is the five-step cv::undistortPoints, not the converged one; off it is (u - cx) / fx; slots past n_pts are untouched;
  2. off means off: unset, and five zeros, give byte-identical gn_pnp_ransac_cov outputs;
  3. parity with the fp64 restatement (tests/pnp_distorted_ref.py) on 24 scenes with outliers, plus the 4- and 5-point branches; the poses reach
     ground truth, and the same inputs solved with distortion off miss it;
  4. the covariance against s^2 (J^T J)^-1 from the restatement's Jacobian;
  5. through gn_estimate_cov with sub-streams and overlap: bitwise the staged match -> gather_points -> pnp_ransac;
  6. the coefficients are captured per call: two pipelined calls with deferred join, D then off;
  7. argument errors.
"""
import dataclasses

import numpy as np
import pytest
import torch

import pnp_distorted_ref as ref
from gisnav_amd import _lib
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu

K, D = ref.K_TEST, ref.D_TEST
SIZES, SEEDS = (16, 24, 64), (1, 2, 3, 4)


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=16, max_kpts=128)
    yield e
    del e


def _stage(eng, scenes, stride):
    B = len(scenes)
    obj, img, n = np.zeros((B, stride, 3), np.float32), np.zeros((B, stride, 2), np.float32), np.zeros(B, np.int32)
    for b, (o, u) in enumerate(scenes):
        obj[b, :len(o)], img[b, :len(o)], n[b] = o, u, len(o)
    d = eng.device
    return torch.from_numpy(obj).to(d), torch.from_numpy(img).to(d), torch.from_numpy(n).to(d)


@pytest.fixture(scope="module")
def scenes():
    """{planar: [(obj, img, rvec, tvec, inlier mask)] for the 12 scenes, then the first 4 and the first 5 inliers of scene (24, seed 1)}."""
    out = {}
    for planar in (True, False):
        s = [ref.make_scene(n, seed, planar) for n in SIZES for seed in SEEDS]
        o, u, rv, tv, inl = s[4]
        for k in (4, 5):
            s.append((o[inl][:k], u[inl][:k], rv, tv, np.ones(k, bool)))
        out[planar] = s
    return out


@pytest.fixture(scope="module")
def solved(eng, scenes):
    """One gn_pnp_ransac_cov call per planarity with D set (B = 14, kstride = 64), one with distortion off; the restatement's results."""
    res = {}
    for planar, s in scenes.items():
        obj, img, n = _stage(eng, [(o, u) for o, u, *_ in s], 64)
        eng.set_distortion(D)
        on = [x.cpu().numpy() for x in eng.pnp_ransac(obj, img, n, K, min_pts=4, covariance=True, sigma_px=0.5)]
        eng.set_distortion(None)
        off = [x.cpu().numpy() for x in eng.pnp_ransac(obj, img, n, K, min_pts=4)]
        want = [ref.solve_pnp_ransac_dist(o, u, K, D) for o, u, *_ in s]
        res[planar] = (on, off, want)
    return res


# ------------------------------------------------------------------------------------------------------------------ 1
def _grid(nx, ny):
    u, v = np.meshgrid(np.linspace(0, 640, nx), np.linspace(0, 480, ny))
    return np.column_stack([u.reshape(-1), v.reshape(-1)]).astype(np.float32)


@pytest.mark.parametrize("to_pixels", [False, True])
def test_undistort_points_is_the_five_step_iteration(eng, to_pixels):
    pts = [_grid(9, 7), _grid(13, 5)]                                   # 63 and 65 points over the whole frame, corners included
    assert [len(p) for p in pts] == [63, 65]
    img = np.zeros((2, 128, 2), np.float32)
    rng = np.random.default_rng(0)
    img[:] = rng.uniform(0, 640, img.shape)                             # live-looking values past n_pts: they must not be touched
    for b, p in enumerate(pts):
        img[b, :len(p)] = p
    dev = eng.device
    img_d, n_d = torch.from_numpy(img).to(dev), torch.tensor([63, 65], dtype=torch.int32, device=dev)
    fxy, cxy = np.array([K[0, 0], K[1, 1]]), np.array([K[0, 2], K[1, 2]])
    eng.set_distortion(D)
    try:
        assert np.array_equal(eng.distortion(), D)
        got = eng.undistort_points(img_d, n_d, K, to_pixels, out=torch.full((2, 128, 2), 7.0, dtype=torch.float32, device=dev)).cpu().numpy()
    finally:
        eng.set_distortion(None)
    assert eng.distortion() is None
    off = eng.undistort_points(img_d, n_d, K, to_pixels, out=torch.full((2, 128, 2), 7.0, dtype=torch.float32, device=dev)).cpu().numpy()
    for b, p in enumerate(pts):
        n = len(p)
        assert np.all(got[b, n:] == 7.0) and np.all(off[b, n:] == 7.0)                  # slots past n_pts untouched
        u5, u50 = ref.undistort(p, K, D), ref.undistort(p, K, D, steps=50)
        plain = (p.astype(np.float64) - cxy) / fxy
        if to_pixels:
            u5, u50, plain = u5 * fxy + cxy, u50 * fxy + cxy, plain * fxy + cxy
        want = u5.astype(np.float32)
        ulps = np.abs(got[b, :n].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"to_pixels={to_pixels} pair {b}: largest distance from the f32-rounded restatement {ulps.max():.2f} ulp")
        assert ulps.max() <= 1.0
        corners = [0, int(np.argmax(p[:, 0] + p[:, 1])), int(np.argmax(p[:, 0] - p[:, 1])), int(np.argmax(p[:, 1] - p[:, 0]))]
        gap = np.abs(got[b, corners].astype(np.float64) - u50[corners]).max(axis=1) * (1.0 if to_pixels else K[0, 0])
        print(f"to_pixels={to_pixels} pair {b}: corners against the converged undistortion {gap} px")
        assert gap.min() > 0.5                                                         # five steps, not the fixed point
        if not to_pixels:
            assert np.array_equal(off[b, :n], plain.astype(np.float32))                 # off: the K^-1 the solvers always applied, exactly
        else:
            # x fx + cx is one fused multiply-add on the GPU: the double differs from numpy's by <= 1 ulp of 640 (1.1e-13), which shows as
            # one f32 rounding flip, or as ~1e-14 px where the result cancels to zero (u = 0): one f32 ulp of max(|value|, 1)
            p32 = plain.astype(np.float32)
            assert np.all(np.abs(off[b, :n].astype(np.float64) - p32) <= np.spacing(np.maximum(np.abs(p32), np.float32(1.0))))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_off_means_off(eng, scenes):
    o, u, _, _, inl = ref.make_scene(40, 1, False)
    batch = [(o[inl][:4], u[inl][:4]), (o[inl][:5], u[inl][:5]), (o, u)]
    obj, img, n = _stage(eng, batch, 64)
    assert n.tolist() == [4, 5, 40]
    fresh = type(eng)(0, max_batch=4, max_kpts=128)                     # a context that never saw gn_set_distortion
    run = lambda e: [x.cpu().numpy().tobytes() for x in e.pnp_ransac(obj, img, n, K, min_pts=4, covariance=True)]  # noqa: E731
    before = run(fresh)
    fresh.set_distortion(D)
    with_d = run(fresh)
    fresh.set_distortion(None)
    unset = run(fresh)
    fresh.set_distortion(np.zeros(5))
    assert fresh.distortion() is None                                   # all zeros count as off
    zeros = run(fresh)
    del fresh
    assert before == unset and before == zeros
    assert with_d[0] != before[0]                                       # (and D does change the pose)


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("planar", [True, False])
def test_parity_with_the_restatement_and_ground_truth(scenes, solved, planar):
    """dR < 1e-8 (Frobenius) and dt < 1e-8 (relative) against the restatement: the bar of test_pnp_inlier_count_and_pose_against_oracle.  Against
    ground truth max |d(rvec, tvec)| <= 2e-4 on the 12 scenes (the restatement alone: <= 8.9e-5, the f32 rounding of the observations); the
    same inputs solved with distortion off miss t by more than 1."""
    on, off, want = solved[planar]
    R, t, n_inl, ok = on[:4]
    worst = [0.0, 0.0, 0.0]
    for b, (o, u, rv, tv, inl) in enumerate(scenes[planar]):
        w_ok, w_r, w_t, w_inl = want[b]
        assert w_ok and ok[b] == 1, (planar, b)
        assert n_inl[b] == len(w_inl) == int(inl.sum()), (planar, b, n_inl[b], len(w_inl))
        dR = np.linalg.norm(R[b] - pr.rodrigues_vec2mat(w_r))
        dt = np.linalg.norm(t[b] - w_t) / np.linalg.norm(w_t)
        line = f"planar={planar} scene {b} (n = {len(o)}): dR {dR:.2e} dt {dt:.2e}"
        worst[0], worst[1] = max(worst[0], dR), max(worst[1], dt)
        if b < 12:
            gt = max(np.abs(pr.rodrigues_mat2vec(R[b]) - rv).max(), np.abs(t[b].reshape(3) - tv).max())
            miss = np.linalg.norm(off[1][b].reshape(3) - tv)
            line += f" | against ground truth {gt:.2e} | distortion off misses t by {miss:.2f}"
            worst[2] = max(worst[2], gt)
        print(line)
    print(f"planar={planar}: worst dR {worst[0]:.3e}, dt {worst[1]:.3e}, against ground truth {worst[2]:.3e}")
    for b, (o, u, rv, tv, inl) in enumerate(scenes[planar]):
        w_ok, w_r, w_t, w_inl = want[b]
        assert np.linalg.norm(R[b] - pr.rodrigues_vec2mat(w_r)) < 1e-8, (planar, b)
        assert np.linalg.norm(t[b] - w_t) / np.linalg.norm(w_t) < 1e-8, (planar, b)
        if b < 12:
            assert max(np.abs(pr.rodrigues_mat2vec(R[b]) - rv).max(), np.abs(t[b].reshape(3) - tv).max()) <= 2e-4, (planar, b)
            assert np.linalg.norm(off[1][b].reshape(3) - tv) > 1.0, (planar, b)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_covariance_uses_the_distorted_forward_model(scenes, solved):
    """cov_rt against 0.25 (J^T J)^-1 from the restatement's Jacobian over the restatement's inliers at the returned pose: scaled difference <= 1e-9
    (the bound of tests/test_gpu_pose_covariance.py).  Scenes: (64, seed 1) planar and non-planar."""
    for planar in (True, False):
        b = 8
        o, u, *_ = scenes[planar][b]
        on, _, want = solved[planar]
        R, t, _, _, cov, sigma, cov_ok = on
        inl = np.asarray(want[b][3]).reshape(-1)
        assert cov_ok[b] == 1
        proj, J = ref.project_points_dist(o[inl].astype(np.float64), pr.rodrigues_mat2vec(R[b]), t[b].reshape(3), K, D, True)
        e = (proj - u[inl].astype(np.float64)).reshape(-1)
        w = 0.25 * np.linalg.inv(J.T @ J)
        s_hat = np.sqrt(float(e @ e) / (2 * len(inl) - 6))
        d = np.sqrt(np.diag(w))
        diff = float((np.abs(cov[b] - w) / np.outer(d, d)).max())
        print(f"planar={planar}: scaled covariance difference {diff:.3e}, sigma_hat {sigma[b]:.3e} (fp64 {s_hat:.3e})")
        assert diff <= 1e-9
        assert abs(sigma[b] - s_hat) <= 1e-10 * s_hat + 1e-14
        # the pinhole Jacobian at the same pose is a different matrix: the check above discriminates
        _, J0 = pr.project_points(o[inl].astype(np.float64), pr.rodrigues_mat2vec(R[b]), t[b].reshape(3), K, True)
        assert float((np.abs(0.25 * np.linalg.inv(J0.T @ J0) - w) / np.outer(d, d)).max()) > 1e-4


# ------------------------------------------------------------------------------------------------------------------ 5, 6
KEYS = ("R", "t", "n_match", "n_inliers", "ok", "cov", "sigma", "cov_ok")


def _distorted_pair(idx, n_q, n_r):
    p = make_pair(idx, n_q=n_q, n_r=n_r)
    xn = (p.kp_q.astype(np.float64) - K_MATRIX[:2, 2]) / np.array([K_MATRIX[0, 0], K_MATRIX[1, 1]])
    xd, yd = ref.distort(xn[:, 0], xn[:, 1], D)
    kp = np.column_stack([xd * K_MATRIX[0, 0] + K_MATRIX[0, 2], yd * K_MATRIX[1, 1] + K_MATRIX[1, 2]]).astype(np.float32)
    return dataclasses.replace(p, kp_q=kp)


@pytest.fixture(scope="module")
def small():
    """The suite's small context: 256 keypoints, synthetic weights, B = 4; query keypoints at their distorted positions."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    e = PoseEngine(0, max_batch=4, max_kpts=256, precision="f32", state_dict=synthetic_state_dict(0))
    pairs = [_distorted_pair(7300 + i, 256 - 9 * i, 256 - 5 * i) for i in range(4)]
    inp = e.stage_inputs(pairs)
    yield e, inp
    del e


def _staged(e, inp, d):
    from gisnav_amd.engine import MIN_MATCHES
    e.set_distortion(d)
    try:
        idx, _, n_match = e.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        mkp, obj = e.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
        R, t, n_inl, ok, cov, sigma, cov_ok = e.pnp_ransac(obj, mkp, n_match, K_MATRIX, min_pts=MIN_MATCHES, covariance=True)
        torch.cuda.synchronize()
    finally:
        e.set_distortion(None)
    return {k: v.clone() for k, v in dict(R=R, t=t, n_match=n_match, n_inliers=n_inl, ok=ok, cov=cov, sigma=sigma, cov_ok=cov_ok).items()}


def _diff(got, want):
    return [k for k in KEYS if not torch.equal(got[k].reshape(want[k].shape), want[k])]


def test_estimate_with_substreams_and_overlap_equals_the_staged_path_bitwise(small):
    e, inp = small
    want, want_off = _staged(e, inp, D), _staged(e, inp, None)
    assert int(want["ok"].sum()) == 4 and int(want["cov_ok"].sum()) == 4
    assert not torch.equal(want["R"], want_off["R"])                    # the coefficients reach this path's PnP
    out = e.alloc_outputs(4, covariance=True)
    try:
        e.set_distortion(D)
        e.set_substreams(2)
        e.set_overlap(True)
        e.estimate(inp, K_MATRIX, out=out, covariance=True)
        e.flush()
        torch.cuda.synchronize()
    finally:
        e.flush()
        e.set_overlap(False)
        e.set_substreams(1)
        e.set_distortion(None)
    assert not _diff(out, want), _diff(out, want)


def test_coefficients_are_captured_per_call(small):
    e, inp = small
    want_d, want_off = _staged(e, inp, D), _staged(e, inp, None)
    out1, out2 = e.alloc_outputs(4, covariance=True), e.alloc_outputs(4, covariance=True)
    try:
        e.set_substreams(2, deferred_join=True)
        e.set_distortion(D)
        e.estimate(inp, K_MATRIX, out=out1, covariance=True)
        e.set_distortion(None)                                          # before the first call's PnP has been joined
        e.estimate(inp, K_MATRIX, out=out2, covariance=True)
        e.flush()
        torch.cuda.synchronize()
    finally:
        e.flush()
        e.set_substreams(1)
        e.set_distortion(None)
    assert not _diff(out1, want_d), _diff(out1, want_d)
    assert not _diff(out2, want_off), _diff(out2, want_off)


# ------------------------------------------------------------------------------------------------------------------ 7
def test_argument_errors(eng):
    lib = _lib.load()
    eng.set_distortion(D)
    try:
        for bad in (np.zeros(8), np.array([0.1, np.nan, 0.0, 0.0, 0.0])):
            a = np.ascontiguousarray(bad, np.float64)
            rc = lib.gn_set_distortion(eng.ctx, a.ctypes.data_as(_lib.c_f64p), len(a))
            assert rc < 0 and rc == lib.gn_set_distortion(None, None, 0)           # GN_ERR_ARG
            assert len(lib.gn_last_error(eng.ctx)) > 0
            assert np.array_equal(eng.distortion(), D)                                # a refused call leaves the state as it was
        with pytest.raises(_lib.GnError, match="not built"):
            eng.set_distortion(np.zeros(12))
        eng.set_distortion(D[:4])
        assert np.array_equal(eng.distortion(), D)                                    # four coefficients: k3 = 0 (D's k3 is 0)
    finally:
        eng.set_distortion(None)


# ------------------------------------------------------------------------------------------------------------------ the host seam
def test_compute_pose_reads_camera_info_d_only_when_asked(eng, scenes, solved):
    """compute_pose(..., use_distortion=True) = the batched call with D, bit for bit; the default ignores d; the engine's state is restored."""
    from gisnav_amd import wire
    from gisnav_amd.pose import compute_pose
    b = 8                                                               # (64, seed 1), non-planar: integer heights from a raster
    o, u, *_ = scenes[False][b]
    on, off, _ = solved[False]
    dem = np.zeros((480, 640), np.uint8)
    cell = np.floor(o[:, :2]).astype(int)
    dem[cell[:, 1], cell[:, 0]] = o[:, 2].astype(np.uint8)
    info = wire.CameraInfo(k=K.reshape(9), height=480, width=640, d=D, distortion_model="plumb_bob")
    R, t, cov = compute_pose(info, u, o[:, :2], dem, engine=eng, return_covariance=True, sigma_px=0.5, use_distortion=True)
    assert eng.distortion() is None
    assert np.array_equal(R, on[0][b]) and np.array_equal(t, on[1][b]) and np.array_equal(cov, on[4][b])
    R0, t0 = compute_pose(info, u, o[:, :2], dem, engine=eng)
    assert np.array_equal(R0, off[0][b]) and np.array_equal(t0, off[1][b])
    eng.set_distortion(D[:4])
    try:                                                                # dist= overrides the engine's state for one call and puts it back
        res = eng.pnp_ransac_host(o, u, K, dist=np.zeros(0))
        assert np.array_equal(eng.distortion(), D) and np.array_equal(res[0], off[0][b])
    finally:
        eng.set_distortion(None)

"""Pose covariance, host side (DESIGN.md "Pose covariance"): `gn_pose_cov_to_camera` and `gn_pose_cov_to_earth` against fp64 central-difference
Jacobians written here, and the function that fills the outgoing PoseWithCovarianceStamped, driven with stand-in objects.  Host code only --
runs without a GPU."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import georef as og  # noqa: E402
from oracle import pnp_ransac as pr  # noqa: E402

SHAPE = (480, 640)


def _crs(lon0=24.94, lat0=60.17, rot_deg=12.0, mpp=1.0):
    """A plausible OrthoStereoImage CRS, built like `_crs` of tests/test_georef.py: rotated / scaled pixel grid -> (lon, lat, alt), z flipped."""
    a = np.radians(rot_deg)
    dlat = mpp / 111_320.0; dlon = dlat / np.cos(np.radians(lat0))
    M = np.array([[np.cos(a) * dlon, np.sin(a) * dlon, 0.0, lon0], [np.sin(a) * dlat, -np.cos(a) * dlat, 0.0, lat0], [0.0, 0.0, -mpp, 12.5]])
    return og.affine_to_proj(M), M


def _cov_rt(rng):
    """A symmetric positive definite covariance of (rvec, tvec) with the standard deviations a 64-point PnP has (rad, raster px), correlated."""
    s = np.array([6e-4, 5e-4, 3e-4, 0.2, 0.2, 0.08])
    A = rng.normal(size=(6, 6))
    return np.diag(s) @ (0.5 * np.eye(6) + 0.5 * (A @ A.T) / 6) @ np.diag(s)


def _scaled_diff(got, want):
    d = np.sqrt(np.diag(want))
    return float((np.abs(got - want) / np.outer(d, d)).max())


def _camera_jacobian_fd(rvec, tvec):
    """d(c, phi) / d(rvec, tvec) by central differences: c = -R^T t, phi = the skew part of R'_wc R_wc^T (rodrigues_mat2vec returns 0 for
    tiny angles, so the increment is read off the matrix)."""
    R0 = pr.rodrigues_vec2mat(rvec)

    def f(x):
        Rm = pr.rodrigues_vec2mat(x[:3])
        dR = Rm.T @ R0                                   # R'_wc R_wc^T = Exp(phi)
        W = 0.5 * (dR - dR.T)
        return np.concatenate([-Rm.T @ x[3:], [W[2, 1], W[0, 2], W[1, 0]]])
    x0 = np.concatenate([rvec, tvec])
    J = np.zeros((6, 6))
    for k in range(6):
        h = 1e-6 * max(1.0, abs(x0[k]))
        xp, xm = x0.copy(), x0.copy()
        xp[k] += h; xm[k] -= h
        J[:, k] = (f(xp) - f(xm)) / (2 * h)
    return J


def _poses(rng, n, spread):
    out = []
    for _ in range(n):
        rv = rng.normal(0, spread, 3); rv[2] += rng.uniform(-3, 3)
        rv = pr.rodrigues_mat2vec(pr.rodrigues_vec2mat(rv))       # the solver's rvec is cv2.Rodrigues of R: the principal one, |rvec| <= pi
        cam = np.array([rng.uniform(100, 400), rng.uniform(100, 500), -rng.uniform(80, 400)])     # camera centre in raster coordinates
        out.append((rv, -pr.rodrigues_vec2mat(rv) @ cam))
    return out


def test_camera_covariance_matches_a_central_difference_jacobian():
    """cov_cam = A cov_rt A^T with A from central differences of (rvec, tvec) -> (c, phi).  Bound 1e-7 on max |dS_ij| / sqrt(S_ii S_jj): the
    difference quotient's rounding error is eps |f| / h = 1.1e-16 * 600 px / 1e-6 = 7e-8 px / rad on entries of size |c| ~ 300 px / rad (2e-10
    relative, its truncation error h^2 ~ 1e-12 is below that), so a covariance built from it is good to ~1e-9 of its scale; 1e-7 leaves two
    orders of margin and a wrong sign or a left / right Jacobian mix-up shows at order 1."""
    from gisnav_amd import georef as gg
    rng = np.random.default_rng(5)
    poses = _poses(rng, 12, 0.4)
    poses.append((np.zeros(3), np.array([-250.0, -200.0, 300.0])))                  # rvec = 0: the small-angle branch of the closed form
    poses.append((np.array([1e-7, -2e-7, 5e-8]), np.array([-250.0, -200.0, 300.0])))
    poses.append((np.array([0.02, -0.01, 3.1]), np.array([300.0, 200.0, 250.0])))   # close to pi
    worst = 0.0
    for rv, tv in poses:
        R, cov_rt = pr.rodrigues_vec2mat(rv), _cov_rt(rng)
        A = _camera_jacobian_fd(rv, tv)
        want = A @ cov_rt @ A.T
        got = gg.pose_cov_to_camera(R, tv, cov_rt)
        assert np.array_equal(got, got.T)
        assert np.linalg.eigvalsh(got).min() > 0
        worst = max(worst, _scaled_diff(got, want))
    print(f"camera covariance vs central differences: worst scaled difference {worst:.2e}")
    assert worst <= 1e-7, worst


def _qmul(a, b):
    x1, y1, z1, w1 = a; x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def _earth_jacobian_fd(R, t, crs, hp, hr):
    """d(ecef, psi) / d(c, phi) by central differences through oracle.georef.pose_to_earth: R_wc -> Exp(phi) R_wc, c -> c + dc, psi read off
    q' (x) conj(q) (q_true = dq(psi) (x) q_est)."""
    Rwc = R.T
    c = -Rwc @ t
    q0 = np.asarray(og.pose_to_earth(R, t.reshape(3, 1), crs, SHAPE)["orientation"])
    q0i = q0 * np.array([-1, -1, -1, 1])

    def f(dc, dphi):
        Rn = (pr.rodrigues_vec2mat(dphi) @ Rwc).T
        o = og.pose_to_earth(Rn, (-Rn @ (c + dc)).reshape(3, 1), crs, SHAPE)
        q = np.asarray(o["orientation"])
        if q @ q0 < 0:
            q = -q
        return np.concatenate([np.asarray(o["position"]).reshape(3), 2 * _qmul(q, q0i)[:3]])
    J = np.zeros((6, 6))
    for k in range(6):
        h = hp if k < 3 else hr
        e = np.zeros(6); e[k] = h
        J[:, k] = (f(e[:3], e[3:]) - f(-e[:3], -e[3:])) / (2 * h)
    return J


def test_earth_covariance_matches_central_differences_through_the_oracle_map():
    """Three CRSs (rotation 12 / 75 / 200 degrees, 1.0 / 0.3 / 2.5 m per px), five poses each; steps 1e-3 px / 1e-6 rad.  Criterion
    max |dS_ij| / sqrt(S_ii S_jj) <= 1e-4: two such finite-difference Jacobians with steps 30 x apart agree to 1.1e-5 on these inputs, the bound is
    ten times that."""
    from gisnav_amd import georef as gg
    rng = np.random.default_rng(0)
    worst = 0.0
    for rot, mpp in [(12.0, 1.0), (75.0, 0.3), (200.0, 2.5)]:
        crs, _ = _crs(rot_deg=rot, mpp=mpp)
        for rv, tv in _poses(rng, 5, 0.1):
            R, cov_rt = pr.rodrigues_vec2mat(rv), _cov_rt(rng)
            A = _camera_jacobian_fd(rv, tv)
            Je = _earth_jacobian_fd(R, tv, crs, 1e-3, 1e-6)
            want = Je @ (A @ cov_rt @ A.T) @ Je.T
            d = gg.pose_to_earth(R, tv.reshape(3, 1), crs, SHAPE, cov_rt=cov_rt)
            plain = gg.pose_to_earth(R, tv.reshape(3, 1), crs, SHAPE)
            assert d is not None and all(np.array_equal(d[k], plain[k]) for k in plain)      # the pose fields do not change
            got = d["covariance"]
            assert got.shape == (6, 6) and np.array_equal(got, got.T)
            w = np.linalg.eigvalsh(got)
            assert w.min() >= -1e-12 * w.max()
            # position standard deviations are metres: those of the camera centre in raster px times the metres per pixel (to the few 1e-3 the
            # map's scale differs between the raster's axes)
            cam = gg.pose_cov_to_camera(R, tv, cov_rt)
            assert abs(np.sqrt(np.trace(got[:3, :3]) / np.trace(cam[:3, :3])) / mpp - 1) < 1e-2
            worst = max(worst, _scaled_diff(got, want))
    print(f"earth covariance vs central differences: worst scaled difference {worst:.2e}")
    assert worst <= 1e-4, worst


def test_earth_covariance_reports_a_camera_outside_the_raster_like_the_pose():
    from gisnav_amd import _lib
    from gisnav_amd import georef as gg
    lib = _lib.load()
    rng = np.random.default_rng(1)
    crs, M = _crs()
    p = lambda a: a.ctypes.data_as(_lib.c_f64p)  # noqa: E731
    n_out = 0
    for i in range(40):
        rv = rng.normal(0, 0.4, 3); rv[2] += rng.uniform(-3, 3)
        R = pr.rodrigues_vec2mat(rv)
        cam = np.array([rng.uniform(-40, 520), rng.uniform(-40, 680), -rng.uniform(80, 400)])
        t = -R @ cam
        cov_rt = _cov_rt(rng)
        R9, t3, c36, aff = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t), np.ascontiguousarray(cov_rt.reshape(36)), np.ascontiguousarray(M.reshape(12))
        pos, q, out = np.zeros(3), np.zeros(4), np.full(36, -7.0)
        rc_pose = lib.gn_pose_to_earth(p(R9), p(t3), p(aff), SHAPE[0], SHAPE[1], p(pos), p(q), None)
        rc_cov = lib.gn_pose_cov_to_earth(p(R9), p(t3), p(c36), p(aff), SHAPE[0], SHAPE[1], p(out))
        assert rc_cov == rc_pose and rc_pose in (0, 1)
        if rc_pose == 1:
            n_out += 1
            assert (out == -7.0).all()
            assert gg.pose_to_earth(R, t, crs, SHAPE, cov_rt=cov_rt) is None
    assert 2 < n_out < 38                       # both branches exercised


def _blank_message():
    ns = types.SimpleNamespace
    return ns(header=ns(frame_id="", stamp=ns(sec=0, nanosec=0)),
              pose=ns(pose=ns(position=ns(x=0.0, y=0.0, z=0.0), orientation=ns(x=0.0, y=0.0, z=0.0, w=1.0)), covariance=[0.0] * 36))


def test_message_filling_writes_the_covariance_row_major_and_leaves_zeros_without_one():
    from gisnav_amd import ros2_node as rn
    from gisnav_amd.wire import Stamp
    rng = np.random.default_rng(2)
    crs, _ = _crs()
    rv = np.array([0.05, -0.03, 0.7])
    R = pr.rodrigues_vec2mat(rv)
    t = -R @ np.array([240.0, 320.0, -200.0])
    cov_rt = _cov_rt(rng)
    # cov_ok = 1: PoseNode.last_covariance is the 6x6 array
    fields = rn.pose_fields(R, t.reshape(3, 1), crs, SHAPE, cov_rt=cov_rt)
    msg = rn.fill_pose_message(_blank_message(), fields, Stamp(41, 7))
    assert msg.header.frame_id == "earth" and (msg.header.stamp.sec, msg.header.stamp.nanosec) == (41, 7)
    assert (msg.pose.pose.position.x, msg.pose.pose.position.y, msg.pose.pose.position.z) == tuple(float(v) for v in fields["position"])
    o = msg.pose.pose.orientation
    assert (o.x, o.y, o.z, o.w) == tuple(float(v) for v in fields["orientation"])
    assert isinstance(msg.pose.covariance, list) and len(msg.pose.covariance) == 36 and all(type(v) is float for v in msg.pose.covariance)
    assert np.array_equal(np.array(msg.pose.covariance).reshape(6, 6), fields["covariance"])
    assert msg.pose.covariance[0 * 6 + 3] == fields["covariance"][0, 3] and msg.pose.covariance[3 * 6 + 0] == fields["covariance"][3, 0]
    assert msg.pose.covariance[0] > 0 and msg.pose.covariance[35] > 0
    # cov_ok = 0: last_covariance is None, the field keeps its zeros and everything else is filled as before
    fields0 = rn.pose_fields(R, t.reshape(3, 1), crs, SHAPE, cov_rt=None)
    assert "covariance" not in fields0
    msg0 = rn.fill_pose_message(_blank_message(), fields0, Stamp(41, 7))
    assert msg0.pose.covariance == [0.0] * 36
    assert msg0.pose.pose.position.x == msg.pose.pose.position.x and msg0.pose.pose.orientation.w == msg.pose.pose.orientation.w
    # the default keeps pose_fields' result what it was
    plain = rn.pose_fields(R, t.reshape(3, 1), crs, SHAPE)
    assert sorted(plain) == ["lonlatalt", "orientation", "position"]

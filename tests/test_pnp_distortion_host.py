"""Lens distortion in the PnP stage, the parts that need no GPU (DESIGN.md "Lens distortion"; the GPU side is tests/test_gpu_pnp_distortion.py).

  1. tests/pnp_distorted_ref.py with d = 0 returns exactly oracle.pnp_ransac.solve_pnp_ransac's result;
  2. forward model against undistortion: round trip <= 1e-12 px after 50 steps; five steps stop short of it at the frame corners;
  3. the analytic Jacobian of the forward model against central differences;
  4. gn_set_distortion / gn_get_distortion / gn_undistort_points resolve in the built library with the argument types _lib.py declares;
  5. wire.CameraInfo defaults, the ValueError for an unsupported model, camera_info_from_ros copying d.
"""
import ctypes
import types

import numpy as np
import pytest

from oracle import pnp_ransac as pr
import pnp_distorted_ref as ref

K, D = ref.K_TEST, ref.D_TEST


@pytest.mark.parametrize("n,seed,planar", [(24, 1, True), (24, 2, False), (64, 3, False), (16, 4, True)])
def test_restatement_with_zero_coefficients_is_the_oracle_exactly(n, seed, planar):
    obj, img, _, _, _ = ref.make_scene(n, seed, planar, d=np.zeros(5))
    for d in (np.zeros(5), np.zeros(4), None):
        want = pr.solve_pnp_ransac(obj, img, K)
        got = ref.solve_pnp_ransac_dist(obj, img, K, d)
        assert want[0] and got[0]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_restatement_with_zero_coefficients_is_the_oracle_on_four_and_five_points():
    obj, img, _, _, inl = ref.make_scene(24, 1, False, d=np.zeros(5))
    for k in (4, 5):
        o, u = obj[inl][:k], img[inl][:k]
        want, got = pr.solve_pnp_ransac(o, u, K), ref.solve_pnp_ransac_dist(o, u, K, np.zeros(5))
        assert want[0] and got[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    proj, J = pr.project_points(obj.astype(np.float64), [0.03, -0.02, 0.1], [1.0, 2.0, 380.0], K, True)
    proj_d, J_d = ref.project_points_dist(obj.astype(np.float64), [0.03, -0.02, 0.1], [1.0, 2.0, 380.0], K, np.zeros(5), True)
    assert np.array_equal(proj, proj_d) and np.array_equal(J, J_d)


def _frame_grid():
    u, v = np.meshgrid(np.linspace(0, 640, 9), np.linspace(0, 480, 7))
    return np.column_stack([u.reshape(-1), v.reshape(-1)])          # 63 points, the four corners included


def test_forward_model_inverts_the_converged_undistortion_and_five_steps_stop_short():
    px = _frame_grid()
    und50 = ref.undistort(px, K, D, steps=50)
    xd, yd = ref.distort(und50[:, 0], und50[:, 1], D)
    back = np.column_stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]])
    print("converged undistortion -> forward model, against the pixels [px]:", np.abs(back - px).max())
    assert np.abs(back - px).max() <= 1e-12
    und5 = ref.undistort(px, K, D)
    gap = np.abs(und5 - und50).max(axis=1) * K[0, 0]
    corners = [0, 8, 54, 62]
    print("5-step against converged undistortion [px]: corners", gap[corners], "| whole grid max", gap.max())
    assert gap[corners].min() > 0.5                                 # five steps are most of a pixel short of the fixed point at the corners
    assert np.array_equal(ref.undistort(px, K, D[:4]), und5)        # four coefficients: k3 = 0


def test_round_trip_is_at_most_1e_12_px_after_50_steps():
    """Forward then 50 undistortion steps, over the frame: the fixed point is reached to <= 1e-12 px."""
    px = _frame_grid()
    x0, y0 = (px[:, 0] - K[0, 2]) / K[0, 0] * 0.8, (px[:, 1] - K[1, 2]) / K[1, 1] * 0.8
    xd, yd = ref.distort(x0, y0, D)
    pix = np.column_stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]])
    back = ref.undistort(pix, K, D, steps=50)
    err_px = np.abs(back - np.column_stack([x0, y0])).max() * K[0, 0]
    print("round trip after 50 steps [px]:", err_px)
    assert err_px <= 1e-12


def test_analytic_jacobian_against_central_differences():
    obj, _, rvec, tvec, _ = ref.make_scene(24, 2, False)
    obj = obj.astype(np.float64)
    p0 = np.concatenate([rvec, tvec])
    _, J = ref.project_points_dist(obj, p0[:3], p0[3:], K, D, True)
    worst = 0.0
    for k in range(6):
        h = 1e-6 * max(1.0, abs(p0[k]))
        e = np.zeros(6); e[k] = h
        num = (ref.project_points_dist(obj, (p0 + e)[:3], (p0 + e)[3:], K, D) - ref.project_points_dist(obj, (p0 - e)[:3], (p0 - e)[3:], K, D)).reshape(-1) / (2 * h)
        worst = max(worst, float(np.abs(num - J[:, k]).max() / max(1.0, np.abs(J[:, k]).max())))
    print("analytic against central differences, relative to the column's largest entry:", worst)
    # central differences with h = 1e-6: truncation h^2 f''' ~ 1e-12, round-off eps |u| / h ~ 2.2e-16 * 640 / 1e-6 = 1.4e-7 absolute
    assert worst <= 1e-6
    # and the 2 x 2 block of the distortion itself
    x, y = np.array([0.3, -1.1, 1.5]), np.array([-0.2, 0.9, 1.1])
    _, _, a, b, c, e = ref.distort(x, y, D, True)
    h = 1e-6
    fx = [(q1 - q0) / (2 * h) for q1, q0 in zip(ref.distort(x + h, y, D), ref.distort(x - h, y, D))]
    fy = [(q1 - q0) / (2 * h) for q1, q0 in zip(ref.distort(x, y + h, D), ref.distort(x, y - h, D))]
    assert np.abs(np.array([a - fx[0], b - fy[0], c - fx[1], e - fy[1]])).max() <= 1e-9


def test_distortion_symbols_resolve_with_the_declared_argument_types():
    from gisnav_amd import _lib, build
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = {"gn_set_distortion": [ctypes.c_void_p, _lib.c_f64p, ctypes.c_int],
            "gn_get_distortion": [ctypes.c_void_p, _lib.c_f64p],
            "gn_undistort_points": [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, _lib.c_f64p, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p]}
    lib = _lib.load()
    for name, args in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    # the argument checks that need no context
    assert lib.gn_set_distortion(None, None, 0) < 0 and lib.gn_get_distortion(None, None) < 0


def test_camera_info_defaults_and_the_ros_conversion_copies_d():
    from gisnav_amd import wire
    from gisnav_amd.ros2_node import camera_info_from_ros
    info = wire.CameraInfo(k=K.reshape(9))
    assert info.d is None and info.distortion_model == "" and info.height == 0 and info.width == 0
    assert wire.CameraInfo(K.reshape(9), 480, 640).width == 640                     # positional constructions keep working
    msg = types.SimpleNamespace(k=list(K.reshape(9)), height=480, width=640, d=list(D), distortion_model="plumb_bob")
    got = camera_info_from_ros(msg)
    assert got.d.dtype == np.float64 and np.array_equal(got.d, D) and got.distortion_model == "plumb_bob" and (got.height, got.width) == (480, 640)
    bare = camera_info_from_ros(types.SimpleNamespace(k=list(K.reshape(9)), height=1, width=2))
    assert bare.d is None and bare.distortion_model == ""
    empty = camera_info_from_ros(types.SimpleNamespace(k=list(K.reshape(9)), height=1, width=2, d=[], distortion_model=""))
    assert empty.d.size == 0


def test_an_unsupported_model_raises_only_when_distortion_is_asked_for():
    from gisnav_amd import wire
    from gisnav_amd.pose import compute_pose, distortion_of
    bad = wire.CameraInfo(k=K.reshape(9), d=np.zeros(8), distortion_model="rational_polynomial")
    pts = np.zeros((3, 2), np.float32)                                               # < 4 points: "no pose" before any device work
    with pytest.raises(ValueError, match="rational_polynomial"):
        compute_pose(bad, pts, pts, None, use_distortion=True)
    assert compute_pose(bad, pts, pts, None) is None                                 # the default ignores d, like the reference
    with pytest.raises(ValueError):
        distortion_of(types.SimpleNamespace(k=K.reshape(9), d=[0.1] * 4, distortion_model="equidistant"))
    assert distortion_of(wire.CameraInfo(k=K.reshape(9))).size == 0                  # missing d: off
    assert distortion_of(wire.CameraInfo(k=K.reshape(9), d=np.array([]), distortion_model="plumb_bob")).size == 0
    assert np.array_equal(distortion_of(wire.CameraInfo(k=K.reshape(9), d=D, distortion_model="plumb_bob")), D)

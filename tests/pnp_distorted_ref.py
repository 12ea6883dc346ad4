"""fp64 restatement of cv2.solvePnPRansac WITH distCoeffs (plumb-bob), composed from the project's oracle -- a test helper, not a test.

[EXT] OpenCV 4.x calib3d (solvepnp.cpp, calibration.cpp, undistort.dispatch.cpp), restated; OpenCV itself cannot be run where these tests
run.  `oracle.pnp_ransac` restates the zero-distortion solver; this module replaces only the three places distortion enters:

  * the inputs of the minimal solvers (EPnP, P3P) and of the planar / DLT start: image points undistorted by cv::undistortPoints' fixed-point
    iteration with EXACTLY five steps (TermCriteria(COUNT, 5, 0.01)) -- float32-stored for the minimal solvers, double for the start;
  * the scoring projection of the RANSAC loop: the forward model with distortion, float32, against the raw image points;
  * the Levenberg-Marquardt residual and Jacobian: raw-pixel residuals of the forward model, Jacobian taken through the distortion.

Model (k1, k2, p1, p2, k3); four coefficients mean k3 = 0:
    x = X/Z, y = Y/Z, r2 = x^2 + y^2, c = 1 + k1 r2 + k2 r2^2 + k3 r2^3
    xd = x c + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y c + p1 (r2 + 2 y^2) + 2 p2 x y,  u = fx xd + cx, v = fy yd + cy
With d = 0 every function here returns exactly what its oracle counterpart returns (tests/test_pnp_distortion_host.py).
"""
from __future__ import annotations

import math

import numpy as np

from oracle.pnp_ransac import (CvRNG, DBL_EPSILON, FLT_EPSILON, epnp, find_homography_ls, get_subset, ransac_update_num_iters, rodrigues_mat2vec,
                               rodrigues_vec2mat, solve_p3p)

# the scenes of the distortion tests (fixed by the issue): the bench camera and a mild plumb-bob distortion, monotonic over the frame
K_TEST = np.array([[205.4696, 0.0, 320.0], [0.0, 205.4696, 240.0], [0.0, 0.0, 1.0]])
D_TEST = np.array([-0.05, 0.002, 5e-4, -3e-4, 0.0])


def coeffs5(d) -> np.ndarray:
    d = np.zeros(0) if d is None else np.asarray(d, np.float64).reshape(-1)
    if d.size not in (0, 4, 5):
        raise ValueError("plumb-bob only: 0, 4 or 5 coefficients")
    out = np.zeros(5)
    out[:d.size] = d
    return out


def distort(x, y, d, jac: bool = False):
    """Normalised (x, y) -> distorted normalised (xd, yd) [, a, b, c, e = dxd/dx, dxd/dy, dyd/dx, dyd/dy]."""
    k1, k2, p1, p2, k3 = coeffs5(d)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = 2.0 * x * y
    a2 = r2 + 2.0 * x * x
    a3 = r2 + 2.0 * y * y
    cd = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * cd + p1 * a1 + p2 * a2
    yd = y * cd + p1 * a3 + p2 * a1
    if not jac:
        return xd, yd
    cp = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4
    a = cd + 2.0 * x * x * cp + 2.0 * p1 * y + 6.0 * p2 * x
    b = 2.0 * x * y * cp + 2.0 * p1 * x + 2.0 * p2 * y
    e = cd + 2.0 * y * y * cp + 6.0 * p1 * y + 2.0 * p2 * x
    return xd, yd, a, b, b, e


def undistort(img, A, d, steps: int = 5) -> np.ndarray:
    """cv::undistortPoints without R / P: pixels (n, 2) -> normalised (n, 2) f64 after `steps` fixed-point steps (OpenCV: 5)."""
    k1, k2, p1, p2, k3 = coeffs5(d)
    img = np.asarray(img, np.float64).reshape(-1, 2)
    x0 = (img[:, 0] - A[0, 2]) / A[0, 0]
    y0 = (img[:, 1] - A[1, 2]) / A[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(steps):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return np.column_stack([x, y])


def project_points_dist(obj, rvec, tvec, A, d, jac: bool = False):
    """cvProjectPoints2 with distCoeffs.  obj (n, 3) f64 -> (n, 2) f64 [, d/d(rvec, tvec) (2n, 6)]."""
    t = np.asarray(tvec, np.float64).reshape(3)
    if jac:
        R, dRdr = rodrigues_vec2mat(rvec, True)
    else:
        R = rodrigues_vec2mat(rvec)
    fx, fy, cx, cy = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    X = obj @ R.T + t
    with np.errstate(divide="ignore"):
        z = np.where(X[:, 2] != 0, 1.0 / X[:, 2], 1.0)
    x, y = X[:, 0] * z, X[:, 1] * z
    if not jac:
        xd, yd = distort(x, y, d)
        return np.column_stack([xd * fx + cx, yd * fy + cy])
    xd, yd, a, b, c, e = distort(x, y, d, True)
    proj = np.column_stack([xd * fx + cx, yd * fy + cy])
    n = obj.shape[0]
    J = np.empty((2 * n, 6))
    # d(xd, yd) / d(X, Y, Z) through x = X z, y = Y z
    dudX = np.column_stack([a * z, b * z, -(a * x + b * y) * z])
    dvdX = np.column_stack([c * z, e * z, -(c * x + e * y) * z])
    J[0::2, 3:6] = fx * dudX
    J[1::2, 3:6] = fy * dvdX
    for i in range(3):
        dX = obj @ dRdr[i].reshape(3, 3).T
        J[0::2, i] = fx * np.einsum("nk,nk->n", dudX, dX)
        J[1::2, i] = fy * np.einsum("nk,nk->n", dvdX, dX)
    return proj, J


def _levmarq_pose_dist(obj, img, A, d, r0, t0, max_iter=20, eps=FLT_EPSILON):
    """oracle.pnp_ransac._levmarq_pose with the residual / Jacobian of the distorted forward model (the loop itself is CvLevMarq's, unchanged)."""
    param = np.concatenate([r0, t0]).astype(np.float64)
    prev_param = param.copy()
    lambda_lg10 = -3
    iters = 0
    prev_err_norm = 0.0
    img_flat = img.reshape(-1)

    def residual(p, jac):
        if jac:
            proj, J = project_points_dist(obj, p[:3], p[3:], A, d, True)
            return proj.reshape(-1) - img_flat, J
        return project_points_dist(obj, p[:3], p[3:], A, d).reshape(-1) - img_flat, None

    def step(JtJ, JtErr):
        lam = math.exp(lambda_lg10 * math.log(10.0))
        M = JtJ.copy()
        M[np.diag_indices(6)] *= 1.0 + lam
        return prev_param - np.linalg.lstsq(M, JtErr, rcond=None)[0]

    err, J = residual(param, True)
    while True:
        JtJ, JtErr = J.T @ J, J.T @ err
        prev_param = param.copy()
        param = step(JtJ, JtErr)
        if iters == 0:
            prev_err_norm = float(np.linalg.norm(err))
        while True:
            err, _ = residual(param, False)
            err_norm = float(np.linalg.norm(err))
            if err_norm > prev_err_norm:
                lambda_lg10 += 1
                if lambda_lg10 <= 16:
                    param = step(JtJ, JtErr)
                    continue
            break
        lambda_lg10 = max(lambda_lg10 - 1, -16)
        iters += 1
        denom = float(np.linalg.norm(prev_param))
        rel = float(np.linalg.norm(param - prev_param)) / (denom if denom > 0 else 1.0)
        if iters >= max_iter or rel < eps:
            break
        prev_err_norm = err_norm
        err, J = residual(param, True)
    return param[:3], param[3:]


def solve_pnp_iterative_dist(obj, img, A, d):
    """oracle.pnp_ransac.solve_pnp_iterative with distCoeffs: the planar / DLT start reads the five-step undistorted points (double)."""
    obj = np.asarray(obj, np.float64)
    img = np.asarray(img, np.float64)
    n = len(obj)
    mn = undistort(img, A, d)
    Mc = obj.mean(axis=0)
    MM = (obj - Mc).T @ (obj - Mc)
    _, W, Vt = np.linalg.svd(MM)
    if W[2] / W[1] < 1e-3:
        R_tr = Vt.copy()
        if Vt[0, 2] ** 2 + Vt[1, 2] ** 2 < 1e-10:
            R_tr = np.eye(3)
        if np.linalg.det(R_tr) < 0:
            R_tr = -R_tr
        T_tr = -R_tr @ Mc
        Mxy = (obj @ R_tr.T + T_tr)[:, :2]
        H = find_homography_ls(Mxy, mn)
        if H is not None and np.all(np.isfinite(H)):
            h1n, h2n = np.linalg.norm(H[:, 0]), np.linalg.norm(H[:, 1])
            h1 = H[:, 0] / max(h1n, DBL_EPSILON)
            h2 = H[:, 1] / max(h2n, DBL_EPSILON)
            t = H[:, 2] * (2.0 / max(h1n + h2n, DBL_EPSILON))
            Rh = np.column_stack([h1, h2, np.cross(h1, h2)])
            Rh = rodrigues_vec2mat(rodrigues_mat2vec(Rh))
            t = t + Rh @ T_tr
            R = Rh @ R_tr
        else:
            R, t = np.eye(3), np.zeros(3)
        r = rodrigues_mat2vec(R)
    else:
        if n < 6:
            raise ValueError("DLT algorithm needs at least 6 points")
        L = np.zeros((2 * n, 12))
        x, y = -mn[:, 0], -mn[:, 1]
        L[0::2, 0:3], L[0::2, 3] = obj, 1.0
        L[0::2, 8:11], L[0::2, 11] = x[:, None] * obj, x
        L[1::2, 4:7], L[1::2, 7] = obj, 1.0
        L[1::2, 8:11], L[1::2, 11] = y[:, None] * obj, y
        _, _, LV = np.linalg.svd(L.T @ L)
        RRt = LV[11].reshape(3, 4).copy()
        if np.linalg.det(RRt[:, :3]) < 0:
            RRt = -RRt
        sc = np.linalg.norm(RRt[:, :3])
        U, _, Vt2 = np.linalg.svd(RRt[:, :3])
        R = U @ Vt2
        t = RRt[:, 3] * (np.linalg.norm(R) / sc)
        r = rodrigues_mat2vec(R)
    return _levmarq_pose_dist(obj, img, A, d, r, t)


def solve_pnp_ransac_dist(obj, img, A, d, iterations_count: int = 10, reproj_error: float = 8.0, confidence: float = 0.99):
    """cv2.solvePnPRansac(obj f32 (K,3), img f32 (K,2), A f64, d, False, iterations_count) -> (ok, rvec (3,1), tvec (3,1), inliers or None):
    oracle.pnp_ransac.solve_pnp_ransac, line for line, with the three replacements named in the module docstring."""
    obj = np.asarray(obj, np.float32)
    img = np.asarray(img, np.float32)
    count = len(obj)
    model_points = 5
    A = np.asarray(A, np.float64).reshape(3, 3)
    obj64, img64 = obj.astype(np.float64), img.astype(np.float64)
    # cv::undistortPoints' output takes the input's depth: computed in double, stored as float32
    und = undistort(img64, A, d).astype(np.float32).astype(np.float64)
    if count == 4:
        sol = solve_p3p(obj64, und)
        if sol is None:
            return False, None, None, None
        r = rodrigues_mat2vec(sol[0])
        return True, r.reshape(3, 1), np.asarray(sol[1]).reshape(3, 1), np.arange(4)
    if count < model_points:
        return False, None, None, None
    fu, fv, uc, vc = float(A[0, 0]), float(A[1, 1]), float(A[0, 2]), float(A[1, 2])
    us_px = np.column_stack([und[:, 0] * fu + uc, und[:, 1] * fv + vc])      # epnp::init_points
    if count == model_points:
        try:
            R, t = epnp(obj64, us_px, fu, fv, uc, vc)
            rvec = rodrigues_mat2vec(R)
            ok = bool(np.all(np.isfinite(rvec)) and np.all(np.isfinite(t)))
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            ok = False
        if not ok:
            return False, None, None, None
        return True, rvec.reshape(3, 1), np.asarray(t).reshape(3, 1), np.arange(count)
    rng = CvRNG(0xFFFFFFFFFFFFFFFF)
    niters = iterations_count
    max_good = 0
    best_mask, best_model = None, None
    thr = np.float32(reproj_error * reproj_error)
    it = 0
    while it < niters:
        idx = get_subset(rng, count, model_points)
        try:
            R, t = epnp(obj64[idx], us_px[idx], fu, fv, uc, vc)
            rvec = rodrigues_mat2vec(R)
            ok = bool(np.all(np.isfinite(rvec)) and np.all(np.isfinite(t)))
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            ok = False
        if ok:
            proj = project_points_dist(obj64, rvec, t, A, d).astype(np.float32)
            diff = img - proj
            err = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]).astype(np.float32)
            mask = err <= thr
            good = int(mask.sum())
            if good > max(max_good, model_points - 1):
                best_mask, best_model, max_good = mask, (rvec, t), good
                niters = ransac_update_num_iters(confidence, (count - good) / count, model_points, niters)
        it += 1
    if best_mask is None:
        return False, None, None, None
    inl = np.nonzero(best_mask)[0]
    try:
        r, t = solve_pnp_iterative_dist(obj64[inl], img64[inl], A, d)
    except ValueError:
        r, t = best_model
    return True, r.reshape(3, 1), np.asarray(t).reshape(3, 1), inl


def make_scene(n: int, seed: int, planar: bool, A=K_TEST, d=D_TEST):
    """One scene of the issue: (obj (n,3) f32, img (n,2) f32 with a quarter of the points displaced by 40-120 px, rvec, tvec, inlier mask).
    The outliers are every fourth point: cv::RNG's ten 5-subsets depend on n alone, and with these indices each n used here has several
    subsets free of outliers (a random choice leaves some scenes without one, where solvePnPRansac rightly finds no model)."""
    rng = np.random.default_rng(seed)
    obj = np.column_stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n),
                           np.zeros(n) if planar else rng.integers(0, 41, n).astype(np.float64)]).astype(np.float32)
    rvec = np.array([0.03, -0.02, 0.1])
    centre = np.array([320 + rng.uniform(-30, 30), 240 + rng.uniform(-30, 30), -rng.uniform(330, 420)])
    R = rodrigues_vec2mat(rvec)
    tvec = -R @ centre
    img = project_points_dist(obj.astype(np.float64), rvec, tvec, A, d)
    out = np.arange(3, n, 4)                    # every fourth point (the positions are random already)
    n_out = len(out)
    ang, mag = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(40, 120, n_out)
    img[out] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
    inl = np.ones(n, bool)
    inl[out] = False
    return obj, img.astype(np.float32), rvec, tvec, inl

"""Pose covariance from the PnP inliers (gn_pnp_ransac_cov / gn_estimate_cov / gn_vo_estimate_cov; DESIGN.md "Pose covariance").

  1. against fp64: cov_rt and sigma_hat of one 8-pair call (flat / smooth DEM, gross outliers, 12 / 7 / 1024 / 5 / 4 points, one pair below min_pts) and
     of a call with fx != fy equal numpy's s^2 (J^T J)^-1 from oracle.pnp_ransac.project_points at the GPU's own pose over the oracle's inlier set;
  2. nothing else moves: R, t, n_inliers, ok are bit for bit gn_pnp_ransac's, and a stated sigma_px only rescales the covariance;
  3. through every call path of gn_estimate_cov (plain, overlap, sub-streams, deferred join, certificate re-run, deferred certificate) and
     gn_vo_estimate_cov: bitwise the staged match -> gather_points -> pnp_ransac(covariance=True);
  4. it means what it says: over 512 noise realisations the sample variance of (rvec, tvec) matches the predicted one and the mean NEES is 6;
  5. end to end: compute_pose(return_covariance=True) -> pose_to_earth(cov_rt=...).

k_pnp_cov has no capacity threshold of its own (no LDS staging: it strides the pair's points with the mask test), so there is no case on either
side of one; the 1024-point pair covers many trips per lane, the 4- and 5-point pairs the branches without a mask.
"""
import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu


def _scene(idx, n, flat=False, K=K_MATRIX):
    """make_pair(idx, n_q=n, n_r=n, match_fraction=1.0): object points = kp_r + the DEM height of the matched rows (f32), image points = their
    exact projection (f64, noise added by the caller)."""
    p = make_pair(idx, n_q=n, n_r=n, flat_dem=flat, match_fraction=1.0)
    r = p.gt_q2r[p.gt_q2r >= 0]
    h, w = p.dem.shape
    z = p.dem[np.minimum(np.floor(p.kp_r[r, 1]).astype(int), h - 1), np.minimum(np.floor(p.kp_r[r, 0]).astype(int), w - 1)].astype(np.float64)
    obj = np.column_stack([p.kp_r[r].astype(np.float64), z])
    cam = obj @ p.R_gt.T + p.t_gt.T
    uv = cam[:, :2] / cam[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    return obj.astype(np.float32), uv, p


def _noisy(uv, rng, sigma=0.5):
    return (uv + rng.normal(0, sigma, uv.shape)).astype(np.float32)


def _stage(eng, scenes):
    """[(obj (n,3) f32, img (n,2) f32)] -> device obj [B,S,3], img [B,S,2], n_pts [B]."""
    B, S = len(scenes), max(len(o) for o, _ in scenes)
    obj, img, n = np.zeros((B, S, 3), np.float32), np.zeros((B, S, 2), np.float32), np.zeros(B, np.int32)
    for b, (o, u) in enumerate(scenes):
        obj[b, :len(o)], img[b, :len(o)], n[b] = o, u, len(o)
    d = eng.device
    return torch.from_numpy(obj).to(d), torch.from_numpy(img).to(d), torch.from_numpy(n).to(d)


def _reference(obj, img, K, R, t, sigma_px=0.0):
    """fp64 covariance at the pose (R, t) over the oracle's inlier set: (cov, sigma_hat, number of inliers)."""
    ok, _, _, inl = pr.solve_pnp_ransac(obj, img, K)
    assert ok
    inl = np.asarray(inl).reshape(-1)
    rvec = pr.rodrigues_mat2vec(R)
    proj, J = pr.project_points(obj[inl].astype(np.float64), rvec, np.asarray(t).reshape(3), K, jac=True)
    e = (proj - img[inl].astype(np.float64)).reshape(-1)
    dof = 2 * len(inl) - 6
    s2 = float(e @ e) / dof
    return (sigma_px ** 2 if sigma_px > 0 else s2) * np.linalg.inv(J.T @ J), np.sqrt(s2), len(inl)


def _scaled_diff(got, want):
    d = np.sqrt(np.diag(want))
    return float((np.abs(got - want) / np.outer(d, d)).max())


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=8, max_kpts=1024)
    yield e
    del e


@pytest.fixture(scope="module")
def eight(eng):
    """The 8-pair call of tests 1 and 2: scenes, the covariance call's outputs (host), computed once."""
    rng = np.random.default_rng(7)
    scenes = []
    o, uv, _ = _scene(1, 64, flat=True); scenes.append((o, _noisy(uv, rng)))                      # 64 points, flat DEM
    o, uv, _ = _scene(0, 64); u = _noisy(uv, rng)                                                 # 64 points, smooth DEM, 20 % gross outliers
    bad = rng.permutation(len(o))[: len(o) // 5]
    u[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))]).astype(np.float32)
    scenes.append((o, u))
    o, uv, _ = _scene(2, 12); scenes.append((o, _noisy(uv, rng)))                                 # 12 points
    o, uv, _ = _scene(5, 12); scenes.append((o[:7], _noisy(uv[:7], rng)))                         # 7 points
    o, uv, _ = _scene(3, 1024); scenes.append((o, _noisy(uv, rng)))                               # 1024 points
    o, uv, _ = _scene(6, 12); scenes.append((o[:5], _noisy(uv[:5], rng)))                         # 5 points: the model_points == npoints branch
    o, uv, _ = _scene(8, 12); scenes.append((o[:4], _noisy(uv[:4], rng)))                         # 4 points: the P3P branch
    o, uv, _ = _scene(9, 12); scenes.append((o[:3], _noisy(uv[:3], rng)))                         # below min_pts
    assert [len(o) for o, _ in scenes][2:] == [12, 7, 1024, 5, 4, 3] and all(len(o) > 48 for o, _ in scenes[:2])
    obj, img, n = _stage(eng, scenes)
    res = eng.pnp_ransac(obj, img, n, K_MATRIX, min_pts=4, covariance=True)
    torch.cuda.synchronize()
    return scenes, (obj, img, n), [x.cpu().numpy() for x in res]


def _check_against_fp64(scenes, res, K, label):
    R, t, n_inl, ok, cov, sigma, cov_ok = res
    worst_c, worst_s = 0.0, 0.0
    for b, (o, u) in enumerate(scenes):
        if len(o) < 4:
            continue
        assert ok[b] == 1 and cov_ok[b] == 1, (label, b)
        want, s_hat, k = _reference(o, u, K, R[b], t[b])
        assert k == n_inl[b], (label, b, k, n_inl[b])                 # the same inlier set, by size
        assert np.array_equal(cov[b], cov[b].T)
        dc, ds = _scaled_diff(cov[b], want), abs(sigma[b] - s_hat) / s_hat
        print(f"{label} pair {b}: n = {len(o)}, inliers {k}, sigma_hat {sigma[b]:.4f} px, scaled cov difference {dc:.2e}, sigma relative {ds:.2e}")
        worst_c, worst_s = max(worst_c, dc), max(worst_s, ds)
    print(f"{label}: worst scaled covariance difference {worst_c:.3e}, worst relative sigma_hat difference {worst_s:.3e}")
    assert worst_c <= 1e-9, worst_c
    assert worst_s <= 1e-10, worst_s


def test_covariance_matches_fp64_numpy_at_the_returned_pose(eng, eight):
    """max |dS_ij| / sqrt(S_ii S_jj) <= 1e-9 (scaled condition number of N 45-142 on these scenes, the fp64 reference differs from itself under a
    permuted summation by 1.7e-14: about 1.5e2 x 1024 x 2.2e-16 = 3e-11 expected), sigma_hat to 1e-10 relative.  Every figure is printed before
    it is asserted; DESIGN.md section 13 is where the measured value is recorded."""
    scenes, _, res = eight
    _check_against_fp64(scenes, res, K_MATRIX, "fx == fy")
    R, t, n_inl, ok, cov, sigma, cov_ok = res
    assert n_inl[1] < len(scenes[1][0]) - 5                           # the outliers were rejected: the mask path saw zeros
    # the pair below min_pts: no pose, no covariance
    assert ok[7] == 0 and cov_ok[7] == 0 and sigma[7] == 0.0 and not cov[7].any()
    # fx != fy once
    K2 = K_MATRIX.copy(); K2[1, 1] = 231.5
    rng = np.random.default_rng(17)
    scenes2 = []
    for idx, n, flat in [(0, 64, False), (1, 64, True)]:
        o, uv, _ = _scene(idx, n, flat, K=K2)
        scenes2.append((o, _noisy(uv, rng)))
    obj, img, n = _stage(eng, scenes2)
    res2 = [x.cpu().numpy() for x in eng.pnp_ransac(obj, img, n, K2, covariance=True)]
    _check_against_fp64(scenes2, res2, K2, "fx != fy")


def test_nothing_else_moves_and_a_stated_sigma_only_rescales(eng, eight):
    scenes, (obj, img, n), res = eight
    plain = [x.cpu().numpy() for x in eng.pnp_ransac(obj, img, n, K_MATRIX, min_pts=4)]
    assert len(plain) == 4
    for name, a, b in zip(("R", "t", "n_inliers", "ok"), plain, res):
        assert np.array_equal(a, b), name
    stated = [x.cpu().numpy() for x in eng.pnp_ransac(obj, img, n, K_MATRIX, min_pts=4, covariance=True, sigma_px=0.5)]
    for name, a, b in zip(("R", "t", "n_inliers", "ok"), plain, stated):
        assert np.array_equal(a, b), name
    cov, sigma, cov_ok = res[4:]
    assert np.array_equal(stated[6], cov_ok) and np.array_equal(stated[5], sigma)        # sigma_hat is reported either way
    assert cov_ok[:7].all()
    for b in range(7):
        assert _scaled_diff(stated[4][b], 0.25 / sigma[b] ** 2 * cov[b]) <= 1e-12, b
    assert not stated[4][7].any()


# ------------------------------------------------------------------------------------------------------------------ call paths
COV_KEYS = ("cov", "sigma", "cov_ok")
ALL_KEYS = ("R", "t", "n_match", "n_inliers", "ok") + COV_KEYS


@pytest.fixture(scope="module")
def call_paths():
    """B = 4 pairs of 256 keypoints; the staged path match -> gather_points -> pnp_ransac(covariance=True) on an f32 context is the reference of
    every estimate(covariance=True) variant."""
    from gisnav_amd.engine import MIN_MATCHES, PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(0)
    pairs = [make_pair(7300 + i, n_q=256 - 9 * i, n_r=256 - 5 * i) for i in range(4)]
    f32 = PoseEngine(0, max_batch=4, max_kpts=256, precision="f32", state_dict=sd)
    inp = f32.stage_inputs(pairs)
    idx, _, n_match = f32.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = f32.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
    R, t, n_inl, ok, cov, sigma, cov_ok = f32.pnp_ransac(obj, mkp, n_match, K_MATRIX, min_pts=MIN_MATCHES, covariance=True)
    torch.cuda.synchronize()
    want = dict(R=R, t=t, n_match=n_match, n_inliers=n_inl, ok=ok, cov=cov, sigma=sigma, cov_ok=cov_ok)
    want = {k: v.clone() for k, v in want.items()}
    assert int(want["cov_ok"].sum()) == 4 and bool((want["sigma"] > 0).all())
    yield sd, pairs, f32, inp, want
    del f32


def _equal(got, want, keys=ALL_KEYS):
    return [k for k in keys if not torch.equal(got[k].reshape(want[k].shape), want[k])]


def _poison(out):
    for k in COV_KEYS:
        out[k].fill_(7)
    return out


@pytest.mark.parametrize("mode", ["plain", "overlap", "substreams", "deferred_join"])
def test_estimate_cov_on_an_f32_context_equals_the_staged_path_bitwise(call_paths, mode):
    sd, pairs, f32, inp, want = call_paths
    out = _poison(f32.alloc_outputs(4, covariance=True))
    try:
        if mode == "overlap":
            f32.set_overlap(True)
        elif mode == "substreams":
            f32.set_substreams(2)
        elif mode == "deferred_join":
            f32.set_substreams(2, deferred_join=True)
        f32.estimate(inp, K_MATRIX, out=out, covariance=True)
        if mode in ("overlap", "deferred_join"):
            f32.flush()
        torch.cuda.synchronize()
    finally:
        f32.flush()
        f32.set_overlap(False)
        f32.set_substreams(1)
    assert not _equal(out, want), (mode, _equal(out, want))


@pytest.mark.parametrize("mode", ["rerun", "substreams_deferred_certificate"])
def test_estimate_cov_through_the_certificate_rerun_equals_the_f32_context_bitwise(call_paths, mode):
    """eps = inf flags every pair: all four go through the gathered exact-f32 re-run and its scatter, which must carry the three covariance arrays."""
    from gisnav_amd.engine import PoseEngine
    sd, pairs, f32, _, want = call_paths
    fast = PoseEngine(0, max_batch=4, max_kpts=256, precision="f16x2_f16_attn", state_dict=sd)
    inp = fast.stage_inputs(pairs)
    out = _poison(fast.alloc_outputs(4, covariance=True))
    fast.certify_stats(reset=True)
    if mode == "rerun":
        fast.set_certify("rerun", eps=float("inf"))
        fast.estimate(inp, K_MATRIX, out=out, covariance=True)
    else:
        fast.set_substreams(2)
        fast.set_certify("deferred", eps=float("inf"))
        fast.estimate(inp, K_MATRIX, out=out, covariance=True)
        fast.flush()
    torch.cuda.synchronize()
    st = fast.certify_stats()
    fast.set_certify("off")
    fast.set_substreams(1)
    del fast
    assert st["rerun_pairs"] == 4, st
    assert not _equal(out, want), (mode, _equal(out, want))


def test_vo_estimate_cov_equals_its_staged_path_bitwise(call_paths):
    sd, pairs, f32, inp, _ = call_paths
    out = _poison(f32.alloc_outputs(4, covariance=True))
    f32.vo_estimate(inp, K_MATRIX, ratio=0.9, min_matches=15, out=out, covariance=True)
    idx, _, n_good = f32.vo_match(inp["desc_q"], inp["n_q"], inp["desc_r"], inp["n_r"], ratio=0.9)
    mkp, obj = f32.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_good, None)
    R, t, n_inl, ok, cov, sigma, cov_ok = f32.pnp_ransac(obj, mkp, n_good, K_MATRIX, min_pts=15, covariance=True)
    plain = f32.vo_estimate(inp, K_MATRIX, ratio=0.9, min_matches=15)
    torch.cuda.synchronize()
    want = dict(R=R, t=t, n_match=n_good, n_inliers=n_inl, ok=ok, cov=cov, sigma=sigma, cov_ok=cov_ok)
    assert not _equal(out, want), _equal(out, want)
    assert not _equal(plain, want, ALL_KEYS[:5]) and sorted(plain) == sorted(ALL_KEYS[:5])
    assert int(out["ok"].sum()) > 0 and torch.equal(out["ok"], out["cov_ok"])


def test_pose_node_keeps_returning_r_t_and_stores_the_covariance(state_dict_np):
    from gisnav_amd import wire
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.pose_node import PoseNode
    p = make_pair(86, n_q=300, n_r=280)
    extractor = lambda ref: (p.kp_r, p.desc_r, p.size_r, p.angle_r)  # noqa: E731
    cam = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    msg = wire.OrthoStereoImage(query_sift=wire.pack_keypoints(p.kp_q, p.size_q, p.angle_q, p.desc_q), reference=wire.ImageMsg(p.ref, wire.Stamp(7, 0)),
                                dem=wire.ImageMsg(p.dem, wire.Stamp(7, 0)))
    node = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32", covariance=True)
    plain_node = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32")
    assert node.last_covariance is None
    r = node.estimate(cam, msg)
    r0 = plain_node.estimate(cam, msg)
    eng = PoseEngine(0, max_batch=1, max_kpts=512, precision="f32", state_dict=state_dict_np)
    want = eng.estimate(eng.stage_inputs([p]), K_MATRIX, covariance=True)
    torch.cuda.synchronize()
    assert r is not None and len(r) == 2 and np.array_equal(r[0], r0[0]) and np.array_equal(r[1], r0[1])
    assert np.array_equal(r[0], want["R"][0].cpu().numpy()) and int(want["cov_ok"][0]) == 1
    assert plain_node.last_covariance is None
    assert node.last_covariance is not None and np.array_equal(node.last_covariance, want["cov"][0].cpu().numpy())
    assert node.last_sigma_px == float(want["sigma"][0])
    empty = wire.OrthoStereoImage(query_sift=b"", reference=msg.reference, dem=msg.dem)
    assert node.estimate(cam, empty) is None and node.last_covariance is None         # no pose: no stale covariance


# ------------------------------------------------------------------------------------------------------------------ statistics
def test_predicted_covariance_matches_the_scatter_of_512_noise_realisations():
    """Scene make_pair(10, 48, 48), 512 realisations of N(0, 0.5 px) from default_rng(99), two calls of B = 256.  The per-component ratio of the
    sample variance of (rvec, tvec) to the mean predicted variance lies in [0.75, 1.33] (a variance ratio over 512 samples has sigma = 6.3 %:
    +- 4 sigma), and the mean NEES d^T cov^-1 d (d = estimate - sample mean) in 6 +- 0.62 = 4 sqrt(12 / 512).  The oracle alone gives ratios
    0.957-1.065 and NEES 6.15 on these inputs."""
    from gisnav_amd.engine import PoseEngine
    obj, uv, _ = _scene(10, 48)
    rng = np.random.default_rng(99)
    imgs = [_noisy(uv, rng) for _ in range(512)]
    e = PoseEngine(0, max_batch=256, max_kpts=128)
    est, pred, n_inl = [], [], []
    for c in range(2):
        o, u, n = _stage(e, [(obj, im) for im in imgs[256 * c: 256 * (c + 1)]])
        R, t, ni, ok, cov, sigma, cov_ok = [x.cpu().numpy() for x in e.pnp_ransac(o, u, n, K_MATRIX, covariance=True)]
        assert ok.all() and cov_ok.all()
        est += [np.concatenate([pr.rodrigues_mat2vec(R[b]), t[b].reshape(3)]) for b in range(256)]
        pred += list(cov)
        n_inl += list(ni)
    del e
    est, pred = np.array(est), np.array(pred)
    assert min(n_inl) >= len(obj) - 1, min(n_inl)
    ratio = np.diag(np.cov(est.T)) / np.diag(pred.mean(0))
    d = est - est.mean(0)
    nees = float(np.mean([d[i] @ np.linalg.solve(pred[i], d[i]) for i in range(512)]))
    print("variance ratio sample / predicted:", np.round(ratio, 3), "| mean NEES", round(nees, 3), "| inliers", min(n_inl), "-", max(n_inl))
    assert ratio.min() >= 0.75 and ratio.max() <= 1.33, ratio
    assert abs(nees - 6.0) <= 0.62, nees


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_compute_pose_covariance_reaches_the_earth_frame():
    import types
    from gisnav_amd import georef as gg
    from gisnav_amd.pose import compute_pose
    from oracle import georef as og
    mpp, rot = 0.8, np.radians(30.0)
    dlat = mpp / 111_320.0; dlon = dlat / np.cos(np.radians(60.17))
    M = np.array([[np.cos(rot) * dlon, np.sin(rot) * dlon, 0.0, 24.94], [np.sin(rot) * dlat, -np.cos(rot) * dlat, 0.0, 60.17], [0.0, 0.0, -mpp, 12.5]])
    crs = og.affine_to_proj(M)
    obj, uv, p = _scene(0, 64)
    img = _noisy(uv, np.random.default_rng(3))
    info = types.SimpleNamespace(k=K_MATRIX.reshape(9))
    R, t, cov_rt = compute_pose(info, img, obj[:, :2], p.dem, return_covariance=True)
    plain = compute_pose(info, img, obj[:, :2], p.dem)
    assert len(plain) == 2 and np.array_equal(plain[0], R) and np.array_equal(plain[1], t)
    assert cov_rt is not None and cov_rt.shape == (6, 6) and np.array_equal(cov_rt, cov_rt.T)
    earth = gg.pose_to_earth(R, t, crs, p.dem.shape, cov_rt=cov_rt)
    assert earth is not None
    C = earth["covariance"]
    assert np.array_equal(C, C.T)
    w = np.linalg.eigvalsh(C)
    assert w.min() >= -1e-12 * w.max() and w.max() > 0
    # Position: the map from the camera centre (raster px) to ECEF is linear at this scale, G = d ecef / d c, taken here by central differences of
    # the oracle's own affine -> WGS 84 -> ECEF chain.  Its columns are mpp long (to the difference between 111 320 m and the ellipsoid's metres
    # per degree at this latitude), and pulled back along the raster's axes the position block is cov_cam's: each standard deviation to 1e-3.
    cam = gg.pose_cov_to_camera(R, t, cov_rt)
    c = -(R.T @ t).reshape(3)
    ecef = lambda x: np.asarray(og.wgs84_to_ecef(*(M @ np.append(x, 1))))  # noqa: E731
    G = np.column_stack([(ecef(c + e) - ecef(c - e)) / 2.0 for e in np.eye(3)])
    assert np.allclose(np.linalg.norm(G, axis=0), mpp, rtol=5e-3)
    Gi = np.linalg.inv(G)
    got, want = np.sqrt(np.diag(Gi @ C[:3, :3] @ Gi.T)), np.sqrt(np.diag(cam)[:3])
    print("position sigma [m] along ECEF x, y, z:", np.sqrt(np.diag(C)[:3]), "| along the raster axes [px]:", got, "| camera-centre sigma [px]:", want)
    assert np.abs(got / want - 1).max() <= 1e-3, (got, want)
    # Orientation: psi = Q phi with Q the rotation the map applies, orthogonal up to the shear of the normalised affine columns (the x and y
    # scales of the lon / lat grid differ by < 3e-3 here): the total rotational variance is kept to 1e-2.
    assert abs(np.trace(C[3:, 3:]) / np.trace(cam[3:, 3:]) - 1) <= 1e-2

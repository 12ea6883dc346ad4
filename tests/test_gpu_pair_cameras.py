"""Per-pair cameras on the GPU: gn_set_pair_cameras from the PnP kernels up to the Python entry points (DESIGN.md "Per-pair cameras").

Scenes and cameras: tests/pair_cameras_common.py (a scene solved with its neighbour's camera misses by far: tests/test_pair_cameras_host.py).

   1. a uniform table is the by-value call, bitwise (PnP with covariance and report, gn_undistort_points; model 0 and 1);
   2. five cameras in one call: against the fp64 restatement, against B = 1 by-value calls (bitwise), reversed order;
   3. gn_undistort_points with a table, three cameras, counts 63 / 65 / 1;
   4. more than 16 iterations: counts and inlier sets of the by-value calls;
   5. the whole path with sub-batch groups and overlap, and two pipelined calls with two tables under deferred join;
   6. certificate re-runs keep their camera: re-run in place from a later pair, and gathered from scattered pairs; synchronous and deferred;
   7. estimate_bucketed carries the rows with the pairs it reorders;
   8. vo_estimate; 9. loftr_pose_batch; 10. compute_pose_batch;
  11. off is off, the refusals, and the stored gn_set_distortion state coming back.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import pair_cameras_common as pc
import pnp_distorted_ref as ref
from gisnav_amd import _lib
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu

PNP_KEYS = ("R", "t", "n_inliers", "ok", "cov", "sigma", "cov_ok", "inlier_mask", "inlier_idx", "reproj_err")


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=16, max_kpts=128)
    yield e
    del e


def _stage(e, scenes, stride):
    B = len(scenes)
    obj, img, n = np.zeros((B, stride, 3), np.float32), np.zeros((B, stride, 2), np.float32), np.zeros(B, np.int32)
    for b, (o, u) in enumerate(scenes):
        obj[b, :len(o)], img[b, :len(o)], n[b] = o, u, len(o)
    d = e.device
    return torch.from_numpy(obj).to(d), torch.from_numpy(img).to(d), torch.from_numpy(n).to(d)


def _table(e, rows):
    return torch.from_numpy(np.ascontiguousarray(rows, np.float64)).to(e.device)


def _pnp(e, obj, img, n, K=None, d=None, cameras=None, model=0, iterations=10, sigma_px=0.5):
    """gn_pnp_ransac_report with covariance: by value (K, d through gn_set_distortion) or with a table; {key: numpy}"""
    if cameras is None:
        e.set_distortion(d)
    try:
        res = e.pnp_ransac(obj, img, n, K, iterations=iterations, min_pts=4, covariance=True, sigma_px=sigma_px, report=True,
                           cameras=cameras, camera_model=model)
        torch.cuda.synchronize()
    finally:
        e.set_distortion(None)
    return {k: v.cpu().numpy() for k, v in zip(PNP_KEYS, res)}


def _differs(got, want, b_got=None, b_want=None, keys=PNP_KEYS):
    """the keys whose bytes differ (between row b_got of `got` and row b_want of `want` when given)"""
    g = (lambda k: got[k]) if b_got is None else (lambda k: got[k][b_got])
    w = (lambda k: want[k]) if b_want is None else (lambda k: want[k][b_want])
    return [k for k in keys if np.ascontiguousarray(g(k)).tobytes() != np.ascontiguousarray(w(k)).tobytes()]


def _points():
    return [(o, u) for o, u, *_ in pc.scenes()]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("model", [0, 1])
def test_uniform_table_is_the_by_value_call_bitwise(eng, model):
    obj, img, n = _stage(eng, _points(), 64)                              # all five scenes under camera 0
    rows = np.repeat(pc.table_rows()[:1], 5, axis=0)
    want = _pnp(eng, obj, img, n, pc.KS[0], pc.DS[0] if model else None)
    got = _pnp(eng, obj, img, n, cameras=_table(eng, rows), model=model)
    assert not _differs(got, want), _differs(got, want)
    assert want["ok"][0] == 1 and want["cov_ok"][0] == 1                  # (scene 0 is camera 0's: something was solved)
    other = _pnp(eng, obj, img, n, pc.KS[0], None if model else pc.DS[0])
    assert _differs(other, want)                                          # and the two models are told apart by their bits


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("to_pixels", [False, True])
def test_uniform_table_undistort_is_the_by_value_call_bitwise(eng, model, to_pixels):
    dev = eng.device
    rng = np.random.default_rng(3)
    img = torch.from_numpy(rng.uniform(0, 640, (3, 128, 2)).astype(np.float32)).to(dev)
    n = torch.tensor([63, 128, 1], dtype=torch.int32, device=dev)
    fill = lambda: torch.full((3, 128, 2), 7.0, dtype=torch.float32, device=dev)  # noqa: E731
    eng.set_distortion(pc.DS[0] if model else None)
    try:
        want = eng.undistort_points(img, n, pc.KS[0], to_pixels, out=fill()).cpu().numpy()
    finally:
        eng.set_distortion(None)
    rows = np.repeat(pc.table_rows()[:1], 3, axis=0)
    got = eng.undistort_points(img, n, None, to_pixels, out=fill(), cameras=_table(eng, rows), camera_model=model).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert (got[0, 63:] == 7.0).all() and (got[2, 1:] == 7.0).all() and (got[1] != 7.0).any()


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def five(eng):
    """B = 5, kstride 64, model 1, sigma_px 0.5: every scene with its own camera, one call"""
    obj, img, n = _stage(eng, _points(), 64)
    return _pnp(eng, obj, img, n, cameras=_table(eng, pc.table_rows()), model=1)


def test_five_cameras_against_the_restatement(five):
    lines = []
    for b in range(pc.NB):
        w_ok, w_r, w_t, w_inl = pc.restated(b, b)
        assert w_ok and five["ok"][b] == 1, b
        k = int(five["n_inliers"][b])
        assert k == len(w_inl) == pc.TRUE_INLIERS[b], (b, k)
        assert np.array_equal(five["inlier_idx"][b, :k], w_inl) and (five["inlier_idx"][b, k:] == -1).all(), b
        dR, dt = pc.pose_error(five["R"][b], five["t"][b], w_r, w_t)
        lines.append((b, dR, dt))
        print(f"pair {b}: dR {dR:.2e} dt {dt:.2e}")
    for b, dR, dt in lines:
        assert dR < 1e-8 and dt < 1e-8, (b, dR, dt)


@pytest.mark.parametrize("b", [1, 4])
def test_five_cameras_covariance_uses_the_pairs_own_camera(five, b):
    o, u, *_ = pc.scenes()[b]
    inl = np.asarray(pc.restated(b, b)[3]).reshape(-1)
    assert five["cov_ok"][b] == 1
    rv, tv = pr.rodrigues_mat2vec(five["R"][b]), five["t"][b].reshape(3)
    proj, J = ref.project_points_dist(o[inl].astype(np.float64), rv, tv, pc.KS[b], pc.DS[b], True)
    w = 0.25 * np.linalg.inv(J.T @ J)
    d = np.sqrt(np.diag(w))
    diff = float((np.abs(five["cov"][b] - w) / np.outer(d, d)).max())
    e = (proj - u[inl].astype(np.float64)).reshape(-1)
    s_hat = np.sqrt(float(e @ e) / (2 * len(inl) - 6))
    print(f"pair {b}: scaled covariance difference {diff:.3e}, sigma_hat {five['sigma'][b]:.3e} (fp64 {s_hat:.3e})")
    assert diff <= 1e-9
    assert abs(five["sigma"][b] - s_hat) <= 1e-10 * s_hat + 1e-14
    # the neighbour's camera at the same pose gives a different matrix: the check discriminates
    c = (b + 1) % pc.NB
    _, Jc = ref.project_points_dist(o[inl].astype(np.float64), rv, tv, pc.KS[c], pc.DS[c], True)
    assert float((np.abs(0.25 * np.linalg.inv(Jc.T @ Jc) - w) / np.outer(d, d)).max()) > 1e-4


def test_five_cameras_equal_lone_by_value_calls(eng, five):
    for b in range(pc.NB):
        obj, img, n = _stage(eng, _points()[b:b + 1], 64)
        if b != 2:      # same instantiation (plumb-bob), same bits
            lone = _pnp(eng, obj, img, n, pc.KS[b], pc.DS[b])
            assert not _differs(five, lone, b, 0), (b, _differs(five, lone, b, 0))
        else:           # zero coefficients through the plumb-bob instantiation against the pinhole instantiation: rounding only
            assert not pc.DS[2].any()
            lone = _pnp(eng, obj, img, n, pc.KS[2], None)
            assert not _differs(five, lone, 2, 0, ("n_inliers", "ok", "cov_ok", "inlier_mask", "inlier_idx"))
            dR = float(np.linalg.norm(five["R"][2] - lone["R"][0]))
            dt = float(np.linalg.norm(five["t"][2] - lone["t"][0]) / np.linalg.norm(lone["t"][0]))
            print(f"pair 2 through the plumb-bob instantiation against the pinhole one: dR {dR:.2e} dt {dt:.2e}")
            assert dR < 1e-8 and dt < 1e-8


def test_reversed_scenes_with_a_reversed_table_give_the_reversed_outputs(eng, five):
    obj, img, n = _stage(eng, _points()[::-1], 64)
    rev = _pnp(eng, obj, img, n, cameras=_table(eng, pc.table_rows()[::-1]), model=1)
    for b in range(pc.NB):
        assert not _differs(rev, five, pc.NB - 1 - b, b), (b, _differs(rev, five, pc.NB - 1 - b, b))


# ------------------------------------------------------------------------------------------------------------------ 3
def _grid(nx, ny, w, h):
    u, v = np.meshgrid(np.linspace(0, w, nx), np.linspace(0, h, ny))
    return np.column_stack([u.reshape(-1), v.reshape(-1)]).astype(np.float32)


def test_undistort_points_with_a_table(eng):
    cams = [0, 1, 4]
    pts = [_grid(9, 7, 640, 480), _grid(13, 5, 640, 480), _grid(1, 1, 1280, 720)]      # each over its camera's frame, corners included
    assert [len(p) for p in pts] == [63, 65, 1]
    img = np.random.default_rng(0).uniform(0, 640, (3, 128, 2)).astype(np.float32)      # live-looking values past n_pts
    for b, p in enumerate(pts):
        img[b, :len(p)] = p
    dev = eng.device
    out = torch.full((3, 128, 2), 7.0, dtype=torch.float32, device=dev)
    got = eng.undistort_points(torch.from_numpy(img).to(dev), torch.tensor([63, 65, 1], dtype=torch.int32, device=dev), None, False, out=out,
                               cameras=_table(eng, pc.table_rows()[cams]), camera_model=1).cpu().numpy()
    worst = []
    for b, (c, p) in enumerate(zip(cams, pts)):
        n = len(p)
        assert np.all(got[b, n:] == 7.0), b                                             # slots past n_pts untouched
        want = ref.undistort(p, pc.KS[c], pc.DS[c]).astype(np.float32)
        ulps = np.abs(got[b, :n].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst.append(float(ulps.max()))
        print(f"pair {b} (camera {c}): largest distance from the f32-rounded restatement {ulps.max():.2f} ulp")
        # and the neighbour's camera is far away: the row reached the right pair
        wrong = ref.undistort(p, pc.KS[cams[(b + 1) % 3]], pc.DS[cams[(b + 1) % 3]])
        assert np.abs(got[b, :n] - wrong).max() > 1e-2, b
    assert max(worst) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ 4
def test_more_than_16_iterations(eng):
    pairs = (1, 4)
    scs = [pc.half_displaced(b) for b in pairs]
    obj, img, n = _stage(eng, [(o, u) for o, u, *_ in scs], 64)
    got = _pnp(eng, obj, img, n, cameras=_table(eng, pc.table_rows()[list(pairs)]), model=1, iterations=300)
    got_counts = eng.ransac_last_counts(2)
    for k, b in enumerate(pairs):
        o1, u1, n1 = _stage(eng, [(scs[k][0], scs[k][1])], 64)
        lone = _pnp(eng, o1, u1, n1, pc.KS[b], pc.DS[b], iterations=300)
        niters, evaluated = eng.ransac_last_counts(1)
        print(f"scene {b}, 50 % outliers, 300 requested: adapted count {niters[0]}, evaluated {evaluated[0]}, inliers {lone['n_inliers'][0]}")
        assert (got_counts[0][k], got_counts[1][k]) == (niters[0], evaluated[0]), (b, got_counts, niters, evaluated)
        assert 16 < niters[0] < 300                                                     # past the classic launches, and adapted
        assert not _differs(got, lone, k, 0), (b, _differs(got, lone, k, 0))
        assert lone["ok"][0] == 1 and np.array_equal(np.nonzero(lone["inlier_mask"][0])[0], np.nonzero(scs[k][4])[0]), b


# ------------------------------------------------------------------------------------------------------------------ whole path
EST_KEYS = ("R", "t", "n_match", "n_inliers", "ok", "cov", "sigma", "cov_ok", "inlier_mask", "inlier_idx", "reproj_err")
EIGHT_K = np.concatenate([pc.KS, pc.KS[:3] * np.array([[1.5, 1, 1], [1, 1, 1], [1, 1, 1]])])      # the five, then cameras 0 .. 2 with fx x 1.5
EIGHT_D = np.concatenate([pc.DS, pc.DS[:3]])


def _pair_for_camera(idx, n_q, n_r, K, d):
    """synthetic.make_pair's scene as camera (K, d) sees it: the query keypoints moved from K_MATRIX's pinhole pixels to the camera's own"""
    p = make_pair(idx, n_q=n_q, n_r=n_r)
    xn = (p.kp_q.astype(np.float64) - K_MATRIX[:2, 2]) / np.array([K_MATRIX[0, 0], K_MATRIX[1, 1]])
    xd, yd = ref.distort(xn[:, 0], xn[:, 1], d)
    kp = np.column_stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]]).astype(np.float32)
    return dataclasses.replace(p, kp_q=kp)


@pytest.fixture(scope="module")
def small():
    """The suite's small context (256 keypoints, synthetic weights, exact f32) and five pairs, pair b seen through camera b"""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    e = PoseEngine(0, max_batch=8, max_kpts=256, precision="f32", state_dict=synthetic_state_dict(0))
    pairs = [_pair_for_camera(7400 + i, 256 - 9 * i, 256 - 5 * i, pc.KS[i], pc.DS[i]) for i in range(5)]
    yield e, pairs, e.stage_inputs(pairs)
    del e


def _np(out, keys=EST_KEYS):
    return {k: out[k].cpu().numpy() for k in keys if k in out}


def _staged_per_pair(e, inp, Ks, Ds):
    """match -> gather_points for the batch, then pnp_ransac(report, covariance) of every pair ALONE under its camera, by value"""
    from gisnav_amd.engine import MIN_MATCHES
    B = inp["kpt_q"].shape[0]
    idx, _, n_match = e.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = e.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
    rows = []
    for b in range(B):
        e.set_distortion(Ds[b])
        try:
            res = e.pnp_ransac(obj[b:b + 1], mkp[b:b + 1], n_match[b:b + 1], Ks[b], min_pts=MIN_MATCHES, covariance=True, report=True)
            torch.cuda.synchronize()
        finally:
            e.set_distortion(None)
        row = {k: v.cpu().numpy()[0] for k, v in zip(PNP_KEYS, res)}
        row["n_match"] = n_match.cpu().numpy()[b]
        rows.append(row)
    return {k: np.stack([r[k] for r in rows]) for k in EST_KEYS}


@pytest.mark.parametrize("groups", [2, 4])
def test_estimate_with_groups_and_overlap_equals_each_pair_alone_by_value(small, groups):
    e, pairs, inp = small
    want = _staged_per_pair(e, inp, pc.KS, pc.DS)
    assert int(want["ok"].sum()) == 5 and int(want["cov_ok"].sum()) == 5
    cams, model = e.pair_cameras(pc.KS, pc.DS)
    out = e.alloc_outputs(5, covariance=True, report=True)
    try:
        e.set_substreams(groups)                                           # 5 pairs: groups of 3 + 2, or 2 + 1 + 1 + 1
        e.set_overlap(True)
        e.estimate(dict(inp, cameras=cams, camera_model=model), None, out=out, covariance=True, report=True)
        e.flush()
        torch.cuda.synchronize()
    finally:
        e.flush()
        e.set_overlap(False)
        e.set_substreams(1)
    got = _np(out)
    for b in range(5):
        diff = _differs(got, want, b, b, EST_KEYS)
        if pc.DS[b].any():      # the plumb-bob instantiation on both sides: the same bits
            assert not diff, (groups, b, diff)
            continue
        # pair 2: zero coefficients run through the plumb-bob instantiation; by value they select the pinhole one (gn_set_distortion: all zeros
        # = off).  As in test_five_cameras_equal_lone_by_value_calls: counts and index lists equal, poses at the 1e-8 bar, the covariance at 1e-9 scaled
        assert not set(diff) & {"n_match", "n_inliers", "ok", "cov_ok", "inlier_mask", "inlier_idx"}, (groups, b, diff)
        dR = float(np.linalg.norm(got["R"][b] - want["R"][b]))
        dt = float(np.linalg.norm(got["t"][b] - want["t"][b]) / np.linalg.norm(want["t"][b]))
        sd = np.sqrt(np.diag(want["cov"][b]))
        dc = float((np.abs(got["cov"][b] - want["cov"][b]) / np.outer(sd, sd)).max())
        k = int(want["n_match"][b])
        de = float(np.abs(got["reproj_err"][b, :k] - want["reproj_err"][b, :k]).max())
        print(f"groups={groups} pair {b} (zero coefficients) against the pinhole instantiation: dR {dR:.2e} dt {dt:.2e} cov {dc:.2e} residuals {de:.2e}")
        assert dR < 1e-8 and dt < 1e-8 and dc <= 1e-9 and abs(got["sigma"][b] - want["sigma"][b]) <= 1e-9 * want["sigma"][b], (groups, b)
        assert de <= 1e-4, (groups, b)      # f32 pixels: an ulp of a residual below 16 px is 1e-6
    # the cameras matter on this path: one camera for all five is another result
    same = e.estimate(inp, pc.KS[0])
    torch.cuda.synchronize()
    assert not np.array_equal(same["t"].cpu().numpy()[1:], got["t"][1:])


def test_two_pipelined_calls_keep_their_own_tables(small):
    e, pairs, inp = small
    tab_a, model = e.pair_cameras(pc.KS, pc.DS)
    tab_b, _ = e.pair_cameras(np.roll(pc.KS, 1, axis=0), np.roll(pc.DS, 1, axis=0))
    assert tab_a.data_ptr() != tab_b.data_ptr() and torch.equal(tab_b, torch.roll(tab_a, 1, 0))
    lone = []
    for tab in (tab_a, tab_b):
        o = e.estimate(dict(inp, cameras=tab, camera_model=model), None, covariance=True, report=True)
        torch.cuda.synchronize()
        lone.append(_np(o))
    assert _differs(lone[0], lone[1], keys=("R", "t"))
    out1, out2 = e.alloc_outputs(5, covariance=True, report=True), e.alloc_outputs(5, covariance=True, report=True)
    try:
        e.set_substreams(2, deferred_join=True)
        e.estimate(dict(inp, cameras=tab_a, camera_model=model), None, out=out1, covariance=True, report=True)
        e.estimate(dict(inp, cameras=tab_b, camera_model=model), None, out=out2, covariance=True, report=True)      # before the first call's PnP was joined
        e.flush()
        torch.cuda.synchronize()
    finally:
        e.flush()
        e.set_substreams(1)
    assert not _differs(_np(out1), lone[0], keys=EST_KEYS), _differs(_np(out1), lone[0], keys=EST_KEYS)
    assert not _differs(_np(out2), lone[1], keys=EST_KEYS), _differs(_np(out2), lone[1], keys=EST_KEYS)


# ------------------------------------------------------------------------------------------------------------------ 6
CB, CKPTS, CACTIVE = 7, 384, 256      # the shapes of tests/test_gpu_workspace_views.py (re-runs from a later pair)
CERT_K = EIGHT_K[:CB]
CERT_D = EIGHT_D[:CB]
CERT_KEYS = ("R", "t", "n_match", "n_inliers", "ok", "inlier_mask", "inlier_idx", "reproj_err")


def _cert_pairs(duplicates=()):
    """The pairs of tests/test_gpu_workspace_views.py, pair i seen through camera i.  duplicates: pairs whose first eight query keypoints are staged
    twice (descriptor, position, size and angle): two rows with equal scores, so a decision of those pairs has no margin at all and the certificate
    flags them at any eps, while every other pair keeps the margins of the synthetic weights (nothing flagged below eps = 0.5)."""
    pairs = [_pair_for_camera(8800 + i, 256 - 8 * i, 200 + 9 * i, CERT_K[i], CERT_D[i]) for i in range(CB)]
    dup = lambda a: np.concatenate([a, a[:8]])  # noqa: E731
    for i in duplicates:
        p = pairs[i]
        pairs[i] = dataclasses.replace(p, kp_q=dup(p.kp_q), desc_q=dup(p.desc_q), size_q=dup(p.size_q), angle_q=dup(p.angle_q))
        assert len(pairs[i].kp_q) <= CACTIVE
    return pairs


def _exact_f32(sd, pairs):
    """the exact-f32 context's call on `pairs` with the same table"""
    from gisnav_amd.engine import PoseEngine
    f32 = PoseEngine(0, max_batch=CB, max_kpts=CKPTS, precision="f32", state_dict=sd)
    f32.set_active_kpts(CACTIVE)
    o = f32.estimate(dict(f32.stage_inputs(pairs), cameras=f32.pair_cameras(CERT_K, CERT_D)[0], camera_model=1), None, report=True)
    torch.cuda.synchronize()
    exact = dict(_np(o, CERT_KEYS), idx=o["idx"].cpu().numpy())
    del f32
    return exact


@pytest.fixture(scope="module")
def cert():
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(0)
    fast = PoseEngine(0, max_batch=CB, max_kpts=CKPTS, precision="f16x2_f16_attn", state_dict=sd)
    assert fast.kmax == CKPTS and fast.set_active_kpts(CACTIVE) == CACTIVE
    cams, model = fast.pair_cameras(CERT_K, CERT_D)
    batches = {}
    for name, dups in (("plain", ()), ("scattered", (1, 3, 5))):
        pairs = _cert_pairs(dups)
        batches[name] = (dict(fast.stage_inputs(pairs), cameras=cams, camera_model=model), _exact_f32(sd, pairs))
    yield fast, batches
    del fast


def _cert_call(fast, inp, mode):
    """one estimate(report=True) with the table under the certificate `mode`, resolved; numpy outputs"""
    out = fast.alloc_outputs(CB, report=True)
    for v in out.values():
        v.zero_()
    fast.estimate(inp, None, out=out, report=True)
    fast.flush()                                                         # (deferred: the flags are read and the flagged pairs re-run here)
    torch.cuda.synchronize()
    return dict(_np(out, CERT_KEYS), idx=out["idx"].cpu().numpy())


def _assert_cert(got, exact, flagged, what):
    flagged = sorted(int(b) for b in flagged)
    rows = pc.table_rows(CERT_K, CERT_D)
    assert any(b >= 1 for b in flagged), (what, flagged)                  # a re-run that does not start at the first row of the table
    assert len(flagged) < CB, (what, flagged)                             # and a pair that keeps the fast arithmetic's result
    unflagged = [b for b in range(CB) if b not in flagged]
    assert all(rows[f].tobytes() != rows[u].tobytes() for f in flagged for u in unflagged), what      # different cameras on the two sides
    assert exact["ok"].all(), what
    for b in range(CB):
        k = int(exact["n_match"][b])
        assert got["n_match"][b] == k and np.array_equal(got["idx"][b, :k], exact["idx"][b, :k]), (what, b, "idx")
        assert got["ok"][b] == 1 and got["n_inliers"][b] == exact["n_inliers"][b], (what, b)
        assert np.array_equal(got["inlier_idx"][b], exact["inlier_idx"][b]) and np.array_equal(got["inlier_mask"][b, :k], exact["inlier_mask"][b, :k]), (what, b)
        if b in flagged:      # the exact-f32 kernels on the same inputs with the pair's own camera: the same bits
            assert not _differs(got, exact, b, b, ("R", "t")), (what, b, "re-run pair")
            assert np.array_equal(got["reproj_err"][b, :k].view(np.uint32), exact["reproj_err"][b, :k].view(np.uint32)), (what, b)
        else:
            dR = float(np.linalg.norm(got["R"][b] - exact["R"][b]))
            dt = float(np.linalg.norm(got["t"][b] - exact["t"][b]) / np.linalg.norm(exact["t"][b]))
            assert dR < 1e-8 and dt < 1e-8, (what, b, dR, dt)
            assert np.abs(got["reproj_err"][b, :k] - exact["reproj_err"][b, :k]).max() < 1e-4, (what, b)


@pytest.mark.parametrize("mode", ["rerun", "deferred"])
def test_a_rerun_in_place_from_a_later_pair_keeps_its_cameras(cert, mode):
    """Group 1 of two (pairs 4 .. 6) starts with its guard word raised (developer knob 25): its pairs are re-run in exact f32 in place, on the call
    sliced at pair 4 -- the table pointer must have advanced with the other per-pair pointers."""
    fast, batches = cert
    inp, exact = batches["plain"]
    knob = lambda v: fast.lib.gn_debug_set_variant(fast.ctx, 25, v)  # noqa: E731
    try:
        fast.set_substreams(2)
        fast.set_certify(mode, eps=1.0e-7)
        fast.certify_stats(reset=True)
        assert knob(2) == 0
        got = _cert_call(fast, inp, mode)
        st = fast.certify_stats(reset=True)
    finally:
        knob(0)
        fast.flush()
        fast.set_certify("off")
        fast.set_substreams(1)
    assert st["flagged_fp16_range"] == 3 and st["flagged_margin"] == 0 and st["rerun_pairs"] == 3, st
    _assert_cert(got, exact, [4, 5, 6], f"in place, {mode}")


def _scattered_eps(fast, inp):
    """An eps at which the margin certificate flags a set of pairs that is not one contiguous run (so the re-run gathers them) and not all of them:
    (eps, flagged pairs, what was seen).  Found on the flags alone ("flag" mode, no re-run) from fixed candidates: 1e-3 (the pairs with duplicated
    keypoints and nobody else), then a fine ladder over the range in which the synthetic weights' own margins lie."""
    seen = []
    try:
        fast.set_substreams(1)
        for eps in [1.0e-3] + np.geomspace(0.5, 1.0, 24).tolist():
            fast.set_certify("flag", eps=eps)
            fast.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
            flags = fast.uncertain(CB)
            fl = np.nonzero(flags)[0].tolist()
            seen.append((eps, fl))
            if 2 <= len(fl) < CB and fl[-1] - fl[0] + 1 != len(fl) and (flags[fl] == 1).all():
                return eps, fl, seen
    finally:
        fast.set_certify("off")
    return None, None, seen


@pytest.mark.parametrize("mode", ["rerun", "deferred"])
def test_a_gathered_rerun_takes_every_pairs_camera_with_it(cert, mode):
    """Scattered flagged pairs are gathered into the staging block for one batched exact-f32 call: slot k of that call must be solved with the
    camera of flagged pair k, not with row k of the table."""
    fast, batches = cert
    inp, exact = batches["scattered"]
    eps, flagged, seen = _scattered_eps(fast, inp)
    assert eps is not None, f"no candidate eps flags a scattered proper subset of the pairs: {seen}"
    print(f"eps {eps:.3e} flags pairs {flagged}")
    try:
        fast.set_substreams(2)
        fast.set_certify(mode, eps=eps)
        fast.certify_stats(reset=True)
        got = _cert_call(fast, inp, mode)
        st = fast.certify_stats(reset=True)
    finally:
        fast.flush()
        fast.set_certify("off")
        fast.set_substreams(1)
    assert st["flagged_margin"] == len(flagged) and st["flagged_fp16_range"] == 0 and st["rerun_pairs"] == len(flagged), (st, flagged)
    _assert_cert(got, exact, flagged, f"gathered, {mode}")


# ------------------------------------------------------------------------------------------------------------------ 7
def test_estimate_bucketed_keeps_every_pairs_camera(small):
    e = small[0]
    counts = (60, 250, 130, 200, 90, 256, 40, 180)
    pairs = [_pair_for_camera(7500 + i, n, n, EIGHT_K[i], EIGHT_D[i]) for i, n in enumerate(counts)]
    inp = e.stage_inputs(pairs)
    n_host = np.array(counts)
    assert np.argsort(-n_host, kind="stable").tolist() != list(range(8))
    cams, model = e.pair_cameras(EIGHT_K, EIGHT_D)
    out, stats = e.estimate_bucketed(dict(inp, cameras=cams, camera_model=model), None, n_host, n_host, bucket_pairs=3, report=True)
    torch.cuda.synchronize()
    assert stats["groups"] == 3
    got = dict(_np(out), idx=out["idx"].cpu().numpy())
    n_ok = 0
    for b in range(8):
        one = e.stage_inputs(pairs[b:b + 1])
        e.set_active_kpts(counts[b])
        e.set_distortion(EIGHT_D[b])
        try:
            lone = e.estimate(one, EIGHT_K[b], report=True)
            torch.cuda.synchronize()
        finally:
            e.set_distortion(None)
            e.set_active_kpts(e.kmax)
        w = {k: v.cpu().numpy()[0] for k, v in lone.items()}
        k = int(w["n_match"])
        assert got["n_match"][b] == k and np.array_equal(got["idx"][b, :k], w["idx"][:k]), (b, "idx")
        assert got["ok"][b] == w["ok"] and got["n_inliers"][b] == w["n_inliers"] and np.array_equal(got["inlier_idx"][b], w["inlier_idx"]), b
        if w["ok"]:
            n_ok += 1
            dR = float(np.linalg.norm(got["R"][b] - w["R"]))
            dt = float(np.linalg.norm(got["t"][b] - w["t"]) / np.linalg.norm(w["t"]))
            print(f"pair {b} ({counts[b]} keypoints): dR {dR:.2e} dt {dt:.2e}")
            assert dR < 1e-8 and dt < 1e-8, (b, dR, dt)
    assert n_ok >= 3


# ------------------------------------------------------------------------------------------------------------------ 8
def test_vo_estimate_with_three_cameras_equals_lone_calls_bitwise(small):
    e, pairs, inp = small
    sel = [0, 1, 3]
    sub = {k: (v[sel].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    cams, model = e.pair_cameras(pc.KS[sel])
    assert model == 0
    out = e.vo_estimate(dict(sub, cameras=cams, camera_model=model), None, ratio=0.9, min_matches=15, covariance=True, report=True)
    torch.cuda.synchronize()
    got = _np(out)
    assert int(got["ok"].sum()) > 0
    for k, b in enumerate(sel):
        one = {key: (v[k:k + 1].contiguous() if isinstance(v, torch.Tensor) else v) for key, v in sub.items()}
        lone = e.vo_estimate(one, pc.KS[b], ratio=0.9, min_matches=15, covariance=True, report=True)
        torch.cuda.synchronize()
        assert not _differs(got, _np(lone), k, 0, EST_KEYS), (b, _differs(got, _np(lone), k, 0, EST_KEYS))
    one_camera = e.vo_estimate(sub, pc.KS[0], ratio=0.9, min_matches=15)
    torch.cuda.synchronize()
    assert not np.array_equal(one_camera["t"].cpu().numpy()[1:], got["t"][1:])      # the rows reach this path's PnP


# ------------------------------------------------------------------------------------------------------------------ 9
def test_loftr_pose_batch_with_two_cameras():
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.loftr import LoFTR, loftr_pose, loftr_pose_batch
    from oracle import loftr as lf
    h, w = 128, 160                                                       # the smallest size of tests/test_loftr_batch.py
    sd = lf.synthetic_state_dict(0)
    pairs = [lf.synthetic_pair(1, h, w), lf.synthetic_pair(2, h, w, shift=(24, 16))]
    dem = (10 + 8 * np.sin(np.arange(h)[:, None] / 30.0) * np.cos(np.arange(w)[None, :] / 45.0)).astype(np.uint8)
    Ks = np.stack([pc.k_matrix(120.0, 118.0, 80.0, 64.0), pc.k_matrix(95.0, 97.0, 77.5, 66.0)])
    Ds = np.stack([pc.DS[1], np.zeros(5)])                                # distortion for the first camera only
    m = LoFTR(state_dict=sd).to("cuda:0").eval()
    m1 = LoFTR(state_dict=sd).to("cuda:0").eval()
    eng = PoseEngine(0, max_batch=2, max_kpts=1024, precision="f32")
    f = torch.stack([p[0] for p in pairs]).cuda()
    t = torch.stack([p[1] for p in pairs]).cuda()
    got = loftr_pose_batch(m, eng, f, t, [dem] * 2, Ks, dist=Ds, return_covariance=True, return_inliers=True)
    got_k = loftr_pose_batch(m, eng, f, t, [dem] * 2, Ks, return_inliers=True)                       # K alone: the pinhole kernels for both
    one_camera = loftr_pose_batch(m, eng, f, t, [dem] * 2, Ks[0], dist=Ds[0], return_inliers=True)   # today's path
    assert len(got) == len(got_k) == 2
    n_pose = 0
    for b in range(2):
        want = loftr_pose(m1, eng, pairs[b][0].cuda(), pairs[b][1].cuda(), dem, Ks[b], return_covariance=True, dist=Ds[b], return_inliers=True)
        want_k = loftr_pose(m1, eng, pairs[b][0].cuda(), pairs[b][1].cuda(), dem, Ks[b], return_inliers=True)
        assert (want is None) == (got[b] is None) and (want_k is None) == (got_k[b] is None), b
        if want_k is not None:      # K alone: the pinhole instantiation on both sides, the same bits
            assert np.array_equal(got_k[b][0], want_k[0]) and np.array_equal(got_k[b][1], want_k[1]) and got_k[b][2] == want_k[2], b
            assert np.array_equal(got_k[b][-1], want_k[-1]), b
        if want is None:
            continue
        n_pose += 1
        assert got[b][2] == want[2] and np.array_equal(got[b][-1], want[-1]), b
        if Ds[b].any():             # the plumb-bob instantiation on both sides: the same bits
            assert np.array_equal(got[b][0], want[0]) and np.array_equal(got[b][1], want[1]), b
            assert (want[3] is None) == (got[b][3] is None) and (want[3] is None or np.array_equal(got[b][3], want[3])), b
        else:                       # zero coefficients through the plumb-bob instantiation against loftr_pose's pinhole one: rounding only
            dR = float(np.linalg.norm(got[b][0] - want[0]))
            dt = float(np.linalg.norm(got[b][1] - want[1]) / np.linalg.norm(want[1]))
            assert dR < 1e-8 and dt < 1e-8, (b, dR, dt)
    assert n_pose >= 1
    if got[1] is not None and one_camera[1] is not None:
        assert not np.array_equal(got[1][1], one_camera[1][1])            # pair 1 was not solved with pair 0's camera


# ------------------------------------------------------------------------------------------------------------------ 10
def test_compute_pose_batch_equals_compute_pose_per_message(eng):
    from gisnav_amd import wire
    from gisnav_amd.pose import compute_pose, compute_pose_batch
    infos, qry, refs, dems = [], [], [], []
    sizes = ((480, 640), (480, 640), (500, 600), (360, 640), (720, 1280))
    for b, (o, u, *_) in enumerate(pc.scenes()):
        dem = np.zeros((480, 640), np.uint8)
        cell = np.floor(o[:, :2]).astype(int)
        dem[cell[:, 1], cell[:, 0]] = o[:, 2].astype(np.uint8)
        infos.append(wire.CameraInfo(k=pc.KS[b].reshape(9), height=sizes[b][0], width=sizes[b][1], d=pc.DS[b], distortion_model="plumb_bob"))
        qry.append(u); refs.append(o[:, :2]); dems.append(dem)
    # a message below the minimum in the middle: None in its slot, the others unmoved
    infos.insert(2, infos[0]); qry.insert(2, qry[0][:3]); refs.insert(2, refs[0][:3]); dems.insert(2, None)
    got = compute_pose_batch(infos, qry, refs, dems, use_distortion=True, return_inliers=True, engine=eng)
    assert len(got) == 6 and got[2] is None
    del got[2], infos[2], qry[2], refs[2], dems[2]
    for b in range(pc.NB):
        want = compute_pose(infos[b], qry[b], refs[b], dems[b], engine=eng, use_distortion=True, return_inliers=True)
        assert want is not None and got[b] is not None, b
        assert got[b][0].shape == (3, 3) and got[b][1].shape == (3, 1) and got[b][2].dtype == np.int32 and got[b][2].shape == (pc.TRUE_INLIERS[b], 1)
        assert np.array_equal(got[b][2], want[2]), b
        if pc.DS[b].any():
            assert np.array_equal(got[b][0], want[0]) and np.array_equal(got[b][1], want[1]), b
        else:      # compute_pose runs a camera without coefficients on the pinhole kernels; the batch runs it through the plumb-bob ones
            assert np.linalg.norm(got[b][0] - want[0]) < 1e-8 and np.linalg.norm(got[b][1] - want[1]) / np.linalg.norm(want[1]) < 1e-8, b
    assert eng.distortion() is None and _lib.load().gn_get_pair_cameras(eng.ctx, None, None, None) == 0
    # without use_distortion: the pinhole kernels, every message bitwise compute_pose's
    plain = compute_pose_batch(infos, qry, refs, dems, engine=eng)
    for b in range(pc.NB):
        want = compute_pose(infos[b], qry[b], refs[b], dems[b], engine=eng)
        assert (want is None) == (plain[b] is None), b
        if want is not None:
            assert len(plain[b]) == 2 and np.array_equal(plain[b][0], want[0]) and np.array_equal(plain[b][1], want[1]), b


# ------------------------------------------------------------------------------------------------------------------ 11
def _get(lib, ctx):
    p, n, m = ctypes.c_void_p(0), ctypes.c_int(-1), ctypes.c_int(-1)
    on = lib.gn_get_pair_cameras(ctx, ctypes.byref(p), ctypes.byref(n), ctypes.byref(m))
    return on, p.value, n.value, m.value


def test_off_is_off_refusals_and_the_stored_distortion(eng):
    from gisnav_amd.engine import PoseEngine
    lib = _lib.load()
    o, u, _, _, inl = ref.make_scene(40, 1, False)
    batch = [(o[inl][:4], u[inl][:4]), (o[inl][:5], u[inl][:5]), (o, u)]
    obj, img, n = _stage(eng, batch, 64)
    assert n.tolist() == [4, 5, 40]
    K, D = ref.K_TEST, ref.D_TEST
    run = lambda e: [x.cpu().numpy().tobytes() for x in e.pnp_ransac(obj, img, n, K, min_pts=4, covariance=True)]  # noqa: E731
    never = PoseEngine(0, max_batch=4, max_kpts=128)                       # a context that never saw a table
    want = run(never)
    never.set_distortion(D)
    want_d = run(never)                                                   # ... and one that only ever had the coefficients
    del never
    e = PoseEngine(0, max_batch=4, max_kpts=128)
    err_arg = lib.gn_set_distortion(None, None, 0)
    tab = _table(e, np.repeat(pc.table_rows()[1:2], 3, axis=0))           # camera 1 for all three: not K, not D
    e.set_distortion(D)
    assert _get(lib, e.ctx) == (0, None, 0, 0)
    assert lib.gn_set_pair_cameras(e.ctx, ctypes.c_void_p(tab.data_ptr()), 3, 1) == 0
    assert _get(lib, e.ctx) == (1, tab.data_ptr(), 3, 1)
    with_table = run(e)                                                   # K and the stored coefficients are ignored
    assert with_table[0] != want_d[0] and with_table[0] != want[0]
    # refusals: GN_ERR_ARG, the setter's name in gn_last_error, the earlier state still reported
    for cams, cnt, model in ((tab, 3, 2), (tab, 3, -1), (tab, 5, 1), (tab, -1, 1)):      # model outside {0, 1}; n > max_batch (4); n < 0
        assert lib.gn_set_pair_cameras(e.ctx, ctypes.c_void_p(cams.data_ptr()), cnt, model) == err_arg, (cnt, model)
        assert b"gn_set_pair_cameras" in lib.gn_last_error(e.ctx), (cnt, model)
        assert _get(lib, e.ctx) == (1, tab.data_ptr(), 3, 1)
    obj4, img4, n4 = _stage(e, batch + batch[:1], 64)                      # B = 4 > n = 3
    with pytest.raises(_lib.GnError, match="gn_set_pair_cameras"):
        e.pnp_ransac(obj4, img4, n4, K, min_pts=4)
    with pytest.raises(_lib.GnError, match="gn_set_pair_cameras"):
        e.undistort_points(img4, n4, K)
    assert _get(lib, e.ctx) == (1, tab.data_ptr(), 3, 1)
    # unset: the stored gn_set_distortion coefficients apply again, bit for bit
    assert lib.gn_set_pair_cameras(e.ctx, None, 0, 0) == 0
    assert _get(lib, e.ctx) == (0, None, 0, 0)
    assert np.array_equal(e.distortion(), D)
    assert run(e) == want_d
    e.set_distortion(None)
    assert run(e) == want                                                 # set-then-unset against the context that never saw a table
    assert lib.gn_set_pair_cameras(e.ctx, ctypes.c_void_p(tab.data_ptr()), 0, 1) == 0 and _get(lib, e.ctx) == (0, None, 0, 0)      # n = 0: off
    del e

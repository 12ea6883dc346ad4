"""Report of the pose stage on the GPU: gn_pnp_ransac_report / gn_estimate_report / gn_vo_estimate_report (DESIGN.md "Report of the pose stage").

  1. against the oracle, one call: 4 / 5 / 12 / 63 / 65 / 130 / 300 points at stride 384 -- inlier_idx is the oracle's `inliers`, inlier_mask its
     indicator, reproj_err the fp64 residual at the GPU's own pose, R / t / n_inliers / ok bit for bit gn_pnp_ransac's;
  2. the round path (iterations_count = 300);
  3. distortion on;
  4. through every call path of gn_estimate_report: bitwise the staged match -> gather_points -> pnp_ransac(report=True);
  5. gn_vo_estimate_report against its staged path;
  6. off means off;
  7. the Python seams: compute_pose / twist_pose / loftr_pose(_batch)(return_inliers=True), PoseNode(report=True).last_report.

Every report array is allocated with one row more than the call has pairs and filled with poison: a kernel that leaves a slot unwritten, or writes
past its row into the canary row, fails an assertion.  The scenes are the constants of tests/pnp_report_scenes.py; tests/test_pnp_report_host.py
shows from the oracle alone that their inlier sets do not depend on the last bits of the scoring.

The residual bound is the one of gn_undistort_points (tests/test_gpu_pnp_distortion.py): the GPU forms the residual in double from fused
multiply-adds, the reference from separate operations and through R -> rvec -> R, so the two doubles differ by a few ulp of the PIXEL COORDINATES
(~1e-13 px) before the one rounding to f32: one f32 ulp of max(|value|, 1).  (In ulps of the residual itself a noise-free inlier, whose residual
is 1e-6 px, shows that 1e-13 px as several ulp -- the reference's own round trip through rvec does the same against a projection with R.)
"""
import numpy as np
import pytest
import torch

import pnp_distorted_ref as ref
import pnp_report_scenes as S
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu

POISON = dict(inlier_mask=7, inlier_idx=7777, reproj_err=7.0, idx=-7777, score=-7.0)
REPORT_KEYS = ("inlier_mask", "inlier_idx", "reproj_err")
OLD_KEYS = ("R", "t", "n_match", "n_inliers", "ok")


def _stage(eng, scenes, stride):
    B = len(scenes)
    obj, img, n = np.zeros((B, stride, 3), np.float32), np.zeros((B, stride, 2), np.float32), np.zeros(B, np.int32)
    for b, (o, u) in enumerate(scenes):
        obj[b, :len(o)], img[b, :len(o)], n[b] = o, u, len(o)
    d = eng.device
    return torch.from_numpy(obj).to(d), torch.from_numpy(img).to(d), torch.from_numpy(n).to(d)


def _poisoned(eng, B, stride, keys=REPORT_KEYS):
    """Report arrays of B + 1 rows filled with poison; the call gets the first B rows, row B is the canary."""
    dt = dict(inlier_mask=torch.uint8, inlier_idx=torch.int32, reproj_err=torch.float32, idx=torch.int64, score=torch.float32)
    full = {k: torch.full((B + 1, stride, 2) if k == "idx" else (B + 1, stride), POISON[k], dtype=dt[k], device=eng.device) for k in keys}
    return full, {k: v[:B] for k, v in full.items()}


def _canary_untouched(full):
    return all(bool((v[-1] == POISON[k]).all()) for k, v in full.items())


def _solve(eng, scenes, K, stride, iterations=10, min_pts=S.MIN_PTS):
    """One report call on poisoned outputs and the plain call on the same inputs -> (report call's host results, plain call's, canary ok)."""
    obj, img, n = _stage(eng, scenes, stride)
    full, view = _poisoned(eng, len(scenes), stride)
    res = eng.pnp_ransac(obj, img, n, K, iterations=iterations, min_pts=min_pts, report=True, report_out=view)
    plain = eng.pnp_ransac(obj, img, n, K, iterations=iterations, min_pts=min_pts)
    torch.cuda.synchronize()
    assert len(res) == 7 and len(plain) == 4
    return [x.cpu().numpy() for x in res], [x.cpu().numpy() for x in plain], _canary_untouched(full)


def _check(label, scenes, res, plain, want_inl, residual, min_pts):
    """The assertions of tests 1 - 3.  want_inl[b]: the oracle's inlier indices, or None where it finds no pose; residual(b, R, t): fp64 residuals
    (n,) of scene b at the pose (R, t)."""
    R, t, n_inl, ok, mask, idx, err = res
    for name, a, b_ in zip(("R", "t", "n_inliers", "ok"), plain, res):
        assert a.tobytes() == b_.tobytes(), (label, name)                     # nothing else moves
    stride = mask.shape[1]
    worst, worst_own = 0.0, 0.0
    for b, (o, u) in enumerate(scenes):
        n = len(o)
        expect_ok = n >= max(min_pts, 4) and want_inl[b] is not None
        assert bool(ok[b]) == expect_ok, (label, b, n)
        if not expect_ok:                                                     # all sentinels
            assert not mask[b].any() and (idx[b] == -1).all() and (err[b] == -1.0).all(), (label, b)
            continue
        inl = np.asarray(want_inl[b]).reshape(-1)
        assert n_inl[b] == len(inl), (label, b, n_inl[b], len(inl))
        assert np.array_equal(idx[b, :len(inl)], inl) and (idx[b, len(inl):] == -1).all(), (label, b)
        ind = np.zeros(stride, np.uint8); ind[inl] = 1
        assert np.array_equal(mask[b], ind), (label, b)
        assert (err[b, n:] == -1.0).all(), (label, b)
        want = residual(b, R[b], t[b]).astype(np.float32)
        d = np.abs(err[b, :n].astype(np.float64) - want.astype(np.float64))
        bound = np.spacing(np.maximum(np.abs(want), np.float32(1.0))).astype(np.float64)
        own = d / np.spacing(np.abs(want)).astype(np.float64)
        print(f"{label} pair {b}: n = {n}, inliers {len(inl)}, residuals {want.min():.2e} .. {want.max():.2e} px, largest difference {d.max():.2e} px = "
              f"{(d / bound).max():.2e} ulp of max(|value|, 1), {own.max():.1f} ulp of the residual itself")
        worst, worst_own = max(worst, float((d / bound).max())), max(worst_own, float(own.max()))
        assert (d <= bound).all(), (label, b, float((d / bound).max()))
    print(f"{label}: measured maximum {worst:.2e} ulp of max(|value|, 1) ({worst_own:.1f} ulp of the residual itself)")


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=8, max_kpts=S.KSTRIDE)
    yield e
    del e


def _pinhole_residual(scenes, K):
    def f(b, R, t):
        o, u = scenes[b]
        p = pr.project_points(o.astype(np.float64), pr.rodrigues_mat2vec(R), np.asarray(t).reshape(3), K)
        e = p - u.astype(np.float64)
        return np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    return f


# ------------------------------------------------------------------------------------------------------------------ 1
def test_one_call_against_the_oracle(eng):
    """B = 7, kstride = 384, min_pts = 15: the 4-, 5- and 12-point pairs are below min_pts and come back as sentinels, 63 / 65 / 130 / 300 carry
    the compaction base over one, two, three and five 64-lane chunks.  The same inputs once more with min_pts = 4, so that the 4-point (P3P) and
    5-point branches, where every point is an inlier, are run as well (the 12-point pair is then an ordinary RANSAC pair).  Fails on a library
    without gn_pnp_ransac_report."""
    scenes = S.one_call_scenes()
    assert eng.kmax == S.KSTRIDE
    oracle = [pr.solve_pnp_ransac(o, u, S.K, 10, S.REPROJ) for o, u in scenes]
    want_inl = [w[3] if w[0] else None for w in oracle]
    assert all(w is not None for w in want_inl)
    for min_pts in (S.MIN_PTS, 4):
        res, plain, canary = _solve(eng, scenes, S.K, S.KSTRIDE, min_pts=min_pts)
        assert canary
        _check(f"min_pts={min_pts}", scenes, res, plain, want_inl, _pinhole_residual(scenes, S.K), min_pts)
        ok = res[3]
        assert ok.tolist() == ([0, 0, 0, 1, 1, 1, 1] if min_pts == S.MIN_PTS else [1] * 7)
    mask = res[4]
    assert mask[0, :4].all() and mask[1, :5].all() and int(mask[6].sum()) < 300          # every point in the small branches; outliers rejected


def test_each_report_pointer_is_optional(eng):
    """Any subset of the three arrays gives the same bytes in those that are asked for; none at all is gn_pnp_ransac(_cov)."""
    scenes = S.one_call_scenes()[3:5]
    obj, img, n = _stage(eng, scenes, 128)
    full, view = _poisoned(eng, 2, 128)
    eng.pnp_ransac(obj, img, n, S.K, report=True, report_out=view)
    torch.cuda.synchronize()
    for keep in REPORT_KEYS:
        f1, v1 = _poisoned(eng, 2, 128, (keep,))
        res = eng.pnp_ransac(obj, img, n, S.K, report=True, report_out=v1, covariance=True)
        torch.cuda.synchronize()
        assert len(res) == 10 and torch.equal(f1[keep], full[keep]), keep
        assert bool(res[6].all())                                                       # the covariance trio rides along
    none = eng.pnp_ransac(obj, img, n, S.K, report=True, report_out={})
    plain = eng.pnp_ransac(obj, img, n, S.K)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(none[:4], plain)) and none[4:] == (None, None, None)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_round_path(eng):
    """iterations_count = 300 goes through k_pnp_round / k_pnp_select: the winner's mask is slot 64 of the round workspace.  The expected inlier sets
    are the golden file's, which holds what solve_pnp_ransac(..., 300) returns (tests/test_ransac_iterations_host.py checks that)."""
    scenes, K = S.round_scenes()
    g = np.load(S.GOLDEN)
    want_inl = []
    for s in S.ROUND_SCENES:
        i = list(g[f"{s}_counts"]).index(S.ROUND_COUNT)
        assert int(g[f"{s}_ok"][i]) == 1
        want_inl.append(np.nonzero(g[f"{s}_inl"][i])[0])
    res, plain, canary = _solve(eng, scenes, K, 128, iterations=S.ROUND_COUNT)
    assert canary
    _check("round path", scenes, res, plain, want_inl, _pinhole_residual(scenes, K), S.MIN_PTS)
    assert [int(v) for v in res[2]] == [30, 30]


# ------------------------------------------------------------------------------------------------------------------ 3
def test_distortion_on(eng):
    scenes = S.dist_scenes()
    oracle = [ref.solve_pnp_ransac_dist(o, u, S.K, S.D, 10, S.REPROJ) for o, u in scenes]
    want_inl = [w[3] if w[0] else None for w in oracle]

    def residual(b, R, t):
        o, u = scenes[b]
        p = ref.project_points_dist(o.astype(np.float64), pr.rodrigues_mat2vec(R), np.asarray(t).reshape(3), S.K, S.D)
        e = p - u.astype(np.float64)
        return np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    eng.set_distortion(S.D)
    try:
        res, plain, canary = _solve(eng, scenes, S.K, 128)
    finally:
        eng.set_distortion(None)
    assert canary
    _check("distortion on", scenes, res, plain, want_inl, residual, S.MIN_PTS)
    off, _, _ = _solve(eng, scenes, S.K, 128)
    assert not np.array_equal(off[6], res[6])                                           # the residuals do go through the distortion


# ------------------------------------------------------------------------------------------------------------------ 4 - 6
ALL_KEYS = OLD_KEYS + ("idx", "score") + REPORT_KEYS


@pytest.fixture(scope="module")
def call_paths():
    """B = 4 pairs of 256 keypoints, the last cut to 12 query keypoints (fewer than MIN_MATCHES matches: an all-sentinel report); the staged
    path match -> gather_points -> pnp_ransac(report=True) on an f32 context is the reference of every estimate(report=True) variant."""
    from gisnav_amd.engine import MIN_MATCHES, PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(0)
    pairs = [make_pair(7300 + i, n_q=256 - 9 * i, n_r=256 - 5 * i) for i in range(3)] + [make_pair(7303, n_q=12, n_r=241)]
    f32 = PoseEngine(0, max_batch=4, max_kpts=256, precision="f32", state_dict=sd)
    inp = f32.stage_inputs(pairs)
    base = {k: v.clone() for k, v in f32.estimate(inp, K_MATRIX).items()}                # the call without the report, before any report call
    idx, score, n_match = f32.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = f32.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
    R, t, n_inl, ok, mask, iidx, err = f32.pnp_ransac(obj, mkp, n_match, K_MATRIX, min_pts=MIN_MATCHES, report=True)
    torch.cuda.synchronize()
    want = dict(R=R, t=t, n_match=n_match, n_inliers=n_inl, ok=ok, idx=idx, score=score, inlier_mask=mask, inlier_idx=iidx, reproj_err=err)
    want = {k: v.clone() for k, v in want.items()}
    assert want["ok"].tolist() == [1, 1, 1, 0] and int(want["n_match"][3]) < MIN_MATCHES
    assert not want["inlier_mask"][3].any() and bool((want["inlier_idx"][3] == -1).all()) and bool((want["reproj_err"][3] == -1).all())
    assert not _diff(base, want, OLD_KEYS)
    # Two sub-stream groups run the matcher as two 2-pair calls, and calls of one or two pairs use the small-grid kernel family, whose summation
    # order differs from the bulk kernels' (PoseEngine.estimate_bucketed): the same matches, scores that differ in the last bits.  The staged
    # reference of those modes is therefore the staged matcher on the same two 2-pair calls -- idx must still be the 4-pair call's.
    halves = [f32.match(*(inp[k][a:a + 2] for k in ("desc_q", "kpt_q", "n_q", "desc_r", "kpt_r", "n_r"))) for a in (0, 2)]
    torch.cuda.synchronize()
    grouped = dict(want, idx=torch.cat([h[0] for h in halves]), score=torch.cat([h[1] for h in halves]))
    assert torch.equal(torch.cat([h[2] for h in halves]), want["n_match"]) and not _diff(grouped, want, ("idx",))
    want["grouped"] = grouped
    yield sd, pairs, f32, inp, want, base
    del f32


def _diff(got, want, keys=ALL_KEYS):
    """Keys whose bytes differ; idx and score are defined in their first n_match rows (the matcher writes no more)."""
    bad = []
    for k in keys:
        g, w = got[k].reshape(want[k].shape), want[k]
        if k in ("idx", "score"):
            same = all(torch.equal(g[b, :int(want["n_match"][b])], w[b, :int(want["n_match"][b])]) for b in range(w.shape[0]))
        else:
            same = torch.equal(g, w)
        if not same:
            bad.append(k)
    return bad


def _poisoned_outputs(e, B):
    out = e.alloc_outputs(B)
    full, view = _poisoned(e, B, e.kmax, ("idx", "score") + REPORT_KEYS)
    out.update(view)
    return out, full


@pytest.mark.parametrize("mode", ["plain", "overlap", "substreams", "deferred_join"])
def test_estimate_report_on_an_f32_context_equals_the_staged_path_bitwise(call_paths, mode):
    sd, pairs, f32, inp, want, base = call_paths
    assert sorted(f32.alloc_outputs(4, report=True)) == sorted(ALL_KEYS)
    out, full = _poisoned_outputs(f32, 4)
    try:
        if mode == "overlap":
            f32.set_overlap(True)
        elif mode == "substreams":
            f32.set_substreams(2)
        elif mode == "deferred_join":
            f32.set_substreams(2, deferred_join=True)
        f32.estimate(inp, K_MATRIX, out=out, report=True)
        if mode in ("overlap", "deferred_join"):
            f32.flush()
        torch.cuda.synchronize()
    finally:
        f32.flush()
        f32.set_overlap(False)
        f32.set_substreams(1)
    staged = want["grouped"] if mode in ("substreams", "deferred_join") else want
    assert not _diff(out, staged), (mode, _diff(out, staged))
    assert not _diff(out, base, OLD_KEYS)                                               # the old outputs are those of a call without the report
    assert _canary_untouched(full)
    # row k of the report refers to row k of idx: an inlier's index is below n_match, and its residual is a number
    nm, ni = want["n_match"].tolist(), want["n_inliers"].tolist()
    for b in range(3):
        rows = out["inlier_idx"][b, :ni[b]]
        assert int(rows.max()) < nm[b] and bool((out["reproj_err"][b, :nm[b]] >= 0).all()) and bool((out["reproj_err"][b, nm[b]:] == -1).all())


@pytest.mark.parametrize("mode", ["rerun", "substreams_deferred_certificate"])
def test_estimate_report_through_the_certificate_rerun_equals_the_f32_context_bitwise(call_paths, mode):
    """eps = inf flags every pair: all four go through the gathered exact-f32 re-run and its scatter, which must carry the match list and the
    three report arrays."""
    from gisnav_amd.engine import PoseEngine
    sd, pairs, f32, _, want, base = call_paths
    fast = PoseEngine(0, max_batch=4, max_kpts=256, precision="f16x2_f16_attn", state_dict=sd)
    inp = fast.stage_inputs(pairs)
    out, full = _poisoned_outputs(fast, 4)
    fast.certify_stats(reset=True)
    if mode == "rerun":
        fast.set_certify("rerun", eps=float("inf"))
        fast.estimate(inp, K_MATRIX, out=out, report=True)
    else:
        fast.set_substreams(2)
        fast.set_certify("deferred", eps=float("inf"))
        fast.estimate(inp, K_MATRIX, out=out, report=True)
        fast.flush()
    torch.cuda.synchronize()
    st = fast.certify_stats()
    fast.set_certify("off")
    fast.set_substreams(1)
    del fast
    assert st["rerun_pairs"] == 4, st
    assert not _diff(out, want), (mode, _diff(out, want))
    assert not _diff(out, base, OLD_KEYS)
    assert _canary_untouched(full)


def test_vo_estimate_report_equals_its_staged_path_bitwise(call_paths):
    sd, pairs, f32, inp4, _, _ = call_paths
    inp = {k: (v[:2] if isinstance(v, torch.Tensor) else v) for k, v in inp4.items()}
    out, full = _poisoned_outputs(f32, 2)
    f32.vo_estimate(inp, K_MATRIX, ratio=0.9, min_matches=15, out=out, report=True)
    idx, dist, n_good = f32.vo_match(inp["desc_q"], inp["n_q"], inp["desc_r"], inp["n_r"], ratio=0.9)
    mkp, obj = f32.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_good, None)
    R, t, n_inl, ok, mask, iidx, err = f32.pnp_ransac(obj, mkp, n_good, K_MATRIX, min_pts=15, report=True)
    plain = f32.vo_estimate(inp, K_MATRIX, ratio=0.9, min_matches=15)
    torch.cuda.synchronize()
    want = dict(R=R, t=t, n_match=n_good, n_inliers=n_inl, ok=ok, idx=idx, score=dist, inlier_mask=mask, inlier_idx=iidx, reproj_err=err)
    assert not _diff(out, want), _diff(out, want)
    assert not _diff(plain, want, OLD_KEYS) and sorted(plain) == sorted(OLD_KEYS)
    assert int(out["ok"].sum()) > 0 and _canary_untouched(full)


def test_off_means_off(call_paths):
    """A plain estimate and a plain pnp_ransac after report calls return the bytes they returned before them."""
    from gisnav_amd.engine import PoseEngine
    sd, pairs, _, _, _, _ = call_paths
    e = PoseEngine(0, max_batch=4, max_kpts=256, precision="f32", state_dict=sd)      # a context that never saw a report call
    inp = e.stage_inputs(pairs)
    scenes = S.one_call_scenes()[3:6]
    obj, img, n = _stage(e, scenes, 256)

    def run():
        est = e.estimate(inp, K_MATRIX, covariance=True)
        pnp = e.pnp_ransac(obj, img, n, S.K, covariance=True)
        torch.cuda.synchronize()
        return [est[k].cpu().numpy().tobytes() for k in sorted(est)] + [x.cpu().numpy().tobytes() for x in pnp]
    before = run()
    e.estimate(inp, K_MATRIX, report=True)
    e.estimate(inp, K_MATRIX, report=True, covariance=True)
    e.pnp_ransac(obj, img, n, S.K, report=True)
    e.vo_estimate(inp, K_MATRIX, ratio=0.9, min_matches=15, report=True)
    after = run()
    del e
    assert before == after
    assert sorted(PoseEngine.alloc_outputs.__defaults__) == [False, False]             # the default is off


# ------------------------------------------------------------------------------------------------------------------ 7
def test_compute_pose_returns_inliers_like_cv2(eng):
    import types
    from gisnav_amd.pose import compute_pose
    o, u = S.one_call_scenes()[4]
    info = types.SimpleNamespace(k=S.K.reshape(9))
    dem = np.zeros((480, 640), np.uint8)
    z = np.floor(o[:, 2]).astype(np.uint8)
    dem[np.floor(o[:, 1]).astype(int), np.floor(o[:, 0]).astype(int)] = z                 # the DEM cells under the reference keypoints
    assert np.array_equal(dem[np.floor(o[:, 1]).astype(int), np.floor(o[:, 0]).astype(int)], o[:, 2])   # (no two keypoints share a cell with two heights)
    plain = compute_pose(info, u, o[:, :2], dem, engine=eng)
    R, t, inl, err = compute_pose(info, u, o[:, :2], dem, engine=eng, return_inliers=True, return_residuals=True)
    want = pr.solve_pnp_ransac(o, u, S.K)[3]
    assert len(plain) == 2 and np.array_equal(plain[0], R) and np.array_equal(plain[1], t)
    assert inl.dtype == np.int32 and inl.shape == (len(want), 1) and np.array_equal(inl[:, 0], want)
    assert err.dtype == np.float32 and err.shape == (len(o),) and (err[inl[:, 0]] < 1e-3).all() and (np.delete(err, inl[:, 0]) > 30).all()
    Rc, tc, cov, inl2 = compute_pose(info, u, o[:, :2], dem, engine=eng, return_covariance=True, return_inliers=True)
    assert np.array_equal(Rc, R) and cov.shape == (6, 6) and np.array_equal(inl2, inl)


def test_pose_node_keeps_returning_r_t_and_stores_the_report(state_dict_np):
    from gisnav_amd import wire
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.pose_node import PoseNode
    p = make_pair(86, n_q=300, n_r=280)
    extractor = lambda r: (p.kp_r, p.desc_r, p.size_r, p.angle_r)  # noqa: E731
    cam = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    msg = wire.OrthoStereoImage(query_sift=wire.pack_keypoints(p.kp_q, p.size_q, p.angle_q, p.desc_q), reference=wire.ImageMsg(p.ref, wire.Stamp(7, 0)),
                                dem=wire.ImageMsg(p.dem, wire.Stamp(7, 0)))
    node = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32", report=True, covariance=True)
    plain_node = PoseNode(state_dict_np, extractor, max_kpts=512, precision="f32")
    assert node.last_report is None
    r, r0 = node.estimate(cam, msg), plain_node.estimate(cam, msg)
    eng = PoseEngine(0, max_batch=1, max_kpts=512, precision="f32", state_dict=state_dict_np)
    want = {k: v.cpu().numpy() for k, v in eng.estimate(eng.stage_inputs([p]), K_MATRIX, report=True, covariance=True).items()}
    assert r is not None and len(r) == 2 and np.array_equal(r[0], r0[0]) and np.array_equal(r[1], r0[1]) and np.array_equal(r[0], want["R"][0])
    assert plain_node.last_report is None and np.array_equal(node.last_covariance, want["cov"][0])
    rep, nm, ni = node.last_report, int(want["n_match"][0]), int(want["n_inliers"][0])
    assert sorted(rep) == ["inliers", "mkp_qry", "mkp_ref", "reproj_err", "score"]
    assert np.array_equal(rep["mkp_qry"], p.kp_q.astype(np.float32)[want["idx"][0, :nm, 0]])
    assert np.array_equal(rep["mkp_ref"], p.kp_r.astype(np.float32)[want["idx"][0, :nm, 1]])
    # (the node feeds the matcher wire records at the padded size this pair needs, the engine call above padded arrays: the same matches, scores
    # that may differ in their last bits -- the score is checked against the node's own device block, its bytes through the call paths above)
    assert np.array_equal(rep["score"], node._out["score"][0, :nm].cpu().numpy()) and np.abs(rep["score"] - want["score"][0, :nm]).max() < 1e-5
    assert np.array_equal(rep["reproj_err"], want["reproj_err"][0, :nm])
    assert rep["inliers"].shape == (ni, 1) and rep["inliers"].dtype == np.int32 and np.array_equal(rep["inliers"][:, 0], want["inlier_idx"][0, :ni])
    empty = wire.OrthoStereoImage(query_sift=b"", reference=msg.reference, dem=msg.dem)
    assert node.estimate(cam, empty) is None and node.last_report is None              # no pose: no stale report


def test_twist_pose_returns_inliers_of_its_ratio_test_survivors():
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.vo import twist_pose
    e = PoseEngine(0, max_batch=1, max_kpts=512, precision="f32")
    p = make_pair(3, n_q=400, n_r=400)
    plain = twist_pose(e, K_MATRIX, p.kp_q, p.desc_q, p.kp_r, p.desc_r)
    R, t, inl = twist_pose(e, K_MATRIX, p.kp_q, p.desc_q, p.kp_r, p.desc_r, return_inliers=True)
    assert len(plain) == 2 and np.array_equal(plain[0], R) and np.array_equal(plain[1], t)
    # the staged path on the same inputs: vo_match -> gather -> pnp_ransac(report=True)
    d = e.device
    k4 = lambda kp: torch.from_numpy(np.concatenate([kp, np.zeros_like(kp)], 1)[None].astype(np.float32)).to(d)  # noqa: E731
    n = torch.tensor([400], dtype=torch.int32, device=d)
    dq, dr = torch.from_numpy(p.desc_q[None].astype(np.float32)).to(d), torch.from_numpy(p.desc_r[None].astype(np.float32)).to(d)
    idx, _, n_good = e.vo_match(dq, n, dr, n, ratio=0.7)
    mkp, obj = e.gather_points(k4(p.kp_q), k4(p.kp_r), idx, n_good, None)
    res = e.pnp_ransac(obj, mkp, n_good, K_MATRIX, min_pts=30, report=True)
    k = int(res[2][0])
    assert inl.dtype == np.int32 and inl.shape == (k, 1) and 30 <= k <= int(n_good[0])
    assert np.array_equal(inl[:, 0], res[5][0, :k].cpu().numpy()) and np.array_equal(R, res[0][0].cpu().numpy())
    assert twist_pose(e, K_MATRIX, p.kp_q[:20], p.desc_q[:20], p.kp_r, p.desc_r, return_inliers=True) is None
    del e


def test_loftr_pose_returns_inliers_single_and_batched():
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.loftr import LoFTR, loftr_pose, loftr_pose_batch
    from oracle import loftr as lf
    h, w = 128, 160
    pair = lf.synthetic_pair(1, h, w)
    dem = (10 + 8 * np.sin(np.arange(h)[:, None] / 30.0) * np.cos(np.arange(w)[None, :] / 45.0)).astype(np.uint8)
    m = LoFTR(state_dict=lf.synthetic_state_dict(0)).to("cuda:0").eval()
    e = PoseEngine(0, max_batch=2, max_kpts=1024, precision="f32")
    plain = loftr_pose(m, e, pair[0].cuda(), pair[1].cuda(), dem, K_MATRIX)
    got = loftr_pose(m, e, pair[0].cuda(), pair[1].cuda(), dem, K_MATRIX, return_inliers=True)
    cov = loftr_pose(m, e, pair[0].cuda(), pair[1].cuda(), dem, K_MATRIX, return_inliers=True, return_covariance=True)
    assert plain is not None and len(plain) == 3 and len(got) == 4 and len(cov) == 5
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and got[2] == plain[2]
    inl = got[3]
    assert inl.dtype == np.int32 and inl.ndim == 2 and inl.shape[1] == 1 and 5 <= len(inl) <= got[2]
    assert (np.diff(inl[:, 0]) > 0).all() and inl.min() >= 0 and inl.max() < got[2] and np.array_equal(cov[4], inl)
    f, t = torch.stack([pair[0], pair[0]]).cuda(), torch.stack([pair[1], pair[1]]).cuda()
    both = loftr_pose_batch(m, e, f, t, [dem, dem], K_MATRIX, return_inliers=True)
    assert len(both) == 2
    for b in both:
        assert len(b) == 4 and np.array_equal(b[0], got[0]) and np.array_equal(b[3], inl) and b[3].dtype == np.int32
    del e, m

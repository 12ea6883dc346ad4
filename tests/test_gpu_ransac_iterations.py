"""iterations_count above 16 in the PnP stage: the round path of gn_pnp_ransac(_cov), gn_set_ransac / gn_get_ransac / gn_ransac_last_counts
(DESIGN.md "RANSAC beyond 16 hypotheses").  The expected values come from tests/golden/pnp_ransac_iters.npz
(tests/golden/make_ransac_iters_golden.py: the repo's restatements of cv2.solvePnPRansac run on the CPU), so no oracle runs here.

  1. parity with the restatement for every fixture row, the counts ROUND - 1, ROUND, ROUND + 1 and 2 ROUND + 1 included; 17 and 64 are accepted;
  2. counts 10 and 16 sent through the round path (developer knob 49) give the bits of the two classic launches;
  3. the early stop is honoured and bounded: 300 and 4096 requested give the same bits, at most one round more than needed is evaluated;
  4. pairs of one call do not see each other;
  5. through gn_estimate_cov, gn_set_ransac and compute_pose;
  6. with lens distortion on;
  7. the covariance at count 300 against fp64;
  8. the payoff: which of eight 50 %-outlier scenes are solved at 10, 100 and 300;
  9. the argument range.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

from gisnav_amd import _lib
from gisnav_amd.synthetic import K_MATRIX, make_pair
from oracle import pnp_ransac as pr

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_ransac_iters.npz"))
ROUND = int(G["round"])
K = G["K"]
PINHOLE = ("A", "B", "C", "D", "E", "clean") + tuple(f"P{i}" for i in range(8))
STRIDE = 384                                                            # scene B has 300 points
KNOB_ROUNDS = 49


def scene(name):
    return G[f"{name}_obj"], G[f"{name}_img"]


def row(name, count):
    i = int(np.nonzero(G[f"{name}_counts"] == count)[0][0])
    return dict(ok=int(G[f"{name}_ok"][i]), ninl=int(G[f"{name}_ninl"][i]), R=G[f"{name}_R"][i], t=G[f"{name}_t"][i],
                niters=int(G[f"{name}_niters"][i]), inl=np.nonzero(G[f"{name}_inl"][i])[0])


@pytest.fixture(scope="module")
def eng():
    from gisnav_amd.engine import PoseEngine
    e = PoseEngine(0, max_batch=16, max_kpts=STRIDE)
    yield e
    del e


def _stage(eng, scenes, stride=STRIDE):
    B = len(scenes)
    obj, img, n = np.zeros((B, stride, 3), np.float32), np.zeros((B, stride, 2), np.float32), np.zeros(B, np.int32)
    for b, (o, u) in enumerate(scenes):
        obj[b, :len(o)], img[b, :len(o)], n[b] = o, u, len(o)
    d = eng.device
    return torch.from_numpy(obj).to(d), torch.from_numpy(img).to(d), torch.from_numpy(n).to(d)


def _solve(eng, scenes, count, covariance=False, min_pts=5, Kmat=None):
    obj, img, n = _stage(eng, scenes)
    res = eng.pnp_ransac(obj, img, n, K if Kmat is None else Kmat, iterations=count, min_pts=min_pts, covariance=covariance)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in res]


def _bits(res):
    return [x.tobytes() for x in res]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("count", [17, 64])
def test_counts_above_16_are_accepted(eng, count):
    """gn_pnp_ransac itself, not the Python wrapper: no GN_ERR_ARG for a count past the old cap."""
    obj, img, n = _stage(eng, [scene("B")])
    d = eng.device
    R, t = torch.empty((1, 9), dtype=torch.float64, device=d), torch.empty((1, 3), dtype=torch.float64, device=d)
    n_inl, ok = torch.empty(1, dtype=torch.int32, device=d), torch.empty(1, dtype=torch.uint8, device=d)
    K9 = np.ascontiguousarray(K.reshape(9))
    rc = eng.lib.gn_pnp_ransac(eng.ctx, 1, obj.data_ptr(), img.data_ptr(), n.data_ptr(), STRIDE, K9.ctypes.data_as(_lib.c_f64p), count, 8.0, 0.99, 5,
                               R.data_ptr(), t.data_ptr(), n_inl.data_ptr(), ok.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.gn_last_error(eng.ctx)
    assert int(ok[0]) == 1


@pytest.fixture(scope="module")
def by_count(eng):
    """{count: {scene name: (R, t, n_inliers, ok, niters, evaluated)}}: one gn_pnp_ransac call per distinct count over every pinhole scene that
    lists it, each followed by gn_ransac_last_counts."""
    counts = sorted({int(c) for name in PINHOLE for c in G[f"{name}_counts"]})
    out = {}
    for c in counts:
        names = [name for name in PINHOLE if c in G[f"{name}_counts"]]
        R, t, n_inl, ok = _solve(eng, [scene(name) for name in names], c)
        niters, evaluated = eng.ransac_last_counts(len(names))
        out[c] = {name: (R[b], t[b].reshape(3), int(n_inl[b]), int(ok[b]), int(niters[b]), int(evaluated[b])) for b, name in enumerate(names)}
    return out


def _compare(label, got, want):
    """ok and n_inliers always; the pose within the suite's 1e-8 where the winner has >= 15 inliers (a 6 to 8 point winner's refinement is
    ill-conditioned: its difference is reported, not asserted)."""
    R, t, n_inl, ok = got[:4]
    assert ok == want["ok"] and n_inl == want["ninl"], (label, ok, n_inl, want["ok"], want["ninl"])
    if not ok:
        assert np.array_equal(R, np.eye(3)) and not t.any(), label
        return
    dR = np.linalg.norm(R - want["R"])
    dt = np.linalg.norm(t - want["t"]) / np.linalg.norm(want["t"])
    print(f"{label}: {n_inl} inliers, dR {dR:.2e} dt {dt:.2e}" + ("" if n_inl >= 15 else "   (reported only)"))
    if n_inl >= 15:
        assert dR < 1e-8 and dt < 1e-8, (label, dR, dt)


def test_parity_with_the_restatement_for_every_fixture_row(by_count):
    rows = 0
    for c, scenes in by_count.items():
        for name, got in scenes.items():
            want = row(name, c)
            _compare(f"{name} at {c}", got, want)
            assert got[4] == want["niters"], (name, c, got[4], want["niters"])      # the adapted count, classic and round path alike
            rows += 1
    assert rows == sum(len(G[f"{name}_counts"]) for name in PINHOLE)
    # the facts the rows were chosen for
    assert [row("A", c)["ninl"] for c in (10, 16, 17, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1, 300, 4096)] == [0, 0, 0] + [30] * 6
    assert [row("B", c)["ninl"] for c in (16, 17, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1, 300)] == [6, 7, 8, 8, 8, 8, 120]
    assert row("A", 4096)["niters"] == 145 and row("B", 1000)["niters"] == 447 and row("clean", 4096)["niters"] < ROUND


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def both_paths(eng):
    """Counts 10 and 16 with covariance on A, B, D, E and the two pnp_outliers fixtures: classic, then the same calls with knob 49 set."""
    here = os.path.dirname(os.path.abspath(__file__))
    scenes = [scene(n) for n in ("A", "B", "D", "E")]
    for f in ("pnp_outliers_dem", "pnp_outliers_flat"):
        g = np.load(os.path.join(here, "golden", f + ".npz"))
        scenes.append((g["obj"], g["img"]))
    res = {}
    for knob in (0, 1):
        assert eng.lib.gn_debug_set_variant(eng.ctx, KNOB_ROUNDS, knob) == 0
        try:
            for c in (10, 16):
                res[knob, c] = _solve(eng, scenes, c, covariance=True)
                res[knob, c].extend(eng.ransac_last_counts(len(scenes)))
        finally:
            assert eng.lib.gn_debug_set_variant(eng.ctx, KNOB_ROUNDS, 0) == 0
    return res


@pytest.mark.parametrize("count", [10, 16])
def test_same_bits_through_both_paths(both_paths, count):
    classic, rounds = both_paths[0, count], both_paths[1, count]
    names = ("R", "t", "n_inliers", "ok", "cov_rt", "sigma_hat", "cov_ok", "niters", "evaluated")
    assert int(classic[3].sum()) >= 3                                   # (poses to compare: D and the two 20 %-outlier fixtures at the least)
    diff = [k for k, a, b in zip(names, classic, rounds) if a.tobytes() != b.tobytes()]
    assert not diff, diff


# ------------------------------------------------------------------------------------------------------------------ 3
def test_early_stop_is_honoured_and_bounded(eng, by_count):
    a300, a4096 = by_count[300]["A"], by_count[4096]["A"]
    assert all(np.array_equal(x, y) for x, y in zip(a300[:4], a4096[:4]))           # bitwise: hypotheses past 145 never count
    up = -(-145 // ROUND) * ROUND
    for got in (a300, a4096):
        assert got[4] == 145 and got[5] <= up, got[4:]
    clean = by_count[4096]["clean"]
    print(f"A: evaluated {a300[5]} of 300 and {a4096[5]} of 4096 requested; clean scene: niters {clean[4]}, evaluated {clean[5]}")
    assert clean[3] == 1 and clean[5] <= ROUND
    # no model: every requested hypothesis is evaluated and none is thrown away
    assert by_count[300]["C"][4:] == (300, 300)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_pairs_of_one_call_are_independent(eng):
    o, u = scene("clean")
    batch = [scene("A"), scene("B"), scene("C"), scene("E"), (o, u), (o[4:8], u[4:8]), (o[:5], u[:5]), (o[:9], u[:9])]      # (P3P solves points 4..7)
    min_pts = 4

    def run(scenes):
        obj, img, n = _stage(eng, scenes)
        n = n.clone()
        n[[i for i, s in enumerate(scenes) if len(s[0]) == 9]] = 3         # below min_pts (nine rows staged, three announced)
        res = eng.pnp_ransac(obj, img, n, K, iterations=300, min_pts=min_pts, covariance=True)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in res]

    together = run(batch)
    assert together[3].tolist() == [1, 1, 0, 1, 1, 1, 1, 0], together[3]
    assert together[2].tolist()[:5] == [30, 120, 0, 36, 200] and together[2].tolist()[5:] == [4, 5, 0]
    for b, s in enumerate(batch):
        alone = run([s])
        diff = [i for i, (x, y) in enumerate(zip(together, alone)) if x[b].tobytes() != y[0].tobytes()]
        assert not diff, (b, diff)


# ------------------------------------------------------------------------------------------------------------------ 5
KEYS = ("R", "t", "n_match", "n_inliers", "ok", "cov", "sigma", "cov_ok")


@pytest.fixture(scope="module")
def small():
    """4 synthetic pairs at 2 x 512 keypoints with half of the query keypoints moved somewhere else (their descriptors still match: gross outliers
    for the pose stage), on an exact-f32 context."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    e = PoseEngine(0, max_batch=4, max_kpts=512, precision="f32", state_dict=synthetic_state_dict(0))
    pairs = []
    for i in range(4):
        p = make_pair(7500 + i, n_q=512 - 9 * i, n_r=512 - 5 * i)
        rng = np.random.default_rng(50 + i)
        kp = p.kp_q.copy()
        bad = rng.permutation(len(kp))[: len(kp) // 2]
        kp[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))]).astype(kp.dtype)
        pairs.append(dataclasses.replace(p, kp_q=kp))
    inp = e.stage_inputs(pairs)
    yield e, inp
    del e


def _staged(e, inp, count):
    from gisnav_amd.engine import MIN_MATCHES
    idx, _, n_match = e.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = e.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
    R, t, n_inl, ok, cov, sigma, cov_ok = e.pnp_ransac(obj, mkp, n_match, K_MATRIX, iterations=count, min_pts=MIN_MATCHES, covariance=True)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in dict(R=R, t=t, n_match=n_match, n_inliers=n_inl, ok=ok, cov=cov, sigma=sigma, cov_ok=cov_ok).items()}


def _diff(got, want):
    return [k for k in KEYS if not torch.equal(got[k].reshape(want[k].shape), want[k])]


@pytest.mark.parametrize("substreams", [1, 2])
def test_estimate_cov_with_set_ransac_equals_the_staged_path_bitwise(small, substreams):
    e, inp = small
    want, want10 = _staged(e, inp, 100), _staged(e, inp, 10)
    print("inliers at 100:", want["n_inliers"].tolist(), "of", want["n_match"].tolist(), "matches; at 10:", want10["n_inliers"].tolist())
    assert int(want["ok"].sum()) >= 1
    assert _diff(want, want10)                                          # the count reaches the pose stage: 100 and 10 differ on these pairs
    out = e.alloc_outputs(4, covariance=True)
    try:
        e.set_ransac(100, 8.0, 0.99)
        assert e.ransac() == (100, 8.0, 0.99)
        e.set_substreams(substreams)
        e.estimate(inp, K_MATRIX, out=out, covariance=True)
        e.flush()
        torch.cuda.synchronize()
        niters, evaluated = e.ransac_last_counts(4)
    finally:
        e.flush()
        e.set_substreams(1)
        e.set_ransac()
    assert e.ransac() == (10, 8.0, 0.99)
    assert not _diff(out, want), _diff(out, want)
    print("niters", niters.tolist(), "evaluated", evaluated.tolist())
    assert np.all(evaluated <= -(-np.maximum(niters, 1) // ROUND) * ROUND) and np.all(niters <= 100)


def test_the_default_told_equals_never_told(small):
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    e, inp = small
    fresh = PoseEngine(0, max_batch=4, max_kpts=512, precision="f32", state_dict=synthetic_state_dict(0))      # never saw gn_set_ransac
    never = fresh.alloc_outputs(4, covariance=True)
    fresh.estimate(inp, K_MATRIX, out=never, covariance=True)
    torch.cuda.synchronize()
    del fresh
    told = e.alloc_outputs(4, covariance=True)
    e.set_ransac(100, 4.0, 0.9)
    e.set_ransac(10, 8.0, 0.99)
    e.estimate(inp, K_MATRIX, out=told, covariance=True)
    torch.cuda.synchronize()
    assert not _diff(told, never), _diff(told, never)


def test_compute_pose_takes_a_count_per_call_and_leaves_the_engine_alone(eng, by_count):
    from gisnav_amd import wire
    from gisnav_amd.pose import compute_pose
    o, u = scene("A")
    dem = np.zeros((480, 640), np.uint8)
    cell = np.floor(o[:, :2]).astype(int)
    dem[cell[:, 1], cell[:, 0]] = o[:, 2].astype(np.uint8)
    assert np.array_equal(dem[cell[:, 1], cell[:, 0]].astype(np.float32), o[:, 2])
    info = wire.CameraInfo(k=K.reshape(9), height=480, width=640)
    eng.set_ransac(12, 6.0, 0.95)
    try:
        assert compute_pose(info, u, o[:, :2], dem, engine=eng) is None                # the reference's 10: no model on scene A
        R, t = compute_pose(info, u, o[:, :2], dem, engine=eng, ransac_iterations=100)
        assert eng.ransac() == (12, 6.0, pytest.approx(0.95))
    finally:
        eng.set_ransac()
    got = _solve(eng, [(o, u)], 100)
    assert np.array_equal(R, got[0][0]) and np.array_equal(t, got[1][0])
    assert np.linalg.norm(R - row("A", 300)["R"]) < 1e-8                                 # (the winner of 100 is the winner of 145)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_with_distortion_on(eng):
    o, u = scene("dist")
    eng.set_distortion(G["dist_d"])
    try:
        got = {c: _solve(eng, [(o, u)], c, Kmat=G["dist_K"]) for c in (10, 100)}
    finally:
        eng.set_distortion(None)
    for c, (R, t, n_inl, ok) in got.items():
        _compare(f"distorted scene at {c}", (R[0], t[0].reshape(3), int(n_inl[0]), int(ok[0])), row("dist", c))
    assert row("dist", 100)["ninl"] >= 15


# ------------------------------------------------------------------------------------------------------------------ 7
def test_covariance_at_300_against_fp64(eng):
    """cov_rt = s^2 (J^T J)^-1 from oracle.pnp_ransac.project_points at the GPU's pose over the restatement's inlier set, at the bounds of
    tests/test_gpu_pose_covariance.py: scaled difference <= 1e-9, sigma_hat 1e-10 relative."""
    o, u = scene("A")
    R, t, n_inl, ok, cov, sigma, cov_ok = _solve(eng, [(o, u)], 300, covariance=True)
    want = row("A", 300)
    assert ok[0] == 1 and cov_ok[0] == 1 and n_inl[0] == len(want["inl"]) == 30
    inl = want["inl"]
    proj, J = pr.project_points(o[inl].astype(np.float64), pr.rodrigues_mat2vec(R[0]), t[0].reshape(3), K, jac=True)
    e = (proj - u[inl].astype(np.float64)).reshape(-1)
    s2 = float(e @ e) / (2 * len(inl) - 6)
    w = s2 * np.linalg.inv(J.T @ J)
    d = np.sqrt(np.diag(w))
    dc, ds = float((np.abs(cov[0] - w) / np.outer(d, d)).max()), abs(sigma[0] - np.sqrt(s2)) / np.sqrt(s2)
    print(f"scene A at 300: scaled covariance difference {dc:.3e}, sigma_hat {sigma[0]:.4f} px, relative difference {ds:.3e}")
    assert np.array_equal(cov[0], cov[0].T)
    assert dc <= 1e-9 and ds <= 1e-10


# ------------------------------------------------------------------------------------------------------------------ 8
def test_the_payoff(by_count):
    solved = {c: [i for i in range(8) if by_count[c][f"P{i}"][3] == 1] for c in (10, 100, 300)}
    print("solved of the eight 50 %-outlier scenes:", solved)
    assert solved == {c: [i for i in range(8) if row(f"P{i}", c)["ok"]] for c in (10, 100, 300)}
    assert solved[10] == [1, 3, 4, 5] and solved[100] == [0, 1, 3, 4, 5, 6, 7] and solved[300] == list(range(8))


# ------------------------------------------------------------------------------------------------------------------ 9
def test_argument_range(eng):
    obj, img, n = _stage(eng, [scene("A")])
    err_arg = eng.lib.gn_set_distortion(None, None, 0)                  # GN_ERR_ARG
    for bad in (0, -1, 4097):
        with pytest.raises(_lib.GnError, match="1..4096"):
            eng.pnp_ransac(obj, img, n, K, iterations=bad)
        assert eng.lib.gn_set_ransac(eng.ctx, bad, 8.0, 0.99) == err_arg
        assert b"4096" in eng.lib.gn_last_error(eng.ctx)
        assert eng.ransac() == (10, 8.0, 0.99)                          # a refused call leaves the state as it was
    assert eng.lib.gn_set_ransac(eng.ctx, 10, 0.0, 0.99) == err_arg and eng.lib.gn_set_ransac(eng.ctx, 10, 8.0, 1.0) == err_arg
    R, t, n_inl, ok = eng.pnp_ransac(obj, img, n, K, iterations=4096)
    torch.cuda.synchronize()
    assert int(ok[0]) == row("A", 4096)["ok"] == 1 and int(n_inl[0]) == row("A", 4096)["ninl"]
    eng.set_ransac(4096)
    assert eng.ransac()[0] == 4096
    eng.set_ransac()

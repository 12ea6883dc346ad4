"""Host tests (no GPU) of tests/match_head_ref.py, the fp64 reference tests/test_gpu_match_head.py compares the match head with:

  * the reference is kornia's operation: pinned to oracle.lightglue_sift.sigmoid_log_double_softmax + filter_matches on small matrices, its rule to
    the sorted-matrix statement of the certificate in tests/test_certificate.py, its critical values to its rule;
  * the GPU cases' preconditions hold in fp64 alone: the grid every case is meant to reach, the share of rows / columns whose arg-max cannot be
    compared, the tie positions of every kind with a deciding entry behind them, and the (a) / (b) / (c) pattern and the margin of every entry of the
    eps / threshold table.
"""
import math

import numpy as np
import pytest
import torch

import match_head_ref as R
from oracle import lightglue_sift as lg


def _small(seed, n0, n1, scale):
    rng = np.random.default_rng(seed)
    md = (rng.normal(0.0, 0.5, (2, max(n0, n1), 256)) * scale).astype(np.float32)
    z = rng.normal(2.0, 3.0, (2, max(n0, n1)))
    return md, z


@pytest.mark.parametrize("n0,n1,scale,th", [(2, 2, 1.0, 0.0), (5, 7, 1.0, 0.1), (33, 20, 1.5, 0.2), (64, 97, 0.7, 0.5), (40, 40, 2.0, 0.0)])
def test_reference_is_the_oracles_double_softmax_and_filter(n0, n1, scale, th):
    md, z = _small(n0 * 100 + n1, n0, n1, scale)
    ls = R.logsigmoid(z)
    S = R.similarity(md[0, :n0], md[1, :n1], "f32", np.float64)
    r = R.evaluate(S, ls[0, :n0], ls[1, :n1], np.float64)
    scores = lg.sigmoid_log_double_softmax(torch.from_numpy(S)[None], torch.from_numpy(z[0, :n0])[None, :, None], torch.from_numpy(z[1, :n1])[None, :, None])
    P = scores[0, :-1, :-1].numpy()
    assert np.abs(P - r["P"]).max() < 1e-12
    assert np.abs(torch.logsumexp(torch.from_numpy(S), 1).numpy() - r["rlse"]).max() < 1e-12
    assert np.abs(torch.logsumexp(torch.from_numpy(S), 0).numpy() - r["clse"]).max() < 1e-12
    m0, m1, ms0, _ = lg.filter_matches(scores, th)
    want = [(i, int(j)) for i, j in enumerate(m0[0].tolist()) if j >= 0]
    got = R.filter_matches(r["max0"], r["m0"], r["m1"], th)
    assert got == want
    assert np.allclose([math.exp(r["max0"][i]) for i, _ in got], [float(ms0[0, i]) for i, _ in got], rtol=1e-12)
    # best / runner-up / arg-max against a full sort
    srt = -np.sort(-r["P"], axis=1)
    assert np.array_equal(srt[:, 0], r["max0"]) and np.array_equal(srt[:, 1], r["max0b"]) and np.array_equal(r["P"].argmax(1), r["m0"])
    srt = -np.sort(-r["P"].T, axis=1)
    assert np.array_equal(srt[:, 0], r["colbest"]) and np.array_equal(srt[:, 1], r["col2"]) and np.array_equal(r["P"].argmax(0), r["m1"])


def test_runner_up_counts_multiplicity_and_argmax_takes_the_lowest_index():
    P = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, -1.0, 0.0, 0.0], [5.0, 4.0, 3.0, 2.0]])
    best, second, arg = R.top2(P, 1)
    assert best.tolist() == [3.0, 0.0, 5.0] and second.tolist() == [3.0, 0.0, 4.0] and arg.tolist() == [1, 0, 0]
    best, second, arg = R.top2(P, 0)
    assert best.tolist() == [5.0, 4.0, 3.0, 2.0] and second.tolist() == [1.0, 3.0, 3.0, 2.0] and arg.tolist() == [2, 2, 0, 0]


def _sorted_certificate(P, th, eps):
    """tests/test_certificate.py's statement (True = certified)."""
    L = math.log(th) if th > 0 else -math.inf
    for M in (P, P.T):
        top = -np.sort(-M, axis=1)[:, :2]
        if np.any((top[:, 0] >= L - eps) & ~(top[:, 0] - top[:, 1] > 2 * eps)):
            return False
    return not np.any(np.abs(P.max(1) - L) <= eps)


def test_rule_is_the_certificate_and_its_verdicts_are_steps_at_the_critical_values():
    rng = np.random.default_rng(5)
    for trial in range(100):
        n0, n1 = int(rng.integers(2, 30)), int(rng.integers(2, 30))
        md, z = _small(9000 + trial, n0, n1, float(rng.uniform(0.5, 2.0)))
        ls = R.logsigmoid(z)
        r = R.evaluate(R.similarity(md[0, :n0], md[1, :n1], "f32", np.float64), ls[0, :n0], ls[1, :n1], np.float64)
        th = float(np.float32(rng.choice([0.0, 0.05, 0.2, 0.5])))
        v = (r["max0"], r["max0b"], r["colbest"], r["col2"])
        eps = float(np.float32(rng.uniform(1e-6, 0.5)))
        assert (not any(R.rule(*v, th, eps))) == _sorted_certificate(r["P"], th, eps), trial
        for k, crit in enumerate(R.critical_eps(*v, th)):
            if math.isfinite(crit):
                assert R.rule(*v, th, crit * (1 + 1e-9) + 1e-12)[k] and (crit <= 1e-12 or not R.rule(*v, th, crit * (1 - 1e-9) - 1e-12)[k]), (trial, k)
            else:
                assert not R.rule(*v, th, 1e30)[k] and R.rule(*v, th, math.inf)[k]
        assert R.rule(*v, th, eps, np.float32) == R.rule(*(np.float32(x) for x in v), th, eps)      # f32 arithmetic on f32 values decides as fp64 does, away from ties


def test_split_model_is_the_f16x2_kernels_operation():
    x = np.random.default_rng(1).normal(0.0, 0.5, (64, 256)).astype(np.float32)
    h, m = R.split_hm16(x)
    assert h.dtype == np.float16 and m.dtype == np.float16
    assert np.abs(x.astype(np.float64) - h.astype(np.float64) - m.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(x).max()
    a, b = x[:32], x[32:]
    (ah, am), (bh, bm) = R.split_hm16(a), R.split_hm16(b)
    f = np.float64
    three = ah.astype(f) @ bh.astype(f).T + ah.astype(f) @ bm.astype(f).T + am.astype(f) @ bh.astype(f).T
    assert np.abs(R.similarity(a, b, "f16x2", np.float64) - three).max() < 1e-13
    # the dropped A_m B_m^T term and the residual e: far below an f32 evaluation's own error
    assert np.abs(three - a.astype(f) @ b.astype(f).T).max() < 5e-6


def test_padding_does_not_touch_the_valid_part():
    g, z = R.case_inputs("np256", "garbage"), R.case_inputs("np256", "zero")
    n0, n1 = g["nvalid"][0]
    for k, w in (("md", 256), ("ls", 1)):
        for side, n in ((0, n0), (1, n1)):
            assert np.array_equal(g[k][0, side, :n], z[k][0, side, :n])
            assert np.all(z[k][0, side, n:] == 0) and np.all(np.isfinite(g[k][0, side, n:])) and np.abs(g[k][0, side, n:]).max() <= 1e4
            assert np.abs(g[k][0, side, n:]).max() > 1e3


def test_cases_reach_the_grids_they_are_meant_to():
    for case, (B, npad, nv, S, _) in R.CASES.items():
        assert R.head_grid(B, npad) == (npad // 128, S), case
        assert len(nv) == B and all(1 <= a <= npad and 1 <= b <= npad for a, b in nv)
    assert not R.renumbered(1, 384) and R.head_grid(1, 384)[0] * 4 == 12            # 12 workgroups: the XCD renumbering is off
    assert R.renumbered(1, 2176) and R.head_grid(1, 2176)[0] == 17 and -(-2100 // 128) == 17      # 17 row blocks hold valid rows: a second trip of the 16-partial merge
    assert -(-130 // 128) == 2 and 130 - 128 == 2                                     # np256: the second row block holds two valid rows
    assert [R.column_place(0, 70, 4)[0], R.column_place(69, 70, 4)[0]] == [1, 3]      # ... and its two column tiles fall to splits 1 and 3 (0 and 2 are empty)
    nv64 = R.CASES["b64_np512"][2]
    assert sum(1 for a, b in nv64 if a == 512 and b == 512) >= 2 and len({a for a, _ in nv64}) > 32
    assert sum(1 for a, b in R.RAGGED8 if a < 2 or b < 2) == 2


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_fp64_alone_keeps_the_excluded_rows_and_columns_under_the_cap(case, fmt):
    """Even at the largest distance the GPU test allows (d = the budget, 4 x e32), at most 1 % of the rows and of the columns -- and at most 2 per 512 -- have
    a top-2 gap within 2 d."""
    ref = R.case_ref(case, fmt)
    er, ec = ref.excluded(ref.budget)
    print(f"{case} {fmt}: e32 {ref.e32:.3g}, budget {ref.budget:.3g}, split model vs unsplit fp64 {ref.split_dist:.3g}, excluded at the budget {er} of {ref.rows} rows, {ec} of {ref.cols} columns")
    assert 1e-7 < ref.e32 < 5e-5      # f32 rounding of scores of magnitude 1 .. 16: nothing below an ulp, nothing near 1e-4
    assert er <= 0.01 * ref.rows and ec <= 0.01 * ref.cols
    assert er <= 2 * math.ceil(ref.rows / 512) and ec <= 2 * math.ceil(ref.cols / 512)
    for p in ref.pairs:
        if p.decides:
            assert all(np.all(np.isfinite(p.r[k])) for k in R.VALUES)
            assert -20.0 < p.r["max0"].min() and p.r["max0"].max() <= 0.0


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_eps_table_has_every_kind_with_its_pattern_and_margin(fmt):
    table, margin = R.eps_table(fmt)
    ref = R.case_ref(R.FLAG_CASE, fmt)
    dec = [b for b, p in enumerate(ref.pairs) if p.decides]
    assert margin == R.MARGIN * ref.budget and len(dec) == 6
    kinds = {e["kind"]: e for e in table}
    assert set(kinds) == {"none", "only a", "only b", "only c", "mixed", "all", "eps 0"}
    for e in table:
        built_on = dec if e["pair"] is None else [e["pair"]]
        assert all(R.pair_margin(ref, e, b) >= margin for b in built_on), (e["kind"], [R.pair_margin(ref, e, b) for b in built_on])
        assert all(e["expect"][b] == (False, False, False) for b in range(8) if b not in dec)      # a pair with a side below 2 never flags
        assert e["eps"] >= 0.0 and e["th"] >= 0.0 and e["swap"] in (False, True)
    assert all(kinds["none"]["expect"][b] == (False, False, False) for b in dec) and 0.0 < kinds["none"]["eps"] < math.inf
    a, b = kinds["only a"], kinds["only b"]
    assert a["pair"] == b["pair"] and a["eps"] == b["eps"] and a["th"] == b["th"] == 0.0 and b["swap"] and not a["swap"]
    assert a["expect"][a["pair"]] == (True, False, False) and b["expect"][b["pair"]] == (False, True, False)
    ea, eb, _ = ref.pairs[a["pair"]].critical(0.0)
    assert ea < a["eps"] < eb      # between half the smallest row gap and half the smallest column gap
    c = kinds["only c"]
    assert c["expect"][c["pair"]] == (False, False, True) and c["th"] > 0.0
    p = ref.pairs[c["pair"]]
    assert np.abs(p.r["max0"] - math.log(c["th"])).min() < 1e-6      # th = exp(best_i) of one of its rows
    flagged = [any(kinds["mixed"]["expect"][b]) for b in dec]
    assert any(flagged) and not all(flagged)
    assert all(kinds["all"]["expect"][b] == (True, True, True) for b in dec) and kinds["all"]["eps"] == math.inf
    assert all(kinds["eps 0"]["expect"][b] == (False, False, False) for b in dec) and kinds["eps 0"]["eps"] == 0.0


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("case", R.TIE_CASES)
def test_tie_positions_cover_the_kinds_and_decide_an_entry(case, fmt):
    B, npad, nv, S, _ = R.CASES[case]
    n0, n1 = nv[0]
    pos = R.tie_positions(case, fmt)
    want_c = [k for k in R.COL_KINDS if case == "np2176" or k != "different tiles"]            # np512: one tile per column split
    want_r = [k for k in R.ROW_KINDS if case == "np2176" or k != "row blocks 0 and 16"]        # np512: four row blocks
    assert list(pos["cols"]) == want_c and list(pos["rows"]) == want_r
    for kind, (p, q) in pos["cols"].items():
        assert p < q < n1 and R.col_kind(p, q, n1, S) == kind
    for kind, (p, q) in pos["rows"].items():
        assert p < q < n0 and R.row_kind(p, q) == kind
    assert len({x for v in pos["cols"].values() for x in v}) == 2 * len(want_c) and len({x for v in pos["rows"].values() for x in v}) == 2 * len(want_r)
    for side, key in ((1, "cols"), (0, "rows")):
        ref = R.tie_ref(case, fmt, side)
        groups = sorted(pos[key].values())
        hit = R.tied_entries(ref.pairs[0], groups, side, ref.budget)
        assert {p for _, p in hit} == {p for p, _ in groups}, (side, hit)      # every duplicated group decides at least one row / column, 2 x budget clear of the rest
        er, ec = ref.excluded(ref.budget)
        assert er <= 0.01 * ref.rows + len(hit) and ec <= 0.01 * ref.cols + len(hit)

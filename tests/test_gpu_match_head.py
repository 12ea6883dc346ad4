"""-m gpu tests of the match head (csrc/gn_match_head.hip) driven directly through gn_debug_match_head, against the fp64 reference of
tests/match_head_ref.py: the row AND column values, the arg-maxima, the returned list, ties, and the certificate's flags against its stated rule.

Every case runs on an "f32" context (k_head_fused<true, .>, compared with S = A . B^T in fp64) and on an "f16x2_bf16_attn" context
(k_head_fused<false, .>, compared with the split-fp16 product the kernel performs, in fp64).  The cases are the smallest at which the head's
partitioning changes (match_head_ref.CASES; the host test asserts the grid of each).  Per case:

  1. values   rowmax + rowlog, colmax + collog, max0, max0b, colbest, col2 over the valid rows / columns: the largest distance d from fp64 stays within
              4 x e32, e32 being the same distance of an f32 NumPy evaluation of the formula on the same operands (the factor the stage tests of the
              other kernels give an f32 stage: summation order over 64 lane partials, up to 8 column splits and 17 row blocks, v_exp_f32 / logf);
  2. decisions  m0 / m1 equal the fp64 arg-max wherever the fp64 gap exceeds 2 d; at most 1 % of the rows / columns fall below that;
  3. the list  is exactly what the GPU's own m0 / m1 / max0 imply, score = exp(max0), pairs with a side below 2 report nothing, and the list is the
              fp64 list for the pairs whose every gap exceeds 2 d;
  4. ties     exact duplicates at positions in the same lane half / tile / column split / row quarter / row block: lowest index, runner-up == best, flagged;
  5. flags    equal the rule evaluated in float32 on the GPU's own vectors, on an eps / threshold table whose every entry has its (a) / (b) / (c)
              pattern fixed by fp64 (the host test asserts pattern and margin);
  6. the five-pass form (developer knob 16 = 0) on what it keeps;
  7. a repeated call gives the same bits (the arrival counters return to zero), and so does zero instead of garbage padding.

Measured on an MI355X (d: largest distance from fp64 over the six values; excluded: rows / columns with an fp64 gap within 2 d; split: the f16x2 operand
model's distance from the unsplit fp64 product, on S):

  1 x 128, (128, 128)      f32    d 7.61e-06  e32 1.36e-05                 d / e32 0.56  excluded 0 of 128 rows, 0 of 128 columns   split --
  1 x 128, (128, 128)      f16x2  d 4.6e-06   e32 1.61e-05                 d / e32 0.29  excluded 0 of 128 rows, 0 of 128 columns   split 1.68e-06
  1 x 128, (2, 2)          f32    d 1.94e-06  e32 1.36e-05 (own 4.13e-07)  d / e32 0.14  excluded 0 of 2 rows, 0 of 2 columns   split --
  1 x 128, (2, 2)          f16x2  d 4.45e-07  e32 1.61e-05 (own 1.4e-06)   d / e32 0.03  excluded 0 of 2 rows, 0 of 2 columns   split 5.2e-07
  1 x 256, (130, 70)       f32    d 7.5e-06   e32 1.35e-05                 d / e32 0.56  excluded 0 of 130 rows, 0 of 70 columns   split --
  1 x 256, (130, 70)       f16x2  d 3.65e-06  e32 1.21e-05                 d / e32 0.30  excluded 0 of 130 rows, 0 of 70 columns   split 1.45e-06
  1 x 384, (300, 384)      f32    d 1.09e-05  e32 1.85e-05                 d / e32 0.59  excluded 0 of 300 rows, 0 of 384 columns   split --
  1 x 384, (300, 384)      f16x2  d 6.88e-06  e32 1.57e-05                 d / e32 0.44  excluded 0 of 300 rows, 0 of 384 columns   split 1.6e-06
  1 x 512, (512, 500)      f32    d 9.52e-06  e32 2.04e-05                 d / e32 0.47  excluded 0 of 512 rows, 0 of 500 columns   split --
  1 x 512, (512, 500)      f16x2  d 5.75e-06  e32 1.87e-05                 d / e32 0.31  excluded 0 of 512 rows, 0 of 500 columns   split 1.76e-06
  8 x 256, ragged          f32    d 1.13e-05  e32 1.87e-05                 d / e32 0.60  excluded 0 of 552 rows, 0 of 648 columns   split --
  8 x 256, ragged          f16x2  d 7.6e-06   e32 1.94e-05                 d / e32 0.39  excluded 0 of 552 rows, 0 of 648 columns   split 1.65e-06
  64 x 512, varied         f32    d 1.62e-05  e32 2.96e-05                 d / e32 0.55  excluded 0 of 18734 rows, 0 of 17734 columns   split --
  64 x 512, varied         f16x2  d 8.66e-06  e32 2.39e-05                 d / e32 0.36  excluded 0 of 18734 rows, 0 of 17734 columns   split 1.92e-06
  1 x 2176, (2100, 2176)   f32    d 1.25e-05  e32 2.94e-05                 d / e32 0.43  excluded 0 of 2100 rows, 0 of 2176 columns   split --
  1 x 2176, (2100, 2176)   f16x2  d 9.88e-06  e32 2.95e-05                 d / e32 0.33  excluded 0 of 2100 rows, 0 of 2176 columns   split 2.1e-06

  five-pass form (rowmax + rowlog, colmax + collog, max0):
  1 x 256, (130, 70)       f32    d 8.91e-06  e32 1.35e-05  d / e32 0.66
  1 x 256, (130, 70)       f16x2  d 5.04e-06  e32 1.21e-05  d / e32 0.42
  8 x 256, ragged          f32    d 1.29e-05  e32 1.87e-05  d / e32 0.69
  8 x 256, ragged          f16x2  d 6.53e-06  e32 1.94e-05  d / e32 0.34
  1 x 512, (512, 500)      f32    d 1.68e-05  e32 2.04e-05  d / e32 0.82
  1 x 512, (512, 500)      f16x2  d 8.04e-06  e32 1.87e-05  d / e32 0.43

  The (2, 2) run of the first case compares twelve numbers; an f32 evaluation's error on them (own: 4.1e-07 / 1.4e-06) is a draw, not a measure, so the
  case's e32 is taken over both of its runs.  Against its own figure the f32 run stands at d / e32 = 4.69 with d 1.94e-06, a quarter of the d of the 128 x 128 run next to it.
  Ties (np512, np2176; tied columns / tied rows): d 5.9e-06 .. 1.24e-05 within the same budgets; every duplicated group decided one to three entries,
  all resolved to the lowest index with runner-up == best, all pairs flagged at eps = 0.  Flag table (8 x 256): every entry's flags equal the rule on
  the GPU's vectors and the fp64 pattern in all eight pairs.  Nothing in gn_match_head.hip had to change.
"""
import functools
import math

import numpy as np
import pytest
import torch

import match_head_ref as R

pytestmark = pytest.mark.gpu

PRECISION = {"f32": "f32", "f16x2": "f16x2_bf16_attn"}
FLOATS = ("rowmax", "rowlog", "colmax", "collog", "max0", "max0b", "colbest", "col2")
FIVE_PASS_VALUES = ("rlse", "clse", "max0")      # the five-pass form keeps no runner-ups and no column scores
_engines = {}


def _engine(fmt, B, npad):
    """One context per (format, batch, padded size), no larger than the case needs; no weights (the head reads none)."""
    from gisnav_amd.engine import PoseEngine
    key = (fmt, B, npad)
    if key not in _engines:
        _engines[key] = PoseEngine(0, max_batch=B, max_kpts=npad, precision=PRECISION[fmt], filter_threshold=R.TH)
        assert _engines[key].kmax == npad
    return _engines[key]


def _run(fmt, inp, th=R.TH, eps=None, fused=True):
    """One gn_debug_match_head call; every output on the host.  eps: None = certificate off, else set_certify("flag", eps, eps)."""
    from gisnav_amd import _lib
    B, npad = inp["B"], inp["npad"]
    eng = _engine(fmt, B, npad)
    _lib.check(eng.ctx, eng.lib.gn_set_filter_threshold(eng.ctx, float(th)), "gn_set_filter_threshold")
    if eps is None:
        eng.set_certify("off")
    else:
        eng.set_certify("flag", eps=eps, eps_f32=eps)
    _lib.check(eng.ctx, eng.lib.gn_debug_set_variant(eng.ctx, 16, 1 if fused else 0), "gn_debug_set_variant")
    dev = eng.device
    try:
        idx, score, n_match = eng.debug_match_head(torch.from_numpy(inp["md"]).to(dev), torch.from_numpy(inp["ls"]).to(dev), torch.from_numpy(inp["nvalid"]).to(dev))
        torch.cuda.synchronize()
        out = {k: eng.debug_read(k, B * npad).reshape(B, npad).copy() for k in FLOATS}
        out.update({k: eng.debug_read(k, B * npad, np.int32).reshape(B, npad).copy() for k in ("m0", "m1")})
        out.update(idx=idx.cpu().numpy(), score=score.cpu().numpy(), n_match=n_match.cpu().numpy(), flags=None if eps is None else eng.uncertain(B).copy())
    finally:
        eng.lib.gn_debug_set_variant(eng.ctx, 16, 1)
    return out


def _pair_values(out, b, p):
    """The GPU's vectors of pair b over its valid rows / columns, under the reference's names."""
    n0, n1 = p.n0, p.n1
    f = np.float64
    return dict(rlse=out["rowmax"][b, :n0].astype(f) + out["rowlog"][b, :n0], clse=out["colmax"][b, :n1].astype(f) + out["collog"][b, :n1],
                max0=out["max0"][b, :n0], max0b=out["max0b"][b, :n0], colbest=out["colbest"][b, :n1], col2=out["col2"][b, :n1],
                m0=out["m0"][b, :n0], m1=out["m1"][b, :n1])


def _distance(out, ref, names=R.VALUES):
    """d: the largest absolute difference from fp64 over `names`, all pairs with a decision; everything compared must be finite."""
    d = 0.0
    for b, p in enumerate(ref.pairs):
        if not p.decides:
            continue
        g = _pair_values(out, b, p)
        for k in names:
            assert np.all(np.isfinite(g[k])), (b, k)
            d = max(d, float(np.abs(g[k].astype(np.float64) - p.r[k]).max()))
    return d


def _check_decisions(out, ref, d, skip=None):
    """Assertion 2.  skip: per pair (rows, columns) checked elsewhere (ties).  Returns the excluded (rows, columns)."""
    ex_r = ex_c = 0
    for b, p in enumerate(ref.pairs):
        if not p.decides:
            continue
        g = _pair_values(out, b, p)
        rows, cols = p.row_gap > 2 * d, p.col_gap > 2 * d
        ex_r += int((~rows).sum()); ex_c += int((~cols).sum())
        assert np.array_equal(g["m0"][rows], p.r["m0"][rows]), (b, np.nonzero(g["m0"] != p.r["m0"])[0][:8])
        assert np.array_equal(g["m1"][cols], p.r["m1"][cols]), (b, np.nonzero(g["m1"] != p.r["m1"])[0][:8])
    sr, sc = skip or (0, 0)
    assert ex_r - sr <= 0.01 * ref.rows and ex_c - sc <= 0.01 * ref.cols, (ex_r, ex_c, ref.rows, ref.cols)
    return ex_r, ex_c


def _check_list(out, ref, th, d, certified):
    """Assertion 3.  Returns the number of pairs whose list was also compared with fp64's."""
    compared = 0
    th32 = np.float32(th)
    for b, p in enumerate(ref.pairs):
        k = int(out["n_match"][b])
        if not p.decides:
            assert k == 0 and (not certified or out["flags"][b] == 0), b
            continue
        m0, m1, max0 = out["m0"][b, :p.n0], out["m1"][b, :p.n1], out["max0"][b, :p.n0]
        assert m0.min() >= 0 and m0.max() < p.n1 and m1.min() >= 0 and m1.max() < p.n0
        sc = np.exp(max0.astype(np.float32))
        mutual = m1[m0] == np.arange(p.n0)
        # expf on the device and NumPy's may differ in the last place: a row whose exp(max0) lies within 4 ulp of th may go either way (none does, as a rule)
        sure, may = mutual & (sc > th32 * np.float32(1 + 5e-7)), mutual & (sc > th32 * np.float32(1 - 5e-7))
        got = out["idx"][b, :k]
        rows = got[:, 0]
        assert np.all(np.diff(rows) > 0) and np.all(may[rows]) and set(np.nonzero(sure)[0]) <= set(rows.tolist()), b
        assert np.array_equal(got[:, 1], m0[rows]), b
        assert np.allclose(out["score"][b, :k], sc[rows], rtol=5e-7, atol=0.0), b
        if p.row_gap.min() > 2 * d and p.col_gap.min() > 2 * d and (th <= 0 or np.abs(p.r["max0"] - math.log(th)).min() > d):
            assert [tuple(x) for x in got.tolist()] == p.matches(th), b
            compared += 1
    return compared


def _check_flags(out, ref, th, eps):
    """Assertion 5, the exact half: the flags are the rule, evaluated in float32 on the GPU's own vectors.  Returns the per-pair (a, b, c)."""
    verdicts, variants = [], {-1: [], 0: [], 1: []}
    for b, p in enumerate(ref.pairs):
        if not p.decides:
            verdicts.append((False, False, False))
            for u in variants:
                variants[u].append(0)
            continue
        g = _pair_values(out, b, p)
        v = (g["max0"], g["max0b"], g["colbest"], g["col2"])
        verdicts.append(R.rule(*v, th, eps, np.float32))
        for u in variants:
            variants[u].append(int(any(R.rule(*v, th, eps, np.float32, ulps=u))))
    flags = out["flags"].tolist()
    assert flags == variants[0] or flags in (variants[-1], variants[1]), (flags, variants)      # (logf(th) on the device may round the other way)
    return verdicts


def _bits(out, ref):
    """Everything a call returns, over the valid rows / columns and list entries, as bytes."""
    parts = [out["n_match"].tobytes(), b"" if out["flags"] is None else out["flags"].tobytes()]
    for b, p in enumerate(ref.pairs):
        k = int(out["n_match"][b])
        parts += [out["idx"][b, :k].tobytes(), out["score"][b, :k].tobytes()]
        if p.decides:
            parts += [out[n][b, :(p.n0 if n in ("rowmax", "rowlog", "max0", "max0b", "m0") else p.n1)].tobytes() for n in FLOATS + ("m0", "m1")]
    return parts


MAIN_EPS = 1.0e-3      # the value runs carry a certificate too, so that every size has its flags compared with the rule


@functools.lru_cache(maxsize=None)
def _main(case, fmt):
    return _run(fmt, R.case_inputs(case), R.TH, MAIN_EPS)


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_values_decisions_list_and_flags_against_fp64(case, fmt):
    ref, out = R.case_ref(case, fmt), _main(case, fmt)
    d = _distance(out, ref)
    ex = ref.excluded(d)
    print(f"\n| {case} | {fmt} | d {d:.3g} | e32 {ref.e32:.3g} (the run's own {ref.own_e32:.3g}) | d / e32 {d / ref.e32:.2f} | excluded {ex[0]} of {ref.rows} rows, {ex[1]} of {ref.cols} columns | split {ref.split_dist:.3g} |")
    assert d <= ref.budget, (d, ref.e32)
    for b, p in enumerate(ref.pairs):
        if p.decides:
            g = _pair_values(out, b, p)
            assert np.all(g["max0b"] <= g["max0"]) and np.all(g["col2"] <= g["colbest"]), b
    assert _check_decisions(out, ref, d) == ex
    compared = _check_list(out, ref, R.TH, d, True)
    _check_flags(out, ref, R.TH, MAIN_EPS)
    print(f"  lists compared with fp64: {compared} of {sum(p.decides for p in ref.pairs)} pairs; matches {out['n_match'].tolist()[:8]}; flags {out['flags'].tolist()[:8]}")


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("case", list(R.CASES))
def test_a_repeated_call_gives_the_same_bits(case, fmt):
    ref, first = R.case_ref(case, fmt), _main(case, fmt)
    again = _run(fmt, R.case_inputs(case), R.TH, MAIN_EPS)
    assert _bits(again, ref) == _bits(first, ref)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_zero_padding_gives_the_same_bits_as_garbage_padding(fmt):
    case = "b8_np256"
    ref = R.case_ref(case, fmt)
    zero = _run(fmt, R.case_inputs(case, "zero"), R.TH, MAIN_EPS)
    assert _bits(zero, ref) == _bits(_main(case, fmt), ref)


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("side", [1, 0], ids=["tied_columns", "tied_rows"])
@pytest.mark.parametrize("case", R.TIE_CASES)
def test_ties_resolve_to_the_lowest_index_and_are_flagged(case, side, fmt):
    ref, inp = R.tie_ref(case, fmt, side), R.tie_inputs(case, fmt, side)
    groups = sorted(R.tie_positions(case, fmt)["cols" if side == 1 else "rows"].values())
    out = _run(fmt, inp, 0.0, 0.0)
    d = _distance(out, ref)
    assert d <= ref.budget, (d, ref.e32)
    p = ref.pairs[0]
    g = _pair_values(out, 0, p)
    entries = R.tied_entries(p, groups, side, d)
    assert {q for _, q in entries} == {q for q, _ in groups}, entries
    arg, best, second = (g["m0"], g["max0"], g["max0b"]) if side == 1 else (g["m1"], g["colbest"], g["col2"])
    for o, lowest in entries:
        assert arg[o] == lowest and second[o] == best[o], (o, lowest, int(arg[o]), float(best[o]), float(second[o]))
    _check_decisions(out, ref, d, skip=(len(entries), len(entries)))
    _check_list(out, ref, 0.0, d, True)
    _check_flags(out, ref, 0.0, 0.0)
    assert out["flags"][0] == 1      # a deciding tie is a gap of 0: flagged at every eps
    print(f"\n  {case} {fmt} side {side}: d {d:.3g} (e32 {ref.e32:.3g}), tied entries (row or column, lowest index) {entries}")
    if case == "np512":              # the five-pass form breaks ties the same way
        out5 = _run(fmt, inp, 0.0, None, fused=False)
        arg5 = out5["m0"][0, :p.n0] if side == 1 else out5["m1"][0, :p.n1]
        assert all(arg5[o] == lowest for o, lowest in entries)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_flags_are_the_rule_on_the_eps_table(fmt):
    table, margin = R.eps_table(fmt)
    ref = R.case_ref(R.FLAG_CASE, fmt)
    inp = R.case_inputs(R.FLAG_CASE)
    swapped_inp = R.swap_sides(inp)
    swapped_ref = R.CaseRef(swapped_inp, fmt)
    for e in table:
        r, i = (swapped_ref, swapped_inp) if e["swap"] else (ref, inp)
        out = _run(fmt, i, e["th"], e["eps"])
        d = _distance(out, r)
        assert d <= r.budget and 8 * d <= margin, (e["kind"], d)
        verdicts = _check_flags(out, r, e["th"], e["eps"])
        # where the entry's eps keeps its margin from the pair's critical values, fp64 fixes the verdicts: the kernel must evaluate (a), (b) and (c) as stated
        held = [b for b in range(r.inp["B"]) if R.pair_margin(ref, e, b) >= margin]
        assert e["pair"] is None or e["pair"] in held
        for b in held:
            assert verdicts[b] == e["expect"][b], (e["kind"], b, verdicts[b], e["expect"][b])
            assert out["flags"][b] == int(any(e["expect"][b])), (e["kind"], b)
        print(f"\n  {fmt} {e['kind']}: th {e['th']:.4g} eps {e['eps']:.4g} flags {out['flags'].tolist()} fixed by fp64 in pairs {held}")


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("case", ["np256", "b8_np256", "np512"])
def test_five_pass_form_against_fp64(case, fmt):
    ref = R.case_ref(case, fmt)
    out = _run(fmt, R.case_inputs(case), R.TH, MAIN_EPS, fused=False)
    d = _distance(out, ref, FIVE_PASS_VALUES)
    print(f"\n| {case} | {fmt} five-pass | d {d:.3g} | e32 {ref.e32:.3g} | d / e32 {d / ref.e32:.2f} |")
    assert d <= ref.budget, (d, ref.e32)
    _check_decisions(out, ref, d)
    _check_list(out, ref, R.TH, d, True)
    assert out["flags"].tolist() == [int(p.decides) for p in ref.pairs]      # k_compact: no runner-ups, so every pair that has a decision reports 1


def test_column_values_a_calibration_measured_are_readable_by_name():
    """gn_calibrate_certify with the ladder on measures the middle level over rows AND columns; its last pass is such a one, over the whole sample, so
    afterwards "colbest" / "col2" hold the column scores that pass compared, next to the same pass's row vectors: on a mutual pair the column's best IS
    the row's best, bit for bit (one score_at() value read by both reductions)."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.synthetic import make_pair
    from gisnav_amd.weights import synthetic_state_dict
    shape = [(200, 180), (97, 256)]
    eng = PoseEngine(0, max_batch=2, max_kpts=256, precision="f16x2_bf16_attn", state_dict=synthetic_state_dict(0))
    inp = eng.stage_inputs([make_pair(7300 + i, n_q=a, n_r=b) for i, (a, b) in enumerate(shape)])
    eng.set_certify_ladder(True)
    cal = eng.calibrate_certify(inp)
    assert cal["eps_mid"] > 0.0                       # the middle level's pass ran
    v = {k: eng.debug_read(k, 2 * 256).reshape(2, 256) for k in ("max0", "colbest", "col2")}
    v.update({k: eng.debug_read(k, 2 * 256, np.int32).reshape(2, 256) for k in ("m0", "m1")})
    for b, (n0, n1) in enumerate(shape):
        cb, c2, m0, m1 = v["colbest"][b, :n1], v["col2"][b, :n1], v["m0"][b, :n0], v["m1"][b, :n1]
        assert np.all(np.isfinite(cb)) and np.all(np.isfinite(c2)) and np.all(c2 <= cb) and np.all(cb <= 0.0)
        rows = np.nonzero(m1[m0] == np.arange(n0))[0]
        assert len(rows) > 20
        assert np.array_equal(cb[m0[rows]], v["max0"][b, rows])
        assert np.array_equal(cb[np.arange(n1)[m0[m1] == np.arange(n1)]], v["max0"][b, m1[m0[m1] == np.arange(n1)]])

"""GPU tests (-m gpu): the preparation kernels, the f32-accurate modes and the margin certificate against float64 on inputs unlike the calibration's.

gn_calibrate_certify measures eps = safety x max |P_mode - P_f32| on a sample; "|P - P_exact| <= eps on the deciding entries" is then an empirical
premise, and every calibration and every certified-vs-fp64 test of the suite so far drew sample and test pairs from one generator (make_pair).  The
product calibrates on its first messages and certifies every later frame with that eps.  Here the calibration sample stays make_pair (four pairs of
other seeds) and the tested pairs come from tests/ood_inputs_common.py: an extractor's real output (shared positions, small sizes, clamped
descriptors), keypoints squeezed into a corner of the extent with sizes up to ~120, repeated structure with exact duplicates, three-bin and all-zero
descriptors, correlated 256-d descriptors -- and `base`, make_pair itself, as the in-distribution control of the same run.  tests/test_ood_inputs_host.py
shows on the CPU that the families are what they claim, that the f32 oracle alone keeps the budgets used here, and that the cases cannot pass vacuously.

Everything runs at 4 x 512, the smallest grid at which every kernel family can be made to run: the bulk kernels forced (test_gpu_round6._forced_headline:
k_qkv, k_attn_pw, k_ffn128 on levels 3 / 2 / 1 and the one-product projection rung), the small-grid kernels unforced, the skinny family on the first
pair alone.  Every case asserts the family from the launch table.

  (a) preparation (k_extent, k_prep; k_prep_sp): desc, cos, sin, extent, nvalid behind one call against the fp64 oracle's RootSIFT, encoding tables and
      extent -- tests/test_gpu_parity.py's bounds (1e-6 relative on desc, 2e-5 absolute on the tables), padding slots inert (0, cos 1, sin 0), all-zero
      descriptors give exact zeros, everything finite;
  (b) f32 and mode 5 (f16x2_f16x2_attn): layers 1 / 5 / 9 and the head's best / runner-up of every row inside F32_LAYER, F32_HEAD;
  (c) the certificate's premise out of sample: headline mode, set_ffn_products("auto"), ladder on, calibrated once per weight family and kernel grid
      on the make_pair sample with safety 4; per family and level that ran, d = max |P - P_fp64| over the rows the calibration rule looks at
      (test_gpu_fp64_parity._head_d) must stay within that level's eps (mode-5 arithmetic: within eps_mid).  d / eps of every case is reported next
      to the `base` row of the same run.  The 16-bit levels' layer errors are recorded, not budgeted (their budgets elsewhere are 2 x maxima measured
      on make_pair: a larger figure here is information);
  (d) "flag": every pair the certificate does not flag has fp64's match set, index for index; `repeated` has a flagged pair and the family the host
      module names has an unflagged one (default-init weights, threshold 0: every pair of every family holds a margin below 4e-2 -- there the case
      can only check that `repeated` is flagged);
  (e) "rerun": match sets equal fp64's except in at most certify_stats()["f32_marginal_pairs"] pairs; re-run and ladder counts are reported;
  (f) the node's way: a one-pair context calibrates on one make_pair pair as pose_node.py does, then certifies one pair of every family at
      set_active_kpts(max(n_q, n_r)) under the (e) rule.

Numbers go to test_reports/ood_inputs.json (git-ignored), stamped with the digest of the loaded library; DESIGN 11.8 quotes them.

Measured on an MI355X.  (a) desc 7.3e-8, tables <= 5.8e-6 (`clustered`, default-init weights).  (b) layers <= 1.8e-6, head <= 5.1e-5.  (c) with eps
from the dense make_pair sample alone the three-product level failed on `sparse`: d / eps 0.90 (margin-built, bulk kernels), 0.87 (one pair, skinny
kernels), 1.15 on mid-margin weights (d 2.41e-3, eps 2.10e-3), the control 0.15 / 0.12 / 0.23 -- few strong bins make a larger input to every block.
gn_calibrate_certify now also measures the sample with every descriptor cut to its three largest bins; since then d / eps <= 0.37 on every family,
level and grid (`sparse` up to 0.37, every other family <= 0.26).  (d) no unflagged pair differs from fp64; (e), (f) no certified pair does.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ood_inputs_common as oc  # noqa: E402
import test_gpu_fp64_parity as fp  # noqa: E402
from test_gpu_fp64_parity import F32_HEAD, F32_LAYER, HEADLINE, MODE5, SAFETY, _head_d, _match, _names, _staged  # noqa: E402
from test_gpu_round6 import _forced_headline  # noqa: E402
from test_ood_inputs_host import DESC_REL, PASSES, TABLE_ABS, WEIGHTS  # noqa: E402

pytestmark = pytest.mark.gpu
B, K = oc.N_PAIRS, oc.MAX_KPTS
_RUNS = {}


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "ood_inputs.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    if data.get("source_digest") != _lib.library_digest():
        data = {"source_digest": _lib.library_digest()}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    print(key, json.dumps(value, sort_keys=True))


def _engine(weights, prec, max_batch=B):
    from gisnav_amd.engine import PoseEngine
    sd, th = oc.state_dict(weights)
    return PoseEngine(0, max_batch=max_batch, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=th,
                      feature="superpoint" if weights.startswith("sp_") else "sift"), th


def _nvalid(pairs):
    return [(len(p.kp_q), len(p.kp_r)) for p in pairs]


def _layer_error(eng, nb, refs, nvalid, nl):
    """max |x - x64| / max |x64| over the valid rows of each side behind layer nl (x as the last call left it)"""
    x = eng.debug_read("x", nb * 2 * K * 256).reshape(nb, 2, K, 256)
    err = 0.0
    for b, r in enumerate(refs):
        for s in (0, 1):
            a, ref = x[b, s, : nvalid[b][s]], r["layers"][nl][s]
            assert np.isfinite(a).all(), (b, s)
            err = max(err, float(np.abs(a - ref).max() / np.abs(ref).max()))
    return err


def _layers(eng, inp, nb, refs, nvalid):
    """{layer1_rel, layer5_rel}: two shortened calls; the caller's own 9-layer call gives layer 9 (_layer_error(..., 9))"""
    row = {}
    for nl in oc.LAYERS[:-1]:
        eng.set_num_layers(nl)
        _match(eng, inp)
        row[f"layer{nl}_rel"] = _layer_error(eng, nb, refs, nvalid, nl)
    eng.set_num_layers(oc.LAYERS[-1])
    return row


def _sets(idx, n, b):
    return {(int(q), int(c)) for q, c in idx[b, : int(n[b])]}


def _want(r):
    return {(int(q), int(c)) for q, c in r["idx"]}


# ---------------------------------------------------------------------------------------------------------------- (a) preparation
def _prep_tables(eng, pairs, refs, what):
    T = B * 2 * K
    cos, sin = eng.debug_read("cos", T * 32).reshape(B, 2, K, 32), eng.debug_read("sin", T * 32).reshape(B, 2, K, 32)
    extent, nv = eng.debug_read("extent", B * 4).reshape(B, 2, 2), eng.debug_read("nvalid", B * 2, np.int32).reshape(B, 2)
    worst = 0.0
    for b, (p, r) in enumerate(zip(pairs, refs)):
        for s, kp in enumerate((p.kp_q, p.kp_r)):
            n = len(kp)
            assert nv[b, s] == n, (what, b, s, nv[b, s])
            assert np.array_equal(extent[b, s], kp.max(0)), (what, b, s, extent[b, s], kp.max(0))      # a maximum of float32 values: exact
            assert np.isfinite(cos[b, s]).all() and np.isfinite(sin[b, s]).all(), (what, b, s)
            d = max(float(np.abs(cos[b, s, :n] - r["cos"][s]).max()), float(np.abs(sin[b, s, :n] - r["sin"][s]).max()))
            worst = max(worst, d)
            assert (cos[b, s, n:] == 1.0).all() and (sin[b, s, n:] == 0.0).all(), (what, b, s)        # padding slots: inert
    return worst


@pytest.mark.parametrize("name", oc.SIFT_FAMILIES)
def test_preparation_stage_against_fp64(name):
    """k_extent + k_prep of a headline context (which also writes the hm16 rows and the rotary table from the same values), margin-built and
    default-init weights (the encoding's Wr differs: default-init's is the larger)."""
    pairs = oc.family(name)
    row = {}
    for weights in ("margin_built", "default_init"):
        refs = oc.refs(weights, name)
        eng, _ = _engine(weights, HEADLINE)
        eng.set_num_layers(1)
        _match(eng, _staged(eng, pairs))
        tab = _prep_tables(eng, pairs, refs, (name, weights))
        desc = eng.debug_read("desc", B * 2 * K * 128).reshape(B, 2, K, 128)
        del eng
        rel = 0.0
        for b, (p, r) in enumerate(zip(pairs, refs)):
            for s, d_in in enumerate((p.desc_q, p.desc_r)):
                n = len(d_in)
                assert np.isfinite(desc[b, s]).all() and (desc[b, s, n:] == 0.0).all(), (name, b, s)
                rel = max(rel, float(np.abs(desc[b, s, :n] - r["desc"][s]).max() / np.abs(r["desc"][s]).max()))
                zero = np.flatnonzero(~d_in.any(1))
                assert (desc[b, s, zero] == 0.0).all(), (name, b, s, zero)       # RootSIFT of an all-zero row: 0 / max(0, 1e-12)
                if name == "sparse" and s == 0:
                    assert len(zero) == 2
        row[weights] = {"tables_abs": tab, "desc_rel": rel}
    _report(f"prep_{name}", row)
    for weights, v in row.items():
        assert v["desc_rel"] <= DESC_REL and v["tables_abs"] <= TABLE_ABS, (weights, row)


@pytest.mark.parametrize("name", oc.SP_FAMILIES)
def test_preparation_stage_256d_against_fp64(name):
    """k_extent + k_prep_sp: an f32 context stopped behind its first projection (developer knob 4) still holds the residual stream as k_prep_sp
    wrote it -- the descriptors, bit for bit, zeros in the padding -- and the tables of the 2-D encoding."""
    pairs, refs = oc.family(name), oc.refs("sp_margin_built", name)
    eng, _ = _engine("sp_margin_built", "f32")
    assert eng.lib.gn_debug_set_variant(eng.ctx, 4, 1) == 0
    _match(eng, _staged(eng, pairs))
    tab = _prep_tables(eng, pairs, refs, name)
    x = eng.debug_read("x", B * 2 * K * 256).reshape(B, 2, K, 256)
    eng.lib.gn_debug_set_variant(eng.ctx, 4, 0)
    del eng
    for b, p in enumerate(pairs):
        for s, d_in in enumerate((p.desc_q, p.desc_r)):
            n = len(d_in)
            assert np.array_equal(x[b, s, :n].view(np.uint32), d_in.view(np.uint32)) and (x[b, s, n:] == 0.0).all(), (name, b, s)
    _report(f"prep_{name}", {"tables_abs": tab})
    assert tab <= TABLE_ABS, tab


# ---------------------------------------------------------------------------------------------------------------- (b) f32 and mode 5
@pytest.mark.parametrize("prec,weights", [(prec, w) for prec in ("f32", MODE5) for w in WEIGHTS] + [("f32", "sp_margin_built")])
def test_f32_accurate_modes_keep_the_f32_budgets_on_every_family(prec, weights):
    eng, th = _engine(weights, prec)
    eng.set_certify("flag")
    rows, fails = {}, []
    for name in (oc.SP_FAMILIES if weights.startswith("sp_") else oc.SIFT_FAMILIES):
        pairs, refs = oc.family(name), oc.refs(weights, name)
        nvalid = _nvalid(pairs)
        inp = _staged(eng, pairs)
        row = _layers(eng, inp, B, refs, nvalid)
        (_, _, n), names = _names(eng, inp)
        fp._family_check(names, prec, "4x512", 3)
        row["layer9_rel"] = _layer_error(eng, B, refs, nvalid, 9)
        row["head_dP"], _ = _head_d(eng, B, K, refs, nvalid)
        rows[name] = row
        if max(row[f"layer{nl}_rel"] for nl in oc.LAYERS) > F32_LAYER or row["head_dP"] > F32_HEAD:
            fails.append((name, row))
    del eng
    _report(f"f32_budgets_{prec}_{weights}", rows)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- (c) (d) (e) the certificate
def _level_setting(eng, level):
    if level == "proj1":        # the rung below level 1: one-product attention input projections
        eng.set_ffn_products(1)
        eng.set_qkv_products(1)
    else:
        eng.set_qkv_products("auto")
        eng.set_ffn_products(level)


def _check_family(names, grid, level, nb):
    ffn = [nm for nm in names if nm.startswith("k_ffn128")]
    if grid == "bulk":
        prod = "1" if level == "proj1" else str(level)
        assert ffn and all(nm.rstrip(">").split(", ")[4] == prod for nm in ffn), names
        assert any(nm.startswith("k_attn_pw") for nm in names) and any(nm.startswith("k_qkv") for nm in names), names
        one = [nm for nm in names if nm.startswith("k_qkv") and nm.endswith(", 1>")] + [nm for nm in ffn if nm.rstrip(">").split(", ")[3] in ("3", "4")]
        assert bool(one) == (level == "proj1"), names
    else:
        assert not ffn and not any(nm.startswith(("k_qkv", "k_attn_pw")) for nm in names), names
        assert any(nm.startswith("k_skinny") for nm in names) == (nb == 1), names


def _certificate_run(weights):
    """One headline context per weight family: calibrated on the make_pair sample per kernel grid, then every family on every level (c), under
    "flag" (d) and under "rerun" (e).  Computed once, the three tests below assert their parts."""
    if weights in _RUNS:
        return _RUNS[weights]
    sp = weights.startswith("sp_")
    families = oc.SP_FAMILIES if sp else oc.SIFT_FAMILIES
    eng, th = _engine(weights, HEADLINE)
    eng.set_ffn_products("auto")
    if not sp:
        eng.set_certify_ladder(True)
    cal_inp = eng.stage_inputs(oc.sp_calibration_pairs() if sp else oc.calibration_pairs())
    out = {"c": {}, "d": {}, "e": {}, "cal": {}}
    try:
        for grid in (("small",) if sp else ("bulk", "small")):       # (256-d: the shared kernels are the SIFT cases'; its own are k_prep_sp and the encoding)
            _forced_headline(eng, grid == "bulk")
            cal = eng.calibrate_certify(cal_inp, safety=SAFETY)
            out["cal"][grid] = cal
            eps = {3: cal["eps_three_products"], 2: cal["eps_two_products"], 1: cal["eps_one_product"], "proj1": cal["eps_one_product_projection"]}
            for name in families:
                pairs, refs = oc.family(name), oc.refs(weights, name)
                nvalid = _nvalid(pairs)
                calls = [(B, _staged(eng, pairs), refs, nvalid)]
                if grid == "small":      # the first pair alone: the skinny family
                    calls.append((1, _staged(eng, pairs[:1]), refs[:1], nvalid[:1]))
                for nb, inp, rf, nv in calls:
                    eng.set_certify("flag")
                    for level in ((3, 2, 1, "proj1") if grid == "bulk" else (3,)):
                        _level_setting(eng, level)
                        row = _layers(eng, inp, nb, rf, nv)
                        (_, _, _), names = _names(eng, inp)
                        _check_family(names, grid, level, nb)
                        row["layer9_rel"] = _layer_error(eng, nb, rf, nv, 9)
                        d_all, d = _head_d(eng, nb, K, rf, nv, th)
                        row.update(d=d, d_all_rows=d_all, eps=eps[level], d_over_eps=d / eps[level])
                        out["c"][f"{name}_{grid}_{nb}x512_lvl{level}"] = row
                    eng.set_qkv_products("auto")
                    eng.set_ffn_products("auto")
                    # (d) flag: what the fast pass alone returns, and which pairs the kernel's own flag logic vouches for
                    idx, _, n = _match(eng, inp)
                    flags = eng.uncertain(nb)
                    wrong = [b for b, r in enumerate(rf) if _sets(idx, n, b) != _want(r)]
                    out["d"][f"{name}_{grid}_{nb}x512"] = {"flags": flags.tolist(), "pairs_differing_from_fp64": wrong,
                                                           "unflagged_wrong": [b for b in wrong if flags[b] == 0], "matches_fp64": [len(r["idx"]) for r in rf]}
                    # (e) rerun
                    eng.set_certify("rerun")
                    eng.certify_stats(reset=True)
                    idx, _, n = _match(eng, inp)
                    st = eng.certify_stats()
                    e = {"pairs_differing_from_fp64": [b for b, r in enumerate(rf) if _sets(idx, n, b) != _want(r)],
                         "f32_marginal_pairs": st["f32_marginal_pairs"], "rerun_pairs": st["rerun_pairs"], "pairs": st["pairs"], "flagged_fp16_range": st["flagged_fp16_range"]}
                    if not sp:
                        e.update({k: v for k, v in eng.certify_ladder_stats().items() if k != "eps_mid"})
                    out["e"][f"{name}_{grid}_{nb}x512"] = e
    finally:
        _forced_headline(eng, False)
        del eng
    if not sp:
        # the ladder's middle level: mode-5 arithmetic (a mode-5 context on the same weights), four pairs and the first pair alone, against eps_mid
        e5, _ = _engine(weights, MODE5)
        e5.set_certify("flag")
        for name in families:
            pairs, refs = oc.family(name), oc.refs(weights, name)
            for nb in (B, 1):
                (_, _, _), names = _names(e5, _staged(e5, pairs[:nb]))
                assert any(nm.startswith("k_attn_f16x2") for nm in names), names
                _, d = _head_d(e5, nb, K, refs[:nb], _nvalid(pairs[:nb]), th)
                em = out["cal"]["small"]["eps_mid"]
                out["c"][f"{name}_mode5_{nb}x512_mid"] = {"d": d, "eps": em, "d_over_eps": d / em, "eps_mid_bulk_calibration": out["cal"]["bulk"]["eps_mid"]}
        del e5
    _report(f"certificate_{weights}", out)
    _RUNS[weights] = out
    return out


CERT_WEIGHTS = WEIGHTS + ("sp_margin_built",)


@pytest.mark.parametrize("weights", CERT_WEIGHTS)
def test_calibrated_eps_bounds_the_error_against_fp64_on_every_family(weights):
    """(c): d <= eps of the level that ran, for every family, grid and level; `base` is the control."""
    out = _certificate_run(weights)
    fails = {k: (v["d"], v["eps"]) for k, v in out["c"].items() if not v["d"] <= v["eps"]}
    table = {k: round(v["d_over_eps"], 3) for k, v in out["c"].items()}
    print(weights, "d / eps", json.dumps(table, sort_keys=True))
    assert all(v["eps"] > 0.0 and np.isfinite(v["d"]) for v in out["c"].values())
    assert not fails, (fails, out["cal"])


@pytest.mark.parametrize("weights", CERT_WEIGHTS)
def test_unflagged_pairs_have_the_fp64_match_set(weights):
    """(d): no exclusions -- a pair the certificate does not flag has every gap above 2 eps."""
    out = _certificate_run(weights)
    bad = {k: v for k, v in out["d"].items() if v["unflagged_wrong"]}
    assert not bad, bad
    four = {k: v for k, v in out["d"].items() if f"_{B}x512" in k}
    if not weights.startswith("sp_"):
        assert all(any(v["flags"]) for k, v in four.items() if k.startswith("repeated_")), four        # the certificate has something to flag ...
    if PASSES[weights] is not None:      # ... and something to pass (None: tests/test_ood_inputs_host.py shows there is no such pair)
        assert all(not all(v["flags"]) for k, v in four.items() if k.startswith(PASSES[weights] + "_")), four


@pytest.mark.parametrize("weights", CERT_WEIGHTS)
def test_certified_match_sets_equal_fp64_but_for_f32_marginal_pairs(weights):
    """(e): tests/test_gpu_fp64_parity.py's rule for a certified call."""
    out = _certificate_run(weights)
    bad = {k: v for k, v in out["e"].items() if len(v["pairs_differing_from_fp64"]) > v["f32_marginal_pairs"]}
    assert all(v["pairs"] in (1, B) for v in out["e"].values())
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (f) the node's way
@pytest.mark.parametrize("weights", WEIGHTS)
def test_one_pair_context_calibrated_on_its_first_message_certifies_every_family(weights):
    """pose_node.py: a one-pair context, set_active_kpts(max(n_q, n_r)) per message, calibrate_certify on the first message (safety 4, its default),
    set_certify("rerun", eps) and the ladder's eps_mid from it; then one pair of every family."""
    eng, th = _engine(weights, HEADLINE, max_batch=1)
    eng.set_certify_ladder(True)
    first = oc.calibration_pairs()[0]
    assert eng.set_active_kpts(max(len(first.kp_q), len(first.kp_r))) == K
    inp = eng.stage_inputs([first])
    cal = eng.calibrate_certify(inp)
    # the node uploads the message's 532-byte records as they are: the calibration (its cut-descriptor pass reads the descriptor out of the record)
    # must state the same eps, bit for bit, as on the unpacked arrays
    from gisnav_amd import _lib
    from gisnav_amd.wire import pack_keypoints
    rq, rr = (torch.from_numpy(np.frombuffer(pack_keypoints(*a), dtype=np.float32).reshape(1, -1, 133).copy()).to(eng.device)
              for a in ((first.kp_q, first.size_q, first.angle_q, first.desc_q), (first.kp_r, first.size_r, first.angle_r, first.desc_r)))
    cal_rec = eng.calibrate_certify(dict(desc_q=None, desc_r=None, kpt_q=rq, kpt_r=rr, n_q=inp["n_q"], n_r=inp["n_r"], kpt_format=_lib.GN_KPT_RECORD))
    assert cal_rec == cal, (cal_rec, cal)
    eng.set_certify("flag", eps=cal["eps"])
    _, names = _names(eng, eng.stage_inputs([first]))
    assert any(nm.startswith("k_skinny") for nm in names), names          # (one pair: the family follows the pair count)
    eng.set_certify("rerun", eps=cal["eps"])
    eng.set_certify_ladder(True, eps_mid=cal["eps_mid"])
    rows, bad = {"calibration": cal}, []
    for name in oc.SIFT_FAMILIES:
        p, r = oc.family(name)[1], oc.ref(weights, name, 1)
        assert eng.set_active_kpts(max(len(p.kp_q), len(p.kp_r))) == K
        eng.certify_stats(reset=True)
        idx, _, n = _match(eng, eng.stage_inputs([p]))
        st = eng.certify_stats()
        differs = _sets(idx, n, 0) != _want(r)
        rows[name] = {"differs_from_fp64": differs, "rerun_pairs": st["rerun_pairs"], "f32_marginal_pairs": st["f32_marginal_pairs"], "matches_fp64": len(r["idx"]),
                      **{k: v for k, v in eng.certify_ladder_stats().items() if k != "eps_mid"}}
        if int(differs) > st["f32_marginal_pairs"]:
            bad.append(name)
    eng.set_active_kpts(K)
    del eng
    _report(f"node_{weights}", rows)
    assert not bad, (bad, rows)

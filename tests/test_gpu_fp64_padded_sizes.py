"""GPU tests (-m gpu) of the LightGlue matcher against float64 at the padded sizes its callers run it at.

PoseNode, PoseEngine.estimate_bucketed and estimate_images all call set_active_kpts(max(n_q, n_r)): any multiple of 128 up to the context's
max_kpts.  tests/test_gpu_fp64_parity.py runs every case at 512 or 1024 slots a side; the dispatch in gn_api.hip pairs other kernels at other
sizes (tests/padded_sizes_common.py lists the pairs and why each size is there):

  1. one pair on a 4096-slot context at P = 128 .. 4096 (k_skinny_qkv / k_skinny_h / k_skinny_out, k_attn_ks on P / 32 workgroups, the fused
     head's P / 32 partial rows), headline mode, mode 5 and f32;
  2. groups whose kernel family turns on the padding: 8 x 1152 (k_qkv feeding k_attn16_v5, small-grid block tail), 26 x 640 (k_qkv fused into
     k_ffn128 at three, two and one products and both work-list forms, feeding k_attn16_v5; the fused-projection self-check at an odd tile count),
     8 x 1024 on a 2048-slot context (k_qkv and k_attn_pw with the small-grid tail);
  3. what padding may change: one pair at 256 against 4096 slots (bitwise: the family follows the pair count), eight pairs at 512, 1024 and 2048
     slots (bitwise where the launch table shows one family, the fp64 budgets where it does not, identical match sets under the certificate).

Measures, weights (margin-built, threshold 0.5) and budgets are those of tests/test_gpu_fp64_parity.py: per layer max |x - x64| / max |x64| over the
valid rows of each side after layers 1, 5 and 9, head max |P - P64| of the best and runner-up score of every valid row.  The budget constants are
copied from that module (tests/test_padded_sizes_host.py compares them), not measured on the code under test.  Every case asserts from the launch
table (set_kernel_timing) which family ran; measured values go to test_reports/fp64_padded_sizes.json (git-ignored), stamped with the digest of
the loaded library.  DESIGN 11.7 quotes them.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import padded_sizes_common as pc  # noqa: E402

pytestmark = pytest.mark.gpu
HEADLINE = "f16x2_f16_attn"
MODE5 = "f16x2_f16x2_attn"
SAFETY = 4.0
LAYERS = pc.LAYERS
# tests/test_gpu_fp64_parity.py's budgets against fp64 (its F32_LAYER / F32_HEAD, FP16_LAYER / FP16_HEAD; level 1 = 2 x level 2, and its layer error
# on the pairs with >= 256 keypoints a side at most LEVEL1_OVER_LEVEL2 x the level-2 case's of the same process)
F32_LAYER, F32_HEAD = 2e-5, 1e-4
FP16_LAYER = {3: 6.5e-5, 2: 1.6e-4, 1: 3.2e-4}
FP16_HEAD = {3: 1.1e-3, 2: 4e-3, 1: 8e-3}
LEVEL1_OVER_LEVEL2 = 2.0
NEEDS_PER_CASE = "run with the level-2 case of this module (it measures what is compared here)"
SIXTEEN_BIT = ("k_skinny", "k_attn_ks", "k_qkv", "k_attn_pw", "k_attn16", "k_attn_bf16", "k_attn_f16x2", "k_ffn128", "k_ffn_fused")
_MEASURED = {}


def _budget(prec, level=3):
    return (FP16_LAYER[level], FP16_HEAD[level]) if prec == HEADLINE else (F32_LAYER, F32_HEAD)


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "fp64_padded_sizes.json")
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


# ---------------------------------------------------------------------------------------------------------------- GPU side
def _engine(B, K, prec):
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=pc.state_dict(), filter_threshold=pc.THRESHOLD)


def _match(eng, inp):
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()


def _names(eng, inp):
    eng.set_kernel_timing(400)
    out = _match(eng, inp)
    names = [r["name"] for r in eng.kernel_table()]
    eng.set_kernel_timing(0)
    return out, names


def _has(names, *prefixes):
    return any(n.startswith(prefixes) for n in names)


def _read_x(eng, B, P):
    """the residual stream as the call laid it out: [pair][side][P rows][256] at the active size P"""
    return eng.debug_read("x", B * 2 * P * 256).reshape(B, 2, P, 256)


def _x_error(x, refs, nvalid, nl, only=None):
    err = 0.0
    for b, r in enumerate(refs):
        if only is not None and b not in only:
            continue
        for s in (0, 1):
            a = x[b, s, :nvalid[b][s]]
            assert np.isfinite(a).all(), (b, s)
            ref = r["layers"][nl][s]
            err = max(err, float(np.abs(a - ref).max() / np.abs(ref).max()))
    return err


def _head_error(eng, B, P, refs, nvalid):
    best = eng.debug_read("max0", B * P).reshape(B, P)
    second = eng.debug_read("max0b", B * P).reshape(B, P)
    d = 0.0
    for b, r in enumerate(refs):
        n = nvalid[b][0]
        assert np.isfinite(best[b, :n]).all() and np.isfinite(second[b, :n]).all(), b
        d = max(d, float(np.abs(best[b, :n].astype(np.float64) - r["best"]).max()), float(np.abs(second[b, :n].astype(np.float64) - r["second"]).max()))
    return d


def _measure(eng, inp, B, P, refs, nvalid):
    """The module's measures of one staged batch at active size P: (row, names, (idx, score, n), valid rows of x after the last layer)."""
    ordinary = {b for b, nv in enumerate(nvalid) if min(nv) >= 256}
    row = {}
    for nl in LAYERS:
        eng.set_num_layers(nl)
        if nl == LAYERS[-1]:
            eng.set_certify("flag")      # (the head keeps every row's runner-up: max0b)
            out, names = _names(eng, inp)
        else:
            _match(eng, inp)
        x = _read_x(eng, B, P)
        row[f"layer{nl}_rel"] = _x_error(x, refs, nvalid, nl)
        if ordinary:
            row[f"layer{nl}_rel_ordinary"] = _x_error(x, refs, nvalid, nl, ordinary)
    row["head_dP"] = _head_error(eng, B, P, refs, nvalid)
    valid = [x[b, s, :nvalid[b][s]].copy() for b in range(B) for s in (0, 1)]
    return row, names, out, valid


def _assert_budget(row, prec, level=3):
    lb, hb = _budget(prec, level)
    for nl in LAYERS:
        assert row[f"layer{nl}_rel"] <= lb, (nl, lb, row)
    assert row["head_dP"] <= hb, (hb, row)


def _bit_differences(a, b):
    """two runs' (idx, score, n, valid residual rows), bit for bit: what differs (nothing: [])"""
    (ia, sa, na, xa), (ib, sb, nb, xb) = a, b
    if not np.array_equal(na, nb):
        return [("match counts", na.tolist(), nb.tolist())]
    diff = []
    for p in range(len(na)):
        k = int(na[p])
        if not np.array_equal(ia[p, :k], ib[p, :k]):
            diff.append(("indices of pair", p))
        if not np.array_equal(sa[p, :k].view(np.uint32), sb[p, :k].view(np.uint32)):
            diff.append(("scores of pair", p))
    diff += [("residual stream of pair / side", divmod(i, 2)) for i, (u, v) in enumerate(zip(xa, xb)) if not np.array_equal(u.view(np.uint32), v.view(np.uint32))]
    return diff


def _match_sets(idx, n):
    return [{(int(q), int(c)) for q, c in idx[b, : n[b]]} for b in range(len(n))]


# ---------------------------------------------------------------------------------------------------------------- 1. one pair at the node's sizes
@pytest.mark.parametrize("P", pc.SINGLE_SIZES)
@pytest.mark.parametrize("prec", [HEADLINE, MODE5, "f32"])
def test_one_pair_at_the_nodes_sizes(prec, P):
    """PoseNode's call: one pair on a 4096-slot context at set_active_kpts(max(n_q, n_r))."""
    p = pc.single_pair(P)
    refs, nvalid = [pc.ref64(p)], [(len(p.kp_q), len(p.kp_r))]
    eng = _engine(1, 4096, prec)
    assert eng.set_active_kpts(max(nvalid[0])) == P
    row, names, (idx, score, n), _ = _measure(eng, eng.stage_inputs([p]), 1, P, refs, nvalid)
    del eng
    if prec == HEADLINE:
        assert all(_has(names, k) for k in ("k_skinny_qkv", "k_skinny_h", "k_skinny_out", "k_attn_ks")), names
        assert not _has(names, "k_qkv", "k_attn_pw", "k_ffn128", "k_attn16"), names
    elif prec == MODE5:
        assert _has(names, "k_attn_f16x2"), names
        assert not _has(names, "k_attn_pw", "k_attn16", "k_attn_bf16", "k_qkv", "k_attn_f32", "k_attn_ks"), names
    else:
        assert not _has(names, *SIXTEEN_BIT), names
    row["kernels"] = sorted(set(names))
    row["matches"], row["matches_fp64"] = int(n[0]), len(refs[0]["idx"])
    _report(f"one_pair_{prec}_P{P}", row)
    _assert_budget(row, prec)


# ---------------------------------------------------------------------------------------------------------------- 2. groups of several pairs
def _group_case(name, level=3, lists=None):
    pairs, B, K, (P,) = pc.group(name)
    refs = [pc.ref64(p) for p in pairs]
    nvalid = [(len(p.kp_q), len(p.kp_r)) for p in pairs]
    eng = _engine(B, K, HEADLINE)
    if level != 3:
        eng.set_ffn_products(level)
    if lists is not None:
        eng.lib.gn_debug_set_variant(eng.ctx, 31, lists)
    assert eng.set_active_kpts(P) == P
    inp = eng.stage_inputs(pairs)
    _match(eng, inp)
    status = eng.fused_projection_status()      # (after the context's first call)
    row, names, out, _ = _measure(eng, inp, B, P, refs, nvalid)
    del eng
    row["kernels"] = sorted(set(names))
    return row, names, status


def test_eight_pairs_at_1152_run_k_qkv_into_k_attn16_v5():
    """16 x 1152 / 128 = 144 tiles: k_qkv (>= 128), the small-grid block tail (< 256), and k_attn16_v5 because 1152 % 256 != 0."""
    row, names, _ = _group_case("8x1152")
    assert _has(names, "k_qkv") and _has(names, "k_attn16_v5") and not _has(names, "k_attn_pw", "k_ffn128"), names
    _report("group_8x1152", row)
    _assert_budget(row, HEADLINE)


@pytest.mark.parametrize("level", [3, 2, 1])
@pytest.mark.parametrize("lists", [pytest.param(2, id="walk"), pytest.param(3, id="onetile")])
def test_26_pairs_at_640_run_k_ffn128_into_k_attn16_v5(lists, level):
    """52 x 640 / 128 = 260 tiles, the fewest pairs that reach k_ffn128 at five tiles a side: the projection fused into k_ffn128 (and k_qkv for the
    first block) feeds k_attn16_v5, k_tile_lists leaves no item lists (640 % 256 != 0), and the fused-projection self-check runs at 26 x 640."""
    row, names, status = _group_case("26x640", level, lists)
    ffn = [n for n in names if n.startswith("k_ffn128")]
    assert _has(names, "k_qkv") and ffn and _has(names, "k_attn16_v5") and not _has(names, "k_attn_pw"), names
    assert all(n.rstrip(">").split(", ")[4] == str(level) for n in ffn), names
    assert all(n.split(", ")[2] == ("true" if lists == 2 else "false") for n in ffn), names
    assert any(n.rstrip(">").split(", ")[3] in ("1", "2") for n in ffn), names      # the next block's projection ran inside the tail
    assert status == 1, status
    two = None
    if level == 1:
        # one more independent rounding of the same relative size: at most 2.0 x the level-2 case, on the pairs with >= 256 keypoints a side
        two = _MEASURED.get((lists, 2))
        if two is None:
            pytest.fail(NEEDS_PER_CASE)
        for nl in LAYERS:
            row[f"layer{nl}_rel_ordinary_over_lvl2"] = row[f"layer{nl}_rel_ordinary"] / two[f"layer{nl}_rel_ordinary"]
    _MEASURED[(lists, level)] = row
    _report(f"group_26x640_lvl{level}_{'walk' if lists == 2 else 'onetile'}", row)
    if level == 1:
        for nl in LAYERS:
            assert row[f"layer{nl}_rel_ordinary"] <= LEVEL1_OVER_LEVEL2 * two[f"layer{nl}_rel_ordinary"], (nl, row, two)
    _assert_budget(row, HEADLINE, level)


def test_eight_pairs_at_1024_of_2048_run_k_qkv_and_k_attn_pw_on_the_small_tail():
    """16 x 1024 / 128 = 128 tiles on a 2048-slot context: k_qkv and k_attn_pw (1024 % 256 == 0, 256 workgroups) with the small-grid block tail."""
    row, names, _ = _group_case("8x1024of2048")
    assert _has(names, "k_qkv") and _has(names, "k_attn_pw") and _has(names, "k_ffn_fused") and not _has(names, "k_ffn128", "k_attn16"), names
    _report("group_8x1024of2048", row)
    _assert_budget(row, HEADLINE)


# ---------------------------------------------------------------------------------------------------------------- 3. what padding may change
@pytest.mark.parametrize("prec", [HEADLINE, MODE5])
def test_one_pair_does_not_depend_on_the_padding(prec):
    """(250, 240) keypoints at 256 and at 4096 slots of one context: the family follows the pair count, so indices, scores and the valid rows of
    the residual stream are the same bits."""
    pairs, B, K, active = pc.group("pad_1")
    refs, nvalid = [pc.ref64(p) for p in pairs], [(len(p.kp_q), len(p.kp_r)) for p in pairs]
    eng = _engine(B, K, prec)
    inp = eng.stage_inputs(pairs)
    runs = {}
    for P in active:
        assert eng.set_active_kpts(P) == P
        row, names, out, valid = _measure(eng, inp, B, P, refs, nvalid)
        runs[P] = (sorted(set(names)), out + (valid,), row)
        _report(f"padding_1_{prec}_P{P}", dict(row, kernels=runs[P][0]))
    del eng
    (fam_a, a, row_a), (fam_b, b, row_b) = runs[active[0]], runs[active[1]]
    assert fam_a == fam_b, (fam_a, fam_b)
    assert int(a[2][0]) >= pc.MIN_MATCHES
    assert _bit_differences(a, b) == []
    _assert_budget(row_a, prec)


@pytest.mark.parametrize("prec", [HEADLINE, MODE5])
def test_eight_pairs_across_padded_sizes(prec):
    """Eight pairs of <= 500 keypoints at 512, 1024 and 2048 slots of one (8, 2048) context.  In the headline mode the family turns on the padding
    (k_qkv from 128 tiles = 1024 slots, k_ffn128 from 256 tiles = 2048 slots, k_attn_pw from 256 workgroups = 1024 slots): results are the same
    bits where the launch table shows the same kernels, within the fp64 budgets everywhere, and under the calibrated certificate ("rerun") the
    match sets are those of fp64 at every size, except in pairs counted as f32-marginal."""
    pairs, B, K, active = pc.group("pad_8")
    refs, nvalid = [pc.ref64(p) for p in pairs], [(len(p.kp_q), len(p.kp_r)) for p in pairs]
    eng = _engine(B, K, prec)
    inp = eng.stage_inputs(pairs)
    runs = {}
    for P in active:
        assert eng.set_active_kpts(P) == P
        row, names, out, valid = _measure(eng, inp, B, P, refs, nvalid)
        runs[P] = (sorted(set(names)), out + (valid,), row)
        if prec == HEADLINE:
            assert _has(names, "k_qkv") == (pc.tiles(B, P) >= 128) and _has(names, "k_ffn128") == (pc.tiles(B, P) >= 256), (P, names)
            assert _has(names, "k_attn_pw") == (P >= 1024) and _has(names, "k_attn16_v5") == (P < 1024), (P, names)
        else:
            assert _has(names, "k_attn_f16x2") and not _has(names, "k_attn_pw", "k_attn16", "k_attn_bf16", "k_qkv", "k_attn_f32"), names
    families = {P: runs[P][0] for P in active}
    size_pairs = [(a, b) for i, a in enumerate(active) for b in active[i + 1:]]
    same = [(a, b) for a, b in size_pairs if families[a] == families[b]]
    differences = {(a, b): _bit_differences(runs[a][1], runs[b][1]) for a, b in size_pairs}
    # (recorded for every two sizes; asserted below where the launch table shows one family)
    summary = {"sizes_with_one_family": same, "sizes_with_equal_bits": [ab for ab in size_pairs if not differences[ab]]}
    for P in active:
        summary[f"P{P}"] = dict(runs[P][2], kernels=families[P])
    # the certificate: calibrated on these pairs at the context's full size, then every size certified with that eps
    eng.set_num_layers(9)
    eng.set_active_kpts(K)
    cal = eng.calibrate_certify(inp, safety=SAFETY)
    eng.set_certify("rerun")
    want = [{(int(q), int(c)) for q, c in r["idx"]} for r in refs]
    sets, marginal = {}, {}
    for P in active:
        assert eng.set_active_kpts(P) == P
        eng.certify_stats(reset=True)
        idx, _, n = _match(eng, inp)
        st = eng.certify_stats()
        sets[P], marginal[P] = _match_sets(idx, n), st["f32_marginal_pairs"]
        differing = [b for b in range(B) if sets[P][b] != want[b]]
        summary[f"P{P}"]["certified"] = {"pairs_differing_from_fp64": len(differing), "f32_marginal_pairs": st["f32_marginal_pairs"], "rerun_pairs": st["rerun_pairs"]}
    summary["calibration"] = dict(cal)
    del eng
    _report(f"padding_8_{prec}", summary)
    for ab in same:
        assert differences[ab] == [], ab
    for P in active:
        _assert_budget(runs[P][2], prec)
        assert int(runs[P][1][2].min()) >= pc.MIN_MATCHES
        assert summary[f"P{P}"]["certified"]["pairs_differing_from_fp64"] <= marginal[P], (P, summary[f"P{P}"])
    for i, a in enumerate(active):
        for b in active[i + 1:]:
            differing = [p for p in range(B) if sets[a][p] != sets[b][p]]
            assert len(differing) <= marginal[a] + marginal[b], (a, b, differing, marginal)

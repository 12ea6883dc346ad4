"""GPU tests (-m gpu) of the one-product block tail, k_ffn128<., ., ., ., 1> (W_h X_h in both GEMMs), and of the automatic level's third level.

  * arithmetic and forms, 4 x 512 with the bulk kernels forced (test_gpu_round6._forced_headline), margin-built weights, one context (module fixture):
    x after the first layer against fp64 (oracle.lightglue_sift.pose_node_match, dtype=float64) on levels 2 and 1 -- level 1 adds one independent
    rounding of the weights, of the relative size of the activations' (2^-12): the two add in quadrature to sqrt 2, the CPU emulation gave 1.3-1.7, the
    bound is 2.0 x level 2's error in the same process --; all eighteen tail launches are `..., 1>`; the walking form gives the one-tile form's bits in
    x and in q | k | V^T; a ragged batch (sides of 2 and of 130 keypoints: a partly valid tile, all-padding tiles) gives the bits of its pairs run alone;
  * certificate, 16 x 1024, level fixed at 1, set_certify("rerun"), margin-built / mid-margin / default-init weights: certified indices and match
    counts equal an exact-f32 context's on every pair, and max |P - P_f32| over the deciding entries of FRESH pairs stays within eps_one; the fused
    projection was proved on this level (fused_projection_status() == 1);
  * automatic level, deferred certificate on two sub-streams: margin-built weights reach level 1 within twelve 16-pair calls with two switches and no
    re-run, mid-margin weights stay on three products; poses equal an f32 context's on every call.
"""
import json
import os

import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import K_MATRIX, make_pair
from tests.test_gpu_round6 import HEADLINE, SAFETY, _family, _forced_headline, _pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B4, K4 = 4, 512
RAGGED = ((2, 512), (130, 300), (512, 130), (400, 2))


def _report(key, value):
    path = os.path.join(ROOT, "test_reports", "ffn_level1_tests.json")      # (git-ignored, as tests/test_gpu_certify_ladder.py's report)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _ref_layer1(tsd, p):
    from oracle import lightglue_sift as lg
    taps = {}
    tq = torch.from_numpy
    lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r), tq(p.angle_r),
                       taps=taps, filter_threshold=0.5, dtype=torch.float64)
    return taps["layer0_0"][0].numpy(), taps["layer0_1"][0].numpy()


def _sizes(pairs):
    return [(len(p.kp_q), len(p.kp_r)) for p in pairs]


def _layer1_error(eng, inp, refs, sizes):
    eng.set_num_layers(1)
    eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    eng.set_num_layers(9)
    x = eng.debug_read("x", B4 * 2 * K4 * 256).reshape(B4, 2, K4, 256)
    err = 0.0
    for b, ref in enumerate(refs):
        for s in (0, 1):
            a = x[b, s, : sizes[b][s]]
            assert np.isfinite(a).all(), (b, s)
            err = max(err, float(np.abs(a - ref[s]).max() / np.abs(ref[s]).max()))
    return err


def _run(eng, inp, nb=B4):
    eng.set_kernel_timing(400)
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table() for _ in range(int(r["launches"])) if r["name"].startswith("k_ffn128")]
    eng.set_kernel_timing(0)
    T = B4 * 2 * K4
    return {"idx": idx.cpu().numpy().copy(), "score": score.cpu().numpy().copy(), "n": n.cpu().numpy().copy(), "names": names,
            "best": eng.debug_read("max0", nb * K4).copy(), "x": eng.debug_read("x", nb * 2 * K4 * 256).copy(),
            # the last projection of the call (the cross block's of layer 9, fused behind the self block's tail): fp16 q | k rows of 256, V^T panels
            "qk": eng.debug_read("qkb", T * 256 // 2, np.uint32).view(np.uint16).copy(), "vt": eng.debug_read("vtb", T * 256 // 2, np.uint32).view(np.uint16).copy()}


@pytest.fixture(scope="module")
def runs():
    from gisnav_amd.engine import PoseEngine
    sd, tsd, _ = _family("margin_built")
    pairs = _pairs("4x512")[0]
    sizes = _sizes(pairs)
    refs = [_ref_layer1(tsd, p) for p in pairs]
    rag = [make_pair(77100 + i, n_q=q, n_r=r) for i, (q, r) in enumerate(RAGGED)]
    eng = PoseEngine(0, max_batch=B4, max_kpts=K4, precision=HEADLINE, state_dict=sd)
    out = {"sizes": sizes}
    try:
        _forced_headline(eng, True)
        inp = eng.stage_inputs(pairs)
        assert eng.lib.gn_debug_set_variant(eng.ctx, 31, 3) == 0          # one workgroup per tile
        eng.set_ffn_products(2)
        out["two"] = _run(eng, inp)
        out["err2"] = _layer1_error(eng, inp, refs, sizes)
        eng.set_ffn_products(1)
        out["one"] = _run(eng, inp)
        out["err1"] = _layer1_error(eng, inp, refs, sizes)
        rinp = eng.stage_inputs(rag)
        out["rag"] = _run(eng, rinp)
        out["rag_alone"] = [_run(eng, eng.stage_inputs([p]), nb=1) for p in rag]
        assert eng.lib.gn_debug_set_variant(eng.ctx, 31, 2) == 0          # one workgroup per CU walking the list of tiles
        out["one_walk"] = _run(eng, inp)
    finally:
        _forced_headline(eng, False)
        eng.lib.gn_debug_set_variant(eng.ctx, 31, 1)
        del eng
    return out


def test_level1_error_against_fp64_is_at_most_twice_level2s(runs):
    e2, e1 = runs["err2"], runs["err1"]
    print(f"x after the first layer against fp64, 4 x 512, margin-built weights: level 2 {e2:.4e}, level 1 {e1:.4e}, ratio {e1 / e2:.3f}")
    _report("layer1_rel_error_vs_fp64_4x512_margin_built", {"level2": e2, "level1": e1, "ratio": e1 / e2})
    assert 0.0 < e2 < 1e-3, e2
    assert e1 <= 2.0 * e2, (e1, e2)


def test_all_eighteen_tail_launches_run_on_one_product(runs):
    for key, loop in (("one", "false"), ("one_walk", "true")):
        names = runs[key]["names"]
        assert len(names) == 18 and all(nm.rstrip(">").split(", ")[4] == "1" and nm.split(", ")[2] == loop for nm in names), names
        assert sorted({nm.split(", ")[3] for nm in names}) == ["0", "1", "2"], names       # the last tail has no projection behind it
    assert len(runs["two"]["names"]) == 18 and all(nm.rstrip(">").split(", ")[4] == "2" for nm in runs["two"]["names"]), runs["two"]["names"]
    # same matches as level 2 on these weights, scores within level 2's existing bound of level 3 (5e-3) doubled
    a, b = runs["two"], runs["one"]
    assert np.array_equal(a["n"], b["n"]) and all(np.array_equal(a["idx"][p, : a["n"][p]], b["idx"][p, : b["n"][p]]) for p in range(B4))
    assert int(a["n"].min()) > 0


def test_walking_form_gives_the_one_tile_forms_bits_in_x_and_in_the_fused_projection(runs):
    a, w, sizes = runs["one"], runs["one_walk"], runs["sizes"]
    assert np.array_equal(a["n"], w["n"])
    ba, bw = a["best"].reshape(B4, K4), w["best"].reshape(B4, K4)
    for p in range(B4):     # (valid rows: the head leaves the entries behind a pair's keypoint count as the previous call left them)
        k = int(a["n"][p])
        assert np.array_equal(ba[p, : sizes[p][0]].view(np.uint32), bw[p, : sizes[p][0]].view(np.uint32)), p
        assert np.array_equal(a["idx"][p, :k], w["idx"][p, :k]) and np.array_equal(a["score"][p, :k].view(np.uint32), w["score"][p, :k].view(np.uint32)), p
    xa, xw = a["x"].reshape(B4, 2, K4, 256), w["x"].reshape(B4, 2, K4, 256)
    qa, qw = a["qk"].reshape(B4, 2, K4, 256), w["qk"].reshape(B4, 2, K4, 256)
    va, vw = a["vt"].reshape(B4, 2, 4, 64, K4), w["vt"].reshape(B4, 2, 4, 64, K4)
    for p in range(B4):
        for s in (0, 1):
            n = sizes[p][s]
            assert np.array_equal(xa[p, s, :n].view(np.uint32), xw[p, s, :n].view(np.uint32)), (p, s)
            assert np.array_equal(qa[p, s, :n], qw[p, s, :n]) and qa[p, s, :n].any(), (p, s)
            n16 = n - n % 16          # (the panels hold the keys permuted inside groups of 16: whole groups of valid keys)
            assert np.array_equal(va[p, s, :, :, :n16], vw[p, s, :, :, :n16]) and va[p, s, :, :, :n16].any(), (p, s)


def test_ragged_batch_gives_the_bits_of_its_pairs_run_alone(runs):
    r = runs["rag"]
    x = r["x"].reshape(B4, 2, K4, 256)
    for p, alone in enumerate(runs["rag_alone"]):
        k = int(r["n"][p])
        assert k == int(alone["n"][0]), (p, k, alone["n"])
        assert np.array_equal(r["idx"][p, :k], alone["idx"][0, :k]) and np.array_equal(r["score"][p, :k].view(np.uint32), alone["score"][0, :k].view(np.uint32)), p
        assert np.array_equal(r["best"].reshape(B4, K4)[p, : RAGGED[p][0]].view(np.uint32), alone["best"][: RAGGED[p][0]].view(np.uint32)), p
        xa = alone["x"].reshape(1, 2, K4, 256)
        for s in (0, 1):
            assert np.array_equal(x[p, s, : RAGGED[p][s]].view(np.uint32), xa[0, s, : RAGGED[p][s]].view(np.uint32)), (p, s)
    assert all(nm.rstrip(">").split(", ")[4] == "1" for nm in r["names"]) and len(r["names"]) == 18, r["names"]


def _deciding_d(best, second, best_e, second_e, n_q, L):
    """max |P - P_f32| over best score and runner-up of the valid rows that come within 1 of L in either arithmetic (all rows when none does): what
    gn_calibrate_certify measures (max_diff in gn_api.hip)."""
    d_all = d_near = 0.0
    near = 0
    for b, n in enumerate(n_q):
        d = np.maximum(np.abs(best[b, :n].astype(np.float64) - best_e[b, :n]), np.abs(second[b, :n].astype(np.float64) - second_e[b, :n]))
        assert np.isfinite(d).all(), b
        d_all = max(d_all, float(d.max()))
        sel = np.maximum(best[b, :n], best_e[b, :n]) >= L - 1.0
        if sel.any():
            near += int(sel.sum())
            d_near = max(d_near, float(d[sel].max()))
    return d_near if near else d_all


@pytest.mark.parametrize("name", ["margin_built", "mid_margin", "default_init"])
def test_level1_certified_indices_equal_exact_f32_and_fresh_pairs_stay_within_eps_one(name):
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family(name)
    pairs, cal_pairs, B, K = _pairs("16x1024")
    n_q = [len(p.kp_q) for p in pairs]

    def match(e, inp):
        idx, score, n = e.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        torch.cuda.synchronize()
        return idx.cpu().numpy(), n.cpu().numpy(), e.debug_read("max0", B * K).reshape(B, K).copy(), e.debug_read("max0b", B * K).reshape(B, K).copy()

    ref = PoseEngine(0, max_batch=B, max_kpts=K, precision="f32", state_dict=sd, filter_threshold=th)
    idx_e, n_e, best_e, second_e = match(ref, ref.stage_inputs(pairs))
    del ref
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_ffn_products(1)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    inp = eng.stage_inputs(pairs)
    eng.set_certify("flag")
    eng.set_kernel_timing(400)
    _, _, best, second = match(eng, inp)                  # the fast pass alone: its scores, nothing re-run
    names = [r["name"] for r in eng.kernel_table() if r["name"].startswith("k_ffn128")]
    eng.set_kernel_timing(0)
    status = eng.fused_projection_status()
    d = _deciding_d(best, second, best_e, second_e, n_q, np.log(th) if th > 0 else -np.inf)
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    idx_c, n_c, _, _ = match(eng, inp)
    st = eng.certify_stats()
    del eng
    row = {"eps_one_product": cal["eps"], "measured_on_calibration_pairs": cal["measured"], "safety": SAFETY, "max_dP_fresh_pairs": d,
           "rerun_fraction": st["rerun_fraction"], "pairs": B}
    print(name, row)
    _report(f"certificate_level1_16x1024_{name}", row)
    assert names and all(nm.rstrip(">").split(", ")[4] == "1" for nm in names), names
    assert status == 1, status
    assert d <= cal["eps"], row
    assert np.array_equal(n_c, n_e), (n_c.tolist(), n_e.tolist(), row)
    assert all(np.array_equal(idx_c[b, : n_c[b]], idx_e[b, : n_e[b]]) for b in range(B)), row
    if name == "margin_built":
        assert st["rerun_pairs"] == 0, row


@pytest.mark.parametrize("name", ["margin_built", "mid_margin"])
def test_automatic_level_reaches_one_product_only_where_the_certificate_allows(name):
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family(name)
    pairs, cal_pairs, B, K = _pairs("16x1024")
    ref = PoseEngine(0, max_batch=B, max_kpts=K, precision="f32", state_dict=sd, filter_threshold=th)
    want = {k: v.clone() for k, v in ref.estimate(ref.stage_inputs(pairs), K_MATRIX).items()}
    torch.cuda.synchronize()
    del ref
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_ffn_products("auto")
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    assert cal["eps_one_product"] >= cal["eps_two_products"] >= cal["eps_three_products"] == cal["eps"] > 0.0, cal
    inp = eng.stage_inputs(pairs)
    eng.set_substreams(2)
    eng.set_certify("deferred")
    eng.certify_stats(reset=True)
    outs = [eng.alloc_outputs(B) for _ in range(12)]
    levels = []
    for i in range(12):
        levels.append(eng.ffn_level()["level"])
        eng.estimate(inp, K_MATRIX, out=outs[i])
    eng.flush()
    torch.cuda.synchronize()
    wrong = [sum(int(not torch.equal(o[k], want[k])) for k in ("n_match", "ok", "n_inliers", "R", "t")) for o in outs]
    eng.set_certify("rerun")
    eng.set_substreams(1)
    lv, st = eng.ffn_level(), eng.certify_stats()
    del eng
    row = {"levels_of_the_calls": levels, "level_after": lv["level"], "switches": lv["switches"], "calls_one_product": lv["calls_one_product"],
           "eps_one_product": cal["eps_one_product"], "eps_two_products": cal["eps_two_products"], "eps_three_products": cal["eps_three_products"],
           "eps_one_over_eps_two": cal["eps_one_product"] / cal["eps_two_products"], "rerun_pairs": st["rerun_pairs"], "mismatches_per_call": wrong}
    print(name, row)
    _report(f"automatic_level1_16x1024_{name}", row)
    assert lv["automatic"] and levels[0] == 3 and all(w == 0 for w in wrong), row
    if name == "margin_built":
        assert lv["level"] == 1 and lv["switches"] == 2 and st["rerun_pairs"] == 0, row
    else:
        assert lv["level"] == 3 and lv["switches"] == 0 and lv["calls_one_product"] == 0 and lv["calls_two_products"] == 0 and st["rerun_pairs"] > 0, row

"""GPU tests (-m gpu) of the two-product block tail's GELU (k_ffn128<., ., ., ., 2>: erf as a degree-4 polynomial inside exp2, tools/erf_fit.py).

2 pairs of 256 / 256 and 256 / 250 keypoints on a 2 x 256 context: 1024 token slots = 8 tiles of 128, one of them partly padding; the bulk kernels are
forced as in test_gpu_round5.py (knobs 14 = 128, 1 = 70, 19 = 2, 27 = 2).  One context, every run made once (module fixture):

  * level 2 against level 3 in the same context: only `..., 2>` tail instantiations in the launch table, the best assignment score of every row
    within 5e-3 (the bound of test_two_product_block_tail_is_repeatable_and_close_to_the_three_product_form), identical correspondence indices, two
    runs bit-identical, the walking form (knob 31 = 2) bit-identical to the one-tile form (knob 31 = 3);
  * against fp64 (oracle.lightglue_sift, the stage helpers of test_gpu_fp64_parity.py): the relative error of the residual stream x after the first
    layer on level 2 must not exceed 1.25 x what the PARENT build's level 2 (degree-7 erf, 2.2e-8) left on the same inputs -- measured once with the
    parent library and kept in tests/golden/erf_level2_parent.json with that library's digest.  Two independent errors of ratio <= 1/2 add in
    quadrature to <= 1.12; 1.25 leaves room for the f32 evaluation.  (The approximation's own error is <= 2^-21 |y| against the level's fp16
    rounding of 2^-12 |h|: tests/test_erf_level2_host.py.)
"""
import json
import os

import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import make_pair
from gisnav_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "erf_level2_parent.json")
HEADLINE = "f16x2_f16_attn"
B, K = 2, 256
SIZES = ((256, 256), (256, 250))
KNOBS = ((14, 128), (1, 70), (19, 2), (27, 2))
DEFAULTS = ((14, 0), (1, 4), (19, 1), (27, 2), (31, 1))


def pairs():
    return [make_pair(13100 + i, n_q=q, n_r=r) for i, (q, r) in enumerate(SIZES)]


def _ref_layer1(sd, p):
    """fp64 residual stream of both sides after the first layer."""
    from oracle import lightglue_sift as lg
    tsd = {n: torch.from_numpy(v) for n, v in sd.items()}
    taps = {}
    tq = torch.from_numpy
    lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r), tq(p.angle_r),
                       taps=taps, filter_threshold=0.5, dtype=torch.float64)
    return taps["layer0_0"][0].numpy(), taps["layer0_1"][0].numpy()


def layer1_error(eng, inp, refs):
    """max over pairs and sides of max |x - x64| / max |x64| over the valid rows, after one layer (the measure of test_gpu_fp64_parity._layer_errors)."""
    eng.set_num_layers(1)
    eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    eng.set_num_layers(9)
    x = eng.debug_read("x", B * 2 * K * 256).reshape(B, 2, K, 256)
    err = 0.0
    for b, ref in enumerate(refs):
        for s in (0, 1):
            n = SIZES[b][s]
            a = x[b, s, :n]
            assert np.isfinite(a).all(), (b, s)
            err = max(err, float(np.abs(a - ref[s]).max() / np.abs(ref[s]).max()))
    return err


def _run(eng, inp):
    eng.set_kernel_timing(400)
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table() if r["name"].startswith("k_ffn128")]
    eng.set_kernel_timing(0)
    return {"idx": idx.cpu().numpy().copy(), "score": score.cpu().numpy().copy(), "n": n.cpu().numpy().copy(), "names": names,
            "best": eng.debug_read("max0", B * K).copy(), "x": eng.debug_read("x", B * 2 * K * 256).copy()}


@pytest.fixture(scope="module")
def runs():
    from gisnav_amd.engine import PoseEngine
    sd = synthetic_state_dict(0)
    ps = pairs()
    refs = [_ref_layer1(sd, p) for p in ps]
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd)
    out = {}
    try:
        for k, v in KNOBS:
            assert eng.lib.gn_debug_set_variant(eng.ctx, k, v) == 0
        inp = eng.stage_inputs(ps)
        assert eng.lib.gn_debug_set_variant(eng.ctx, 31, 3) == 0          # one workgroup per tile
        eng.set_ffn_products(3)
        out["three"] = _run(eng, inp)
        out["err3"] = layer1_error(eng, inp, refs)
        eng.set_ffn_products(2)
        out["two_a"] = _run(eng, inp)
        out["two_b"] = _run(eng, inp)
        out["err2"] = layer1_error(eng, inp, refs)
        assert eng.lib.gn_debug_set_variant(eng.ctx, 31, 2) == 0          # one workgroup per CU walking the list of tiles
        out["two_walk"] = _run(eng, inp)
    finally:
        for k, v in DEFAULTS:
            eng.lib.gn_debug_set_variant(eng.ctx, k, v)
        del eng
    return out


def test_only_two_product_tails_run_and_the_walking_form_is_selected_when_asked(runs):
    for key in ("two_a", "two_b", "two_walk"):
        names = runs[key]["names"]
        assert len(names) >= 2 and all(nm.rstrip(">").split(", ")[4] == "2" for nm in names), names
    assert all(nm.split(", ")[2] == "false" for nm in runs["two_a"]["names"]), runs["two_a"]["names"]
    assert all(nm.split(", ")[2] == "true" for nm in runs["two_walk"]["names"]), runs["two_walk"]["names"]
    assert all(nm.rstrip(">").split(", ")[4] == "3" for nm in runs["three"]["names"]), runs["three"]["names"]


def test_level2_scores_stay_within_the_existing_bound_of_level3_with_identical_indices(runs):
    a, b = runs["three"], runs["two_a"]
    valid = np.concatenate([np.arange(K * p, K * p + SIZES[p][0]) for p in range(B)])
    d = float(np.abs(a["best"][valid] - b["best"][valid]).max())
    print("level 2 against level 3: max |d best score| =", d)
    assert np.isfinite(b["best"][valid]).all()
    assert 0.0 < d < 5e-3, d
    assert np.array_equal(a["n"], b["n"]) and all(np.array_equal(a["idx"][p, : a["n"][p]], b["idx"][p, : b["n"][p]]) for p in range(B))
    assert int(a["n"].min()) > 0


def test_level2_is_repeatable_and_the_walking_form_gives_the_one_tile_forms_bits(runs):
    a, b, w = runs["two_a"], runs["two_b"], runs["two_walk"]
    for other in (b, w):
        assert np.array_equal(a["best"].view(np.uint32), other["best"].view(np.uint32))
        assert np.array_equal(a["idx"], other["idx"]) and np.array_equal(a["n"], other["n"])
        assert np.array_equal(a["score"].view(np.uint32), other["score"].view(np.uint32))
        # the residual stream behind the last block, valid rows of every side (padding rows of a partly filled tile are defined but unspecified)
        xa, xo = a["x"].reshape(B, 2, K, 256), other["x"].reshape(B, 2, K, 256)
        for p in range(B):
            for s in (0, 1):
                assert np.array_equal(xa[p, s, : SIZES[p][s]].view(np.uint32), xo[p, s, : SIZES[p][s]].view(np.uint32)), (p, s)


def test_level2_error_against_fp64_is_no_larger_than_the_parents(runs):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["sizes"] == [list(s) for s in SIZES] and gold["pair_seed"] == 13100, gold
    parent = float(gold["level2_layer1_rel_error"])
    print(f"level-2 error of x after the first layer against fp64: {runs['err2']:.4e} (parent build {gold['library_digest']}: {parent:.4e}; level 3 here: {runs['err3']:.4e})")
    assert 0.0 < parent < 1e-3, gold
    assert runs["err2"] <= 1.25 * parent, (runs["err2"], parent)

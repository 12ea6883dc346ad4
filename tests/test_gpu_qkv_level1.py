"""GPU tests (-m gpu) of the attention input projections on one fp16 product (W_h X_h): k_qkv<., true, 1>, the fused forms k_ffn128<., ., ., 3 / 4, 1>
and the rung they add to the automatic ladder below level 1 (set_qkv_products).

  * bits, 4 x 512 with the bulk kernels forced (test_gpu_round6._forced_headline), block tail on level 1, one context (module fixture; max_batch 32, so that
    the context proves the fused forms on its own weights):
      - on weights whose projection matrices are exact in fp16 (the W_m plane of their fragments is all zeros) k_qkv<., true, 2> computes W_h X_h + 0: the
        one-product kernels must give its q | k rows and V^T panels bit for bit, self and cross, and -- the projections being equal -- the whole call must
        equal today's level 1 in x, q | k, V^T, indices and scores, fused and separate, one-tile and walking;
      - on the margin-built weights the fused forms give the bits of tail level 1 + k_qkv<., true, 1> launched separately, one-tile and walking;
  * a ragged batch (sides of 2 and of 130 keypoints) gives the bits of its pairs run alone on the rung;
  * error: the cross block's qk rows behind the first self block against fp64 -- one more rounding of the weights of the size of the output rounding the rows
    carry anyway: sqrt 2 predicted, at most 2.0 x the two-product projections' error asserted (the level-1 test's bound for the same argument);
  * the range guard on the rung (q x 1e6 in every Wqkv, tests/test_gpu_bulk_guard.py's case);
  * certificate, 16 x 1024, rung fixed (set_ffn_products(1) + set_qkv_products(1)), the three weight families;
  * automatic: 16 calls of 16 margin-built pairs end on the rung with three switches and no re-run; mid-margin weights never leave three products.
"""
import json
import os

import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import K_MATRIX, make_pair
from tests.test_gpu_bulk_guard import _close_to_oracle, _weights
from tests.test_gpu_ffn_level1 import RAGGED, _deciding_d, _sizes
from tests.test_gpu_round6 import HEADLINE, SAFETY, _family, _forced_headline, _pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B4, K4 = 4, 512
T4 = B4 * 2 * K4


def _report(key, value):
    path = os.path.join(ROOT, "test_reports", "qkv_level1_tests.json")      # (git-ignored, as tests/test_gpu_ffn_level1.py's report)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _fp16_exact_projections(sd):
    """The same weights with every attention input projection matrix rounded to fp16: the hm16 split of such a matrix has an all-zero W_m plane (the split's
    scale is a power of two), so the two-product kernels compute W_h X_h + 0 on it."""
    out = dict(sd)
    n = 0
    for k, v in sd.items():
        if k.endswith(("Wqkv.weight", "to_qk.weight", "to_v.weight")):
            out[k] = v.astype(np.float16).astype(np.float32)
            n += 1
    assert n == 27, n
    return out


def _run(eng, inp, nb=B4):
    eng.set_kernel_timing(400)
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table() for _ in range(int(r["launches"])) if r["name"].startswith(("k_ffn128", "k_qkv"))]
    eng.set_kernel_timing(0)
    T = nb * 2 * K4
    # qk: the whole q | k buffer, rows of 512 fp16 as the self projections write them; a cross projection (the last of every call) writes rows of 256 into its
    # first half, so the second half still holds the LAST SELF projection's rows of the tokens T / 2 .. T - 1
    return {"idx": idx.cpu().numpy().copy(), "score": score.cpu().numpy().copy(), "n": n.cpu().numpy().copy(), "names": names,
            "best": eng.debug_read("max0", nb * K4).copy(), "x": eng.debug_read("x", T * 256).copy(),
            "qk": eng.debug_read("qkb", T * 256, np.uint32).view(np.uint16).copy(), "vt": eng.debug_read("vtb", T * 256 // 2, np.uint32).view(np.uint16).copy()}


def _same_call(a, b, sizes, what, x=True):
    """Bit equality of two runs over everything valid tokens wrote: indices, scores, best row scores, x rows, the last cross projection's qk rows and V^T
    panels, and the last self projection's q | k rows of the second half of the batch."""
    assert np.array_equal(a["n"], b["n"]), (what, a["n"], b["n"])
    ba, bb = a["best"].reshape(B4, K4), b["best"].reshape(B4, K4)
    xa, xb = a["x"].reshape(B4, 2, K4, 256), b["x"].reshape(B4, 2, K4, 256)
    ca, cb = a["qk"][: T4 * 256].reshape(B4, 2, K4, 256), b["qk"][: T4 * 256].reshape(B4, 2, K4, 256)
    sa, sb = a["qk"][T4 * 256:].reshape(B4 // 2, 2, K4, 512), b["qk"][T4 * 256:].reshape(B4 // 2, 2, K4, 512)
    va, vb = a["vt"].reshape(B4, 2, 4, 64, K4), b["vt"].reshape(B4, 2, 4, 64, K4)
    for p in range(B4):
        k = int(a["n"][p])
        assert np.array_equal(a["idx"][p, :k], b["idx"][p, :k]) and np.array_equal(a["score"][p, :k].view(np.uint32), b["score"][p, :k].view(np.uint32)), (what, p)
        assert np.array_equal(ba[p, : sizes[p][0]].view(np.uint32), bb[p, : sizes[p][0]].view(np.uint32)), (what, p)
        for s in (0, 1):
            n = sizes[p][s]
            if x:
                assert np.array_equal(xa[p, s, :n].view(np.uint32), xb[p, s, :n].view(np.uint32)), (what, "x", p, s)
            assert np.array_equal(ca[p, s, :n], cb[p, s, :n]) and ca[p, s, :n].any(), (what, "qk", p, s)
            n16 = n - n % 16          # (the panels hold the keys permuted inside groups of 16: whole groups of valid keys)
            assert np.array_equal(va[p, s, :, :, :n16], vb[p, s, :, :, :n16]) and va[p, s, :, :, :n16].any(), (what, "vt", p, s)
            if p >= B4 // 2:
                q = p - B4 // 2
                assert np.array_equal(sa[q, s, :n], sb[q, s, :n]) and sa[q, s, :n].any(), (what, "self q | k", p, s)


def _knob(eng, which, value):
    assert eng.lib.gn_debug_set_variant(eng.ctx, which, value) == 0, (which, value)


def _ref_qk(tsd, p):
    """fp64: the cross block's qk rows of both sides behind the first self block (to_qk x * d_head^-0.25)."""
    from oracle import lightglue_sift as lg
    taps = {}
    tq = torch.from_numpy
    dsd = {k: v.double() for k, v in tsd.items()}
    lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r), tq(p.angle_r),
                       taps=taps, filter_threshold=0.5, dtype=torch.float64)
    w, b = dsd["transformers.0.cross_attn.to_qk.weight"], dsd["transformers.0.cross_attn.to_qk.bias"]
    return [((taps[f"self0_{s}"][0].double() @ w.T + b) * 64.0 ** -0.25).numpy() for s in (0, 1)]


def _qk_error(eng, inp, refs, sizes):
    eng.set_num_layers(1)
    r = _run(eng, inp)
    eng.set_num_layers(9)
    qk = r["qk"][: T4 * 256].view(np.float16).astype(np.float64).reshape(B4, 2, K4, 256)
    err = 0.0
    for b, ref in enumerate(refs):
        for s in (0, 1):
            a = qk[b, s, : sizes[b][s]]
            assert np.isfinite(a).all(), (b, s)
            err = max(err, float(np.abs(a - ref[s]).max() / np.abs(ref[s]).max()))
    return err, r["names"]


@pytest.fixture(scope="module")
def runs():
    from gisnav_amd.engine import PoseEngine
    sd, tsd, _ = _family("margin_built")
    pairs = _pairs("4x512")[0]
    sizes = _sizes(pairs)
    refs = [_ref_qk(tsd, p) for p in pairs]
    rag = [make_pair(77100 + i, n_q=q, n_r=r) for i, (q, r) in enumerate(RAGGED)]
    eng = PoseEngine(0, max_batch=32, max_kpts=K4, precision=HEADLINE, state_dict=_fp16_exact_projections(sd))
    out = {"sizes": sizes}
    try:
        _forced_headline(eng, True)
        inp = eng.stage_inputs(pairs)
        _knob(eng, 31, 3)                   # one workgroup per tile
        eng.set_ffn_products(1)
        # ---- fp16-exact projection weights: one product against two products + a zero W_m plane
        for setting, key in ((2, "exact_two"), (1, "exact_one")):
            eng.set_qkv_products(setting)
            out[key] = _run(eng, inp)                       # fused (the default)
            _knob(eng, 32, 0)
            out[key + "_sep"] = _run(eng, inp)              # every projection a k_qkv launch
            eng.set_num_layers(1)
            out[key + "_sep_l1"] = _run(eng, inp)           # ... and one layer: the first self and cross projections' own outputs
            eng.set_num_layers(9)
            _knob(eng, 32, 1)
        _knob(eng, 31, 2)                   # one workgroup per CU walking the list of tiles
        out["exact_one_walk"] = _run(eng, inp)
        _knob(eng, 31, 3)
        # ---- margin-built weights
        eng.load_state_dict(sd)
        eng.set_qkv_products(2)
        out["err2"], out["names2_l1"] = _qk_error(eng, inp, refs, sizes)
        eng.set_qkv_products(1)
        out["err1"], out["names1_l1"] = _qk_error(eng, inp, refs, sizes)
        out["one"] = _run(eng, inp)
        out["status"] = eng.fused_projection_status()
        out["level"] = eng.ffn_level()
        _knob(eng, 32, 0)
        out["one_sep"] = _run(eng, inp)
        _knob(eng, 32, 1)
        rinp = eng.stage_inputs(rag)
        out["rag"] = _run(eng, rinp)
        out["rag_alone"] = [_run(eng, eng.stage_inputs([p]), nb=1) for p in rag]
        _knob(eng, 31, 2)
        out["one_walk"] = _run(eng, inp)
    finally:
        _forced_headline(eng, False)
        eng.lib.gn_debug_set_variant(eng.ctx, 31, 1)
        eng.lib.gn_debug_set_variant(eng.ctx, 32, 1)
        del eng
    return out


def _tails(names):
    return [nm for nm in names if nm.startswith("k_ffn128")]


def test_one_product_k_qkv_gives_the_bits_of_two_products_on_a_zero_w_m_plane(runs):
    for key in ("_sep_l1", "_sep"):
        a, b = runs["exact_two" + key], runs["exact_one" + key]
        qa, qb = [nm for nm in a["names"] if nm.startswith("k_qkv")], [nm for nm in b["names"] if nm.startswith("k_qkv")]
        assert len(qa) == len(qb) == (2 if key == "_sep_l1" else 18), (qa, qb)
        assert sorted(set(qa)) == ["k_qkv<false, true, 2>", "k_qkv<true, true, 2>"] and sorted(set(qb)) == ["k_qkv<false, true, 1>", "k_qkv<true, true, 1>"], (qa, qb)
        assert all(nm.rstrip(">").split(", ")[3:] == ["0", "1"] for nm in _tails(a["names"]) + _tails(b["names"])), (a["names"], b["names"])
        _same_call(a, b, runs["sizes"], "k_qkv one product against two products on a zero W_m plane" + key)


def test_fused_forms_give_the_bits_of_the_separate_launches_and_x_equals_todays_level_one(runs):
    sizes = runs["sizes"]
    for key, loop in (("exact_one", "false"), ("exact_one_walk", "true"), ("one", "false"), ("one_walk", "true")):
        names = runs[key]["names"]
        tails = _tails(names)
        assert len(tails) == 18 and all(nm.split(", ")[2] == loop and nm.rstrip(">").split(", ")[4] == "1" for nm in tails), names
        assert sorted(nm.split(", ")[3] for nm in tails) == ["0"] + ["3"] * 8 + ["4"] * 9, names      # the last tail has no projection behind it
        assert [nm for nm in names if nm.startswith("k_qkv")] == ["k_qkv<false, true, 1>"], names      # the first block's projection
    two = _tails(runs["exact_two"]["names"])
    assert sorted(nm.split(", ")[3] for nm in two) == ["0"] + ["1"] * 8 + ["2"] * 9, two
    # fp16-exact projection weights: the rung IS today's level 1 -- every x row, fused or separate, one-tile or walking
    for key in ("exact_two_sep", "exact_one", "exact_one_sep", "exact_one_walk"):
        _same_call(runs["exact_two"], runs[key], sizes, "today's level 1 against " + key)
    # margin-built weights: the fused forms against tail level 1 + k_qkv<., true, 1>
    assert all(nm.rstrip(">").split(", ")[3:] == ["0", "1"] for nm in _tails(runs["one_sep"]["names"])), runs["one_sep"]["names"]
    assert sum(nm in ("k_qkv<false, true, 1>", "k_qkv<true, true, 1>") for nm in runs["one_sep"]["names"]) == 18, runs["one_sep"]["names"]
    _same_call(runs["one"], runs["one_sep"], sizes, "fused against separate")
    _same_call(runs["one"], runs["one_walk"], sizes, "one-tile against walking")
    assert int(runs["one"]["n"].min()) > 0
    assert runs["status"] == 1, runs["status"]
    assert runs["level"]["level"] == 1 and runs["level"]["projection_one_product"] and not runs["level"]["automatic"], runs["level"]


def test_ragged_batch_gives_the_bits_of_its_pairs_run_alone_on_the_rung(runs):
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
    tails = _tails(r["names"])
    assert len(tails) == 18 and sorted(nm.rstrip(">").split(", ")[3] + nm.rstrip(">").split(", ")[4] for nm in tails) == ["01"] + ["31"] * 8 + ["41"] * 9, r["names"]
    assert runs["status"] == 1, runs["status"]


def test_projection_error_against_fp64_is_at_most_twice_the_two_product_projections(runs):
    e2, e1 = runs["err2"], runs["err1"]
    print(f"cross qk rows behind the first self block against fp64, 4 x 512, margin-built weights: two products {e2:.4e}, one product {e1:.4e}, ratio {e1 / e2:.3f}")
    _report("qk_rel_error_vs_fp64_4x512_margin_built", {"two_products": e2, "one_product": e1, "ratio": e1 / e2})
    assert "k_qkv<false, true, 2>" in runs["names2_l1"] and "k_ffn128<0, true, false, 2, 1>" in runs["names2_l1"], runs["names2_l1"]
    assert "k_qkv<false, true, 1>" in runs["names1_l1"] and "k_ffn128<0, true, false, 4, 1>" in runs["names1_l1"], runs["names1_l1"]
    assert 0.0 < e2 < 1e-2, e2
    assert e1 <= 2.0 * e2, (e1, e2)


class _Rung:
    """A 4 x 512 fp16-attention context on the bulk kernels, tail on level 1, projections on one product (the knobs are put back when it goes)."""

    def __init__(self, sd, guard="flag"):
        from gisnav_amd.engine import PoseEngine
        self.eng = PoseEngine(0, max_batch=B4, max_kpts=K4, precision=HEADLINE, state_dict=sd, guard=guard)

    def __enter__(self):
        _forced_headline(self.eng, True)
        self.eng.set_ffn_products(1)
        self.eng.set_qkv_products(1)
        return self.eng

    def __exit__(self, *exc):
        _forced_headline(self.eng, False)
        del self.eng


def _guard_pairs():
    from tests.test_gpu_bulk_guard import _pairs as guard_pairs
    return guard_pairs()


def _on_rung(names):
    tails = _tails(names)
    assert tails and any(nm.endswith(", 3, 1>") for nm in tails) and any(nm.endswith(", 4, 1>") for nm in tails), names
    assert not any(nm.endswith((", 1, 1>", ", 2, 1>")) for nm in tails) and "k_qkv<false, true, 1>" in names, names


def test_range_guard_on_the_rung_flag_reports_no_match_and_the_context_recovers():
    pairs = _guard_pairs()
    with _Rung(_weights("qk")) as eng:
        inp = eng.stage_inputs(pairs)
        r = _run(eng, inp)
        _on_rung(r["names"])
        assert eng.guard_status()[0], r["n"].tolist()
        assert (r["n"] == 0).all(), r["n"]
        out = eng.estimate(inp, K_MATRIX)
        torch.cuda.synchronize()
        assert eng.guard_status()[0]
        assert (out["ok"].cpu().numpy() == 0).all() and (out["n_match"].cpu().numpy() == 0).all(), (out["ok"], out["n_match"])
        eng.load_state_dict(_weights("plain"))
        again = _run(eng, inp)
        assert not eng.guard_status()[0]
        _on_rung(again["names"])
    with _Rung(_weights("plain")) as eng:
        fresh = _run(eng, eng.stage_inputs(pairs))
        assert eng.guard_status() == (False, 0)
    assert np.array_equal(again["n"], fresh["n"]) and int(fresh["n"].min()) > 50, (again["n"], fresh["n"])
    for p in range(B4):
        k = int(fresh["n"][p])
        assert np.array_equal(again["idx"][p, :k], fresh["idx"][p, :k]) and np.array_equal(again["score"][p, :k].view(np.uint32), fresh["score"][p, :k].view(np.uint32)), p
    _close_to_oracle(fresh["idx"], fresh["n"], "plain")


def test_range_guard_on_the_rung_sync_counts_one_fallback():
    with _Rung(_weights("qk"), guard="sync") as eng:
        r = _run(eng, eng.stage_inputs(_guard_pairs()))
        st = eng.guard_status()
    assert any(nm.endswith(", 3, 1>") for nm in r["names"]) and "k_qkv<false, true, 1>" in r["names"], r["names"]
    _close_to_oracle(r["idx"], r["n"], "qk")
    assert st[1] == 1, st


def test_certificate_on_the_rung_flags_every_pair_of_a_call_that_left_the_fp16_range():
    pairs = _guard_pairs()
    qk = _weights("qk")
    from gisnav_amd.engine import PoseEngine
    e32 = PoseEngine(0, max_batch=B4, max_kpts=K4, precision="f32", state_dict=qk)
    want = _run(e32, e32.stage_inputs(pairs))
    del e32
    _close_to_oracle(want["idx"], want["n"], "qk")
    with _Rung(_weights("plain")) as eng:
        cal = eng.calibrate_certify(eng.stage_inputs([make_pair(77260 + i, n_q=500, n_r=490) for i in range(B4)]), safety=SAFETY)
        assert 0.0 < cal["eps"] < 0.1, cal
        inp = eng.stage_inputs(pairs)
        eng.load_state_dict(qk)
        eng.set_certify("flag", eps=cal["eps"])
        r = _run(eng, inp)
        _on_rung(r["names"])
        assert eng.guard_status()[0]
        flags = eng.uncertain(B4)
        assert (flags == 2).all(), flags.tolist()
        assert (r["n"] == 0).all(), r["n"]
        eng.set_certify("rerun", eps=cal["eps"])
        eng.certify_stats(reset=True)
        got = _run(eng, inp)
        st = eng.certify_stats()
    assert st["pairs"] == B4 and st["flagged_fp16_range"] == B4 and st["rerun_pairs"] == B4, st
    assert np.array_equal(got["n"], want["n"]) and all(np.array_equal(got["idx"][p, : got["n"][p]], want["idx"][p, : want["n"][p]]) for p in range(B4)), (got["n"], want["n"])


@pytest.mark.parametrize("name", ["margin_built", "mid_margin", "default_init"])
def test_rung_certified_indices_equal_exact_f32_and_fresh_pairs_stay_within_its_eps(name):
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
    eng.set_qkv_products(1)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    inp = eng.stage_inputs(pairs)
    eng.set_certify("flag")
    eng.set_kernel_timing(400)
    _, _, best, second = match(eng, inp)                  # the fast pass alone: its scores, nothing re-run
    names = [r["name"] for r in eng.kernel_table() if r["name"].startswith(("k_ffn128", "k_qkv"))]
    eng.set_kernel_timing(0)
    status = eng.fused_projection_status()
    d = _deciding_d(best, second, best_e, second_e, n_q, np.log(th) if th > 0 else -np.inf)
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    idx_c, n_c, _, _ = match(eng, inp)
    st = eng.certify_stats()
    del eng
    row = {"eps_one_product_projection": cal["eps"], "measured_on_calibration_pairs": cal["measured"], "safety": SAFETY, "max_dP_fresh_pairs": d,
           "rerun_fraction": st["rerun_fraction"], "pairs": B}
    print(name, row)
    _report(f"certificate_rung_16x1024_{name}", row)
    tails = _tails(names)
    assert tails and all(nm.endswith((", 3, 1>", ", 4, 1>", ", 0, 1>")) for nm in tails) and sum(nm.endswith(", 0, 1>") for nm in tails) == 1, names
    assert [nm for nm in names if nm.startswith("k_qkv")] == ["k_qkv<false, true, 1>"], names
    assert status == 1, status
    assert d <= cal["eps"], row
    assert np.array_equal(n_c, n_e), (n_c.tolist(), n_e.tolist(), row)
    assert all(np.array_equal(idx_c[b, : n_c[b]], idx_e[b, : n_e[b]]) for b in range(B)), row
    if name == "margin_built":
        assert st["rerun_pairs"] == 0, row


@pytest.mark.parametrize("name", ["margin_built", "mid_margin"])
def test_automatic_ladder_reaches_the_rung_only_where_the_certificate_allows(name):
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
    assert cal["eps_one_product_projection"] >= cal["eps_one_product"] >= cal["eps_two_products"] >= cal["eps_three_products"] == cal["eps"] > 0.0, cal
    inp = eng.stage_inputs(pairs)
    eng.set_substreams(2)
    eng.set_certify("deferred")
    eng.certify_stats(reset=True)
    outs = [eng.alloc_outputs(B) for _ in range(16)]
    levels, rung = [], []
    for i in range(16):
        lv = eng.ffn_level()
        levels.append(lv["level"])
        rung.append(int(lv["projection_one_product"]))
        eng.estimate(inp, K_MATRIX, out=outs[i])
    eng.flush()
    torch.cuda.synchronize()
    wrong = [sum(int(not torch.equal(o[k], want[k])) for k in ("n_match", "ok", "n_inliers", "R", "t")) for o in outs]
    eng.set_certify("rerun")
    eng.set_substreams(1)
    lv, st = eng.ffn_level(), eng.certify_stats()
    del eng
    row = {"levels_of_the_calls": levels, "rung_of_the_calls": rung, "level_after": lv["level"], "on_the_rung_after": lv["projection_one_product"], "switches": lv["switches"],
           "calls_one_product": lv["calls_one_product"], "calls_projection_one_product": lv["calls_projection_one_product"],
           "eps_one_product_projection": cal["eps_one_product_projection"], "eps_one_product": cal["eps_one_product"], "eps_two_products": cal["eps_two_products"],
           "eps_three_products": cal["eps_three_products"], "eps_proj1_over_eps_one": cal["eps_one_product_projection"] / cal["eps_one_product"],
           "rerun_pairs": st["rerun_pairs"], "mismatches_per_call": wrong}
    print(name, row)
    _report(f"automatic_rung_16x1024_{name}", row)
    assert lv["automatic"] and levels[0] == 3 and all(w == 0 for w in wrong), row
    if name == "margin_built":
        assert lv["level"] == 1 and lv["projection_one_product"] and lv["switches"] == 3 and st["rerun_pairs"] == 0, row
    else:
        assert lv["level"] == 3 and not lv["projection_one_product"] and lv["switches"] == 0 and lv["calls_one_product"] == 0 and lv["calls_two_products"] == 0 \
            and lv["calls_projection_one_product"] == 0 and st["rerun_pairs"] > 0, row

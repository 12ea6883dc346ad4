"""Sub-batch groups and the certificate's in-place re-run work on VIEWS of the per-pair workspaces (csrc/gn_api.hip: Workspace, view_of).  One f16x2
engine where every condition that changes a view's offsets holds at once: max_batch 7 at max_kpts 384 with the active size at 256 (slices step by
npad_run, the match lists and PnP masks by gn_kmax), two sub-streams (groups of 4 and 3 pairs: uneven, neither small enough for the one- or
two-pair kernels), report=True (the caller's match lists), and a re-run in exact f32 from a non-zero first pair.

The margin certificate and point pruning refuse each other (gn_set_certify / gn_set_width_pruning, tests/test_gpu_width_pruning.py::test_g_edges),
so the product is covered by two tests on the same shapes: the certificate's re-run with pruning off (gn_get_prune then reports n_layers for every
keypoint, from the same per-call state), and pruning on with the certificate off.  Every expected value is the SAME engine's ungrouped call;
everything is compared bit for bit.  score[:n_match]: reproduced between grouped and ungrouped calls by the commit before the views, so asserted."""
import numpy as np
import pytest
import torch

from gisnav_amd.engine import PoseEngine
from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

B, KPTS, ACTIVE, NL = 7, 384, 256, 9
EPS = 1.0e-7           # stated: no decision of these pairs lies this close to flipping (asserted from certify_stats below)
WC, MINK = 0.99, 100   # point pruning as tests/test_gpu_width_pruning.py sets it up
TAU = float(np.log((1.0 - WC) / WC))      # a row is kept while sigmoid(z) > 1 - width_confidence


def _pairs():
    return [make_pair(8800 + i, n_q=256 - 8 * i, n_r=200 + 9 * i) for i in range(B)]      # 200..256 keypoints per side


def _engine(sd):
    eng = PoseEngine(0, max_batch=B, max_kpts=KPTS, precision="f16x2_f16_attn", state_dict=sd)
    assert eng.kmax == KPTS and eng.set_active_kpts(ACTIVE) == ACTIVE
    return eng


def _call(eng, inp):
    """One estimate(report=True) and everything the context keeps of it, on the host."""
    out = eng.alloc_outputs(B, report=True)
    for v in out.values():
        v.zero_()
    eng.estimate(inp, K_MATRIX, out=out, report=True)
    eng.flush()
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o["prune0"], o["prune1"] = eng.last_prune(B)
    o["niters"], o["evaluated"] = eng.ransac_last_counts(B)
    return o


def _assert_pairs_equal(got, want, pairs, what, counts=True):
    for b in pairs:
        k = int(want["n_match"][b])
        for name in ("R", "t", "n_match", "n_inliers", "ok", "prune0", "prune1") + (("niters", "evaluated") if counts else ()):
            assert np.array_equal(got[name][b], want[name][b]), (what, b, name)
        assert np.array_equal(got["idx"][b, :k], want["idx"][b, :k]), (what, b, "idx")
        assert np.array_equal(got["inlier_mask"][b, :k], want["inlier_mask"][b, :k]), (what, b, "inlier_mask")
        assert np.array_equal(got["score"][b, :k].view(np.uint32), want["score"][b, :k].view(np.uint32)), (what, b, "score")


def test_a_tripped_group_is_rerun_in_place_from_its_first_pair():
    eng = _engine(synthetic_state_dict(0))
    inp = eng.stage_inputs(_pairs())
    eng.set_certify("rerun", eps=EPS)
    knob = lambda v: eng.lib.gn_debug_set_variant(eng.ctx, 25, v)  # noqa: E731
    try:
        eng.set_substreams(1)
        eng.certify_stats(reset=True)
        plain = _call(eng, inp)                                   # ungrouped, untripped: the f16x2 arithmetic
        st = eng.certify_stats(reset=True)
        assert st["pairs"] == B and st["flagged_margin"] == 0 and st["flagged_fp16_range"] == 0 and st["rerun_pairs"] == 0, st
        assert (plain["n_match"] > 30).all() and plain["ok"].all()
        assert knob(1) == 0                                        # the call's one guard word raised: every pair again in exact f32
        exact = _call(eng, inp)
        st = eng.certify_stats(reset=True)
        assert st["flagged_margin"] == 0 and st["flagged_fp16_range"] == B and st["rerun_pairs"] == B, st
        eng.set_substreams(2)
        assert knob(2) == 0                                        # group 1 (pairs 4..6) raised: re-run in place from pair 4
        got = _call(eng, inp)
        st = eng.certify_stats(reset=True)
        assert st["flagged_margin"] == 0 and st["flagged_fp16_range"] == 3 and st["rerun_pairs"] == 3, st
    finally:
        knob(0)
        eng.set_substreams(1)
    _assert_pairs_equal(got, plain, range(0, 4), "group 0")
    # (gn_ransac_last_counts folds the hypotheses with the match counts of the stage it recorded -- that of the pairs from 0 on, where the tripped
    #  group had no match: the counts of a re-run from a later first pair are not the re-run's own, before and after the views)
    _assert_pairs_equal(got, exact, range(4, 7), "group 1, exact f32", counts=False)
    assert all((got["prune0"][b, :256 - 8 * b] == NL).all() for b in range(B))      # pruning off: every keypoint in every layer


def test_b_pruned_groups_equal_the_ungrouped_call():
    sd = synthetic_state_dict(0)
    eng = _engine(sd)
    pairs = _pairs()
    inp = eng.stage_inputs(pairs)
    eng.set_certify("off")
    eng.set_width_pruning(WC, MINK)
    # the last pruning layer's bias moved so that its threshold is the median z of the call's valid rows: about half of every side leaves there
    _call(eng, inp)
    z = eng.debug_read("prune_z", 2 * B * ACTIVE).reshape(B, 2, ACTIVE)
    valid = np.concatenate([z[b, s, :n] for b, p in enumerate(pairs) for s, n in ((0, len(p.kp_q)), (1, len(p.kp_r)))])
    name = f"log_assignment.{NL - 2}.matchability.bias"
    sd = dict(sd)
    sd[name] = (sd[name] + np.float32(TAU - np.median(valid))).astype(np.float32)
    eng.load_state_dict(sd)
    try:
        eng.set_substreams(1)
        want = _call(eng, inp)
        eng.set_substreams(2)
        got = _call(eng, inp)
    finally:
        eng.set_substreams(1)
    for b, p in enumerate(pairs):      # pruning fired on both sides of every pair, in both groups, and left rows standing
        for pr, n in ((want["prune0"][b], len(p.kp_q)), (want["prune1"][b], len(p.kp_r))):
            assert (pr[:n] == NL).any() and (pr[:n] == NL - 1).any() and (pr[n:] == 0).all(), b
    assert (want["n_match"] > 0).all()
    _assert_pairs_equal(got, want, range(B), "pruned")

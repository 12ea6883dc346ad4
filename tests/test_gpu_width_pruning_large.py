"""LightGlue point pruning on the GPU on sides above 1024 keypoints, against the CPU restatement tests/width_pruning_ref.py: the worlds of
tests/width_pruning_large_common.py (their docstrings say which path of gn_prune.hip each one is for).  Preconditions, margins and budgets are
those of tests/test_gpu_width_pruning.py and are asserted on the CPU when a world is built; nothing here is measured on the code under test --
every comparison is exact, or uses F32_SCORE / FP16_LAYER3 / F32_LAYER as copied there.

kornia is not importable here: the helper restates the public kornia 0.7.2 / cvg LightGlue source and parity with it is unpinned.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import width_pruning_large_common as lc  # noqa: E402
import width_pruning_ref as wp  # noqa: E402
from gisnav_amd.engine import PoseEngine  # noqa: E402
from width_pruning_large_common import F32_SCORE, NL, WC  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(w, B, K, prec="f32"):
    return PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=w["sd"], filter_threshold=w["th"], feature=w["feature"])


def _match(eng, inp):
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()


def _padded(v, kmax):
    out = np.zeros(kmax, np.int32)
    out[:len(v)] = v
    return out


def _sizes(w):
    return [(len(p.kp_q), len(p.kp_r)) for p in w["pairs"]]


def _kmax(w):
    return int(lc.tiles(max(max(s) for s in _sizes(w))) * 128)


def _same_as_helper(got, b, ref, score_tol, nq, nr):
    """The match list of pair b: the helper's indices exactly, ascending in the query index, ORIGINAL keypoint indices (k_unprune_idx on every
    workgroup of the list: an entry it missed would be a row of the pruned side, which repeats or leaves the order), the scores within score_tol."""
    idx, score, n = got
    k = int(n[b])
    assert k == len(ref["idx"]) and np.array_equal(idx[b, :k], ref["idx"]), (b, k, len(ref["idx"]))
    assert k > 0 and (np.diff(idx[b, :k, 0]) > 0).all()
    assert idx[b, :k].min() >= 0 and idx[b, :k, 0].max() < nq and idx[b, :k, 1].max() < nr
    assert len(np.unique(idx[b, :k], axis=0)) == k and len(np.unique(idx[b, :k, 1])) == k      # (mutual matches: a reference keypoint at most once)
    if score_tol is not None:
        assert np.abs(score[b, :k] - ref["score"]).max() < score_tol, b


def _prune_equals(p0, p1, b, r, kmax):
    assert np.array_equal(p0[b], _padded(r["prune0"], kmax)) and np.array_equal(p1[b], _padded(r["prune1"], kmax)), b


def _check_f32_pair(kmax, got, p0, p1, counts, b, r, nq, nr):
    _prune_equals(p0, p1, b, r, kmax)
    assert p0[b].max() == 1 + len([k for k in r["kept"] if k[1] == 0]) and p1[b].max() == 1 + len([k for k in r["kept"] if k[1] == 1])
    assert np.array_equal(counts[b].T, np.array(r["counts"][:NL - 1])), (b, counts[b].T, r["counts"])
    _same_as_helper(got, b, r, F32_SCORE, nq, nr)


@functools.lru_cache(maxsize=None)
def _one_pair_f32(name):
    """One matcher call of a one-pair world in f32 on an engine of the side maximum rounded up to 128; shared with the active-size test."""
    w = lc.WORLDS[name]()
    eng = _engine(w, 1, _kmax(w))
    eng.set_width_pruning(WC, w["mink"])
    assert eng.width_pruning() == (pytest.approx(WC), w["mink"]) and eng.kmax == _kmax(w)
    got = _match(eng, eng.stage_inputs(w["pairs"]))
    p0, p1 = eng.last_prune(1)
    counts = eng.debug_read("prune_counts", 2 * NL, dtype=np.int32).reshape(1, 2, NL)[:, :, :NL - 1]
    return eng.kmax, got, p0, p1, counts      # (the engine goes: nothing of it is kept for the rest of the run)


@pytest.mark.parametrize("name", ["L-A", "L-B1", "L-B2", "L-T"])
def test_one_pair_f32_equals_the_helper(name):
    w = lc.WORLDS[name]()
    kmax, got, p0, p1, counts = _one_pair_f32(name)
    (nq, nr), = _sizes(w)
    _check_f32_pair(kmax, got, p0, p1, counts, 0, w["refs"][0]["r32"], nq, nr)
    if name == "L-T":      # n == min_kpts is not pruned, n == min_kpts + 1 is
        assert (p1[0][:nr] == 1).all() and p0[0].max() > 1 and p0[0][:nq].min() < p0[0].max()


def test_256d_feature_equals_the_helper():
    w = lc.world_ls()
    kmax, got, p0, p1, counts = _one_pair_f32("L-S")
    (nq, nr), = _sizes(w)
    _check_f32_pair(kmax, got, p0, p1, counts, 0, w["refs"][0]["r32"], nq, nr)


def test_default_threshold_two_pair_batch_and_each_pair_alone():
    w = lc.world_lc()
    sizes = _sizes(w)
    eng = _engine(w, 2, _kmax(w))
    eng.set_width_pruning(WC)                                   # no min_kpts: the default
    assert eng.width_pruning() == (pytest.approx(WC), 1536)
    got = _match(eng, eng.stage_inputs(w["pairs"]))
    p0, p1 = eng.last_prune(2)
    counts = eng.debug_read("prune_counts", 2 * 2 * NL, dtype=np.int32).reshape(2, 2, NL)[:, :, :NL - 1]
    for b, (nq, nr) in enumerate(sizes):
        _check_f32_pair(eng.kmax, got, p0, p1, counts, b, w["refs"][b]["r32"], nq, nr)
    assert p1[0][:1537].min() < p1[0].max() and (p0[1][:1536] == 1).all() and (p0[1][1536:] == 0).all()      # 1537 is pruned, 1536 never is
    assert int(got[2][1]) > 1000
    for b in range(2):
        alone = _match(eng, eng.stage_inputs(w["pairs"][b:b + 1]))
        a0, a1 = eng.last_prune(1)
        k = int(got[2][b])
        assert int(alone[2][0]) == k and np.array_equal(alone[0][0, :k], got[0][b, :k]), b
        assert np.array_equal(a0[0], p0[b]) and np.array_equal(a1[0], p1[b]), b


@pytest.mark.parametrize("prec", sorted(lc.D_MODES))
def test_sixteen_bit_modes_on_a_bulk_grid(prec):
    w = lc.world_ld()
    pairs, inps, sd, refs, mink = w["pairs"], w["inps"], w["sd"], w["refs"], w["mink"]
    assert min(r["worst"] for r in refs) > lc.D_MODES[prec]      # the precondition: every |z - tau| > ||w_i||_1 max|x64| L of this mode
    _, B, K = lc.grid_d()
    eng = _engine(w, B, K, prec)
    eng.set_certify("off")
    eng.set_ffn_products(3)
    eng.set_ragged(True)                      # the block tail walks the lists whatever the previous call's padding
    inp = eng.stage_inputs(pairs)
    eng.set_width_pruning(WC, mink)
    eng.set_kernel_timing(400)
    got = _match(eng, inp)
    table = {r["name"]: int(r["launches"]) for r in eng.kernel_table()}
    eng.set_kernel_timing(0)
    lists_on = eng.debug_read("lists", 2, dtype=np.int32)      # the call's work lists as its last launches walked them: [0] tiles, [1] attention items
    assert eng.guard_status()[0] is False
    count = lambda t, pre: sum(v for k, v in t.items() if k.startswith(pre))  # noqa: E731
    assert count(table, "k_prune") == NL - 1, table
    assert count(table, "k_ffn128<0, true, true,") == 2 * NL, table      # the block tail is k_ffn128 in its walking form (third template argument)
    if prec == "f16x2_f16_attn":
        assert count(table, "k_attn_pw") > 0, table                       # bulk attention, walking the lists' items
    p0, p1 = eng.last_prune(B)
    counts = eng.debug_read("prune_counts", 2 * B * NL, dtype=np.int32).reshape(B, 2, NL)
    sizes = np.array(_sizes(w))
    per_slot = [lc.tiles(sizes)] + [lc.tiles(counts[:, :, i]) for i in range(NL - 1)]      # [in front of layer 0, after layer 0 .. NL - 2][pair][side]
    totals = [int(t.sum()) for t in per_slot]
    first = lc.PRUNE_LAYERS[0]
    assert totals[1] == totals[0] and totals[first + 1] < totals[first] and totals[-1] < totals[first + 1], totals
    assert (per_slot[first] - per_slot[first + 1]).max() >= 2, per_slot      # a slot's share of the lists shrinks by several tiles at once
    # the lists themselves, read from the device: rebuilt behind the last pruning layer, they hold the tiles of the FINAL counts
    final = np.array([refs[b]["r64"]["counts"][-1] for b in range(B)])
    assert int(lists_on[0]) == int(lc.tiles(final).sum()) == totals[-1], (lists_on, totals)
    assert int(lists_on[1]) == 4 * int(lc.tiles(final, 256).sum()), (lists_on, final)
    for b, (nq, nr) in enumerate(sizes):
        _prune_equals(p0, p1, b, refs[b]["r64"], eng.kmax)
        forced = {}
        for s, pv, n in ((0, p0[b], nq), (1, p1[b], nr)):      # the GPU's own kept sets, from its prune vectors and per-layer counts
            before = [int(n)] + [int(c) for c in counts[b, s, :NL - 2]]
            forced.update({(i, s): v for i, v in wp.kept_from_prune(pv, int(n), before, mink, NL).items()})
        replay = wp.forward(sd, inps[b], "sift", NL, 0.5, WC, mink, torch.float32, forced_keep=forced)
        _same_as_helper(got, b, replay, None, nq, nr)
    assert int(got[2].max()) > 256


def _two_sizes(eng, w, n_active, np_active):
    """The same call at the context's full padding and at the active size: not a result bit may differ (gn_set_active_kpts' rule)."""
    (nq, nr), = _sizes(w)
    inp = eng.stage_inputs(w["pairs"])
    assert eng.set_active_kpts(eng.kmax) == eng.kmax
    full = _match(eng, inp)
    f0, f1 = eng.last_prune(1)
    assert eng.set_active_kpts(n_active) == np_active < eng.kmax
    act = _match(eng, inp)
    a0, a1 = eng.last_prune(1)
    k = int(full[2][0])
    assert k > 256 and int(act[2][0]) == k and np.array_equal(act[0][0, :k], full[0][0, :k])
    assert np.array_equal(act[1][0, :k].view(np.uint32), full[1][0, :k].view(np.uint32))
    for f, a, n in ((f0, a0, nq), (f1, a1, nr)):
        assert f.shape == a.shape == (1, eng.kmax) and np.array_equal(f[0, :n], a[0, :n]) and f[0, :n].min() >= 1
        assert (f[0, n:] == 0).all() and (a[0, n:] == 0).all()
    assert f0[0].max() > f0[0, :nq].min()                       # pruning dropped rows in these calls
    return full, f0, f1


def test_active_size_with_pruning_on_changes_no_bit():
    w = lc.world_lb1()
    (nq, nr), = _sizes(w)
    eng = _engine(w, 1, 2304)
    eng.set_width_pruning(WC, w["mink"])
    full, f0, f1 = _two_sizes(eng, w, 1025, 1152)
    # the engine of test_one_pair_f32_equals_the_helper[L-B1], whose max_kpts is 1152
    kmax1, got1, p0, p1, _ = _one_pair_f32("L-B1")
    k = int(got1[2][0])
    assert kmax1 == 1152 and int(full[2][0]) == k and np.array_equal(full[0][0, :k], got1[0][0, :k])
    assert np.array_equal(full[1][0, :k].view(np.uint32), got1[1][0, :k].view(np.uint32))
    assert np.array_equal(f0[0, :nq], p0[0, :nq]) and np.array_equal(f1[0, :nr], p1[0, :nr])
    # a 16-bit mode: full padding against the active size only (no helper: its decisions need not be the f32 ones with these dense weights)
    eng16 = _engine(w, 1, 2304, "f16x2_f16_attn")
    eng16.set_certify("off")
    eng16.set_width_pruning(WC, w["mink"])
    _two_sizes(eng16, w, 1025, 1152)

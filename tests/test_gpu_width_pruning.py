"""LightGlue point pruning on the GPU (gn_set_width_pruning) against the CPU restatement tests/width_pruning_ref.py.

Precondition of every comparison, asserted on the CPU and never skipped -- "the decisions are settled": the helper's fp64 and f32 runs agree on
every keep / drop decision and every |z - tau| exceeds the case's margin, so a GPU run that is within its mode's error budget MUST take the same
decisions.  Margins: f32 cases 1e-3 (absolute, in z).  16-bit modes: ||w_i||_1 * max|x64| * L with L the per-layer relative budget that
tests/test_gpu_fp64_parity.py asserts for the mode (FP16_LAYER[3] = 6.5e-5 for "f16x2_f16_attn" on three products, F32_LAYER = 2e-5 for
"f16x2_f16x2_attn"; copied below, not measured on the code under test): |z_gpu - z_64| <= ||w||_1 max|dx| <= ||w||_1 max|x| L.

Weights: width_pruning_ref.build_pruning_weights -- margin-built weights, matchability bias +30 everywhere but on three pruning layers (1, 4, 6),
where the bias puts the threshold into the widest gap of the pooled fp64 z.  For the 16-bit cases the pruning layers' matchability WEIGHT is
one-hot instead of dense: the 16-bit margin is relative to ||w||_1 max|x| (scaling w does not help), and the widest gap of the pooled values of a
dense 256-term z over a bulk grid's keypoints is narrower than that margin whatever the seed, while a one-hot w (||w||_1 = |w_k|) clears it at every
decision of the grid.  The margin formula itself is as stated.

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

import width_pruning_ref as wp  # noqa: E402
from gisnav_amd import _lib  # noqa: E402
from gisnav_amd.engine import MIN_MATCHES, PoseEngine  # noqa: E402
from gisnav_amd.synthetic import K_MATRIX, make_pair, make_pair_256  # noqa: E402
from gisnav_amd.weights import synthetic_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

WC, MINK, NL = 0.99, 100, 9
PRUNE_LAYERS = (1, 4, 6)
KEEP = {1: (0.7, 0.85), 4: (0.5, 0.7), 6: (0.5, 0.75)}
F32_MARGIN = 1e-3
F32_SCORE = 1e-5                                   # tests/test_gpu_parity.py: match scores of the f32 kernels against the torch-CPU oracle
FP16_LAYER3, F32_LAYER = 6.5e-5, 2e-5              # tests/test_gpu_fp64_parity.py: FP16_LAYER[3] (headline mode, three products), F32_LAYER (mode 5)
SIZES = [(300, 173), (90, 260), (129, 128)]        # A = the first; B = all three: one side under min_kpts beside a pruned one, a pair astride a tile edge
SEED = 21000                                       # (chosen on the CPU: the precondition below holds with 5x room)


def _check_world(sd, inps, feature, th, margin_of, need=1.0):
    """The preconditions on the CPU; returns per pair the fp64 / f32 runs and `worst`, the smallest |z - tau| / margin over its decisions."""
    refs = []
    for b, inp in enumerate(inps):
        r64, r32, worst = wp.settled(sd, inp, feature, WC, MINK, margin_of, NL, th)
        assert worst > need, (b, worst)                                                  # every |z - tau| exceeds the margin, in both runs
        fired = {k[0] for k in r64["kept"] if len(r64["kept"][k]) < len(r64["present"][k])}
        assert min(r64["counts"][-1]) >= 2, (b, r64["counts"])                           # every side keeps at least two points
        refs.append(dict(r64=r64, r32=r32, fired=fired, worst=worst))
    assert len(set().union(*[r["fired"] for r in refs])) >= 2                            # at least two layers prune
    return refs


@functools.lru_cache(maxsize=None)
def world_f32():
    pairs = [make_pair(SEED + i, n_q=q, n_r=r) for i, (q, r) in enumerate(SIZES)]
    inps = [wp.sift_inputs(p) for p in pairs]
    sd, half = wp.build_pruning_weights(inps, "sift", 0, PRUNE_LAYERS, WC, MINK, 100.0, KEEP)
    refs = _check_world(sd, inps, "sift", 0.5, lambda l, s, r: F32_MARGIN)
    c0 = [c[0] for c in refs[0]["r32"]["counts"]]      # case A: the 300-keypoint side loses whole 128-row tiles twice
    assert c0[0] == 300 and 128 < c0[PRUNE_LAYERS[0]] <= 256 and c0[-1] <= 128, c0
    c1 = refs[1]["r32"]["counts"]                      # case B: the 90-keypoint side is never pruned, its partner is
    assert all(c[0] == 90 for c in c1) and c1[-1][1] < 260
    return pairs, inps, sd, refs


@functools.lru_cache(maxsize=None)
def world_sp():
    pairs = [make_pair_256(SEED + 50, n_q=260, n_r=150)]
    inps = [wp.sp_inputs(p) for p in pairs]
    sd, half = wp.build_pruning_weights(inps, "superpoint", 0, PRUNE_LAYERS, WC, MINK, 100.0, KEEP)
    refs = _check_world(sd, inps, "superpoint", 0.1, lambda l, s, r: F32_MARGIN)
    return pairs, inps, sd, refs


@functools.lru_cache(maxsize=None)
def world_one():
    """A pair whose query side is pruned down to ONE keypoint (the reference side starts under min_kpts and is never pruned): the f32 weights with
    the layer-2 bias moved between the largest and the second largest z of the query rows that layer sees.  filter_threshold 0: the one row's best
    column is a mutual match whatever its score, so 'runs on' shows as exactly one match."""
    _, _, sd, _ = world_f32()
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    pair = make_pair(SEED + 20, n_q=300, n_r=95)
    inp = wp.sift_inputs(pair)
    sd["log_assignment.2.matchability.bias"] = np.array([30.0], np.float32)
    sd["log_assignment.2.matchability.weight"] = (20.0 * sd["log_assignment.2.matchability.weight"]).astype(np.float32)      # (widens the top gap)
    r = wp.forward(sd, inp, "sift", NL, 0.0, WC, MINK, torch.float64, stop_before_layer=3)
    u = np.sort(r["z"][(2, 0)].numpy() - 30.0)
    assert (2, 1) not in r["z"] and u[-1] - u[-2] > 4 * F32_MARGIN
    sd["log_assignment.2.matchability.bias"] = np.array([wp.tau(WC) - 0.5 * (u[-1] + u[-2])], np.float32)
    r64, r32, worst = wp.settled(sd, inp, "sift", WC, MINK, lambda l, s, rr: F32_MARGIN, NL, 0.0)
    assert worst > 1.0 and r32["counts"][-1] == (1, 95) and len(r32["idx"]) == 1, (worst, r32["counts"], r32["idx"])
    return pair, sd, r32


def _grid_d():
    """tests/test_gpu_fp64_parity.py::_grid("4x512") with the sides shrunk to ~300 and max_kpts raised to 4096 (PoseNode's default): 4 pairs x 2 x
    4096 rows = 256 tiles of 128, the fewest pairs with which the block tail runs as k_ffn128 (it needs 256 tiles; k_qkv and k_attn_pw need 128)
    -- the CPU reference costs per pair, the padding costs the list-walking kernels nothing."""
    return [make_pair(11200 + i, n_q=300 - 23 * i, n_r=300 - 11 * i) for i in range(4)], 4, 4096


@functools.lru_cache(maxsize=None)
def world_d():
    """One set of weights and CPU runs for both 16-bit modes: `worst` is measured in units of ||w_i||_1 max|x64|, to be compared with the mode's L."""
    pairs, B, K = _grid_d()
    inps = [wp.sift_inputs(p) for p in pairs]
    base = synthetic_state_dict(0)
    rng = np.random.default_rng(3)
    for li in PRUNE_LAYERS:      # one-hot matchability weights on the pruning layers (module docstring)
        w = np.zeros((1, 256), np.float32)
        w[0, int(rng.integers(256))] = 0.01 * float(rng.choice([-1.0, 1.0]))
        base[f"log_assignment.{li}.matchability.weight"] = w
    sd, half = wp.build_pruning_weights(inps, "sift", 0, PRUNE_LAYERS, WC, MINK, 100.0, KEEP, base=base)
    l1 = {i: float(np.abs(sd[f"log_assignment.{i}.matchability.weight"]).sum()) for i in range(NL)}
    refs = _check_world(sd, inps, "sift", 0.5, lambda l, s, r: l1[l] * r["xmax"][(l, s)], need=0.0)
    return pairs, inps, sd, refs


def _engine(sd, B, K, prec="f32", feature="sift", th=0.5):
    return PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=th, feature=feature)


def _match(eng, inp):
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()


def _padded(v, kmax):
    out = np.zeros(kmax, np.int32)
    out[:len(v)] = v
    return out


def _same_as_helper(eng, got, b, ref, score_tol):
    idx, score, n = got
    k = int(n[b])
    assert k == len(ref["idx"]) and np.array_equal(idx[b, :k], ref["idx"]), b
    assert k > 0 and (np.diff(idx[b, :k, 0]) > 0).all()
    if score_tol is not None:
        assert np.abs(score[b, :k] - ref["score"]).max() < score_tol, b


@pytest.fixture(scope="module")
def eng3():
    _, _, sd, _ = world_f32()
    return _engine(sd, 3, 384)


def test_a_one_pair_f32_equals_the_helper(eng3):
    pairs, _, _, refs = world_f32()
    eng3.set_width_pruning(WC, MINK)
    assert eng3.width_pruning() == (pytest.approx(WC), MINK)
    got = _match(eng3, eng3.stage_inputs(pairs[:1]))
    p0, p1 = eng3.last_prune(1)
    r = refs[0]["r32"]
    assert np.array_equal(p0[0], _padded(r["prune0"], eng3.kmax)) and np.array_equal(p1[0], _padded(r["prune1"], eng3.kmax))
    assert p0[0].max() == 1 + len([k for k in r["kept"] if k[1] == 0])
    _same_as_helper(eng3, got, 0, r, F32_SCORE)
    counts = eng3.debug_read("prune_counts", 2 * NL, dtype=np.int32).reshape(2, NL)[:, :NL - 1]
    assert np.array_equal(counts.T, np.array(r["counts"][:NL - 1]))


def test_b_ragged_batch_equals_the_helper_and_each_pair_alone(eng3):
    pairs, _, _, refs = world_f32()
    eng3.set_width_pruning(WC, MINK)
    got = _match(eng3, eng3.stage_inputs(pairs))
    p0, p1 = eng3.last_prune(3)
    for b in range(3):
        r = refs[b]["r32"]
        assert np.array_equal(p0[b], _padded(r["prune0"], eng3.kmax)) and np.array_equal(p1[b], _padded(r["prune1"], eng3.kmax)), b
        _same_as_helper(eng3, got, b, r, F32_SCORE)
    assert (p0[1][:90] == 1).all() and p1[1].max() > 1          # the side under min_kpts was never up for pruning, its partner was
    for b in range(3):
        alone = _match(eng3, eng3.stage_inputs(pairs[b:b + 1]))
        a0, a1 = eng3.last_prune(1)
        k = int(got[2][b])
        assert int(alone[2][0]) == k and np.array_equal(alone[0][0, :k], got[0][b, :k]), b
        assert np.array_equal(a0[0], p0[b]) and np.array_equal(a1[0], p1[b]), b


def test_c_neutral_settings_are_bitwise_off(eng3):
    pairs, _, _, _ = world_f32()
    inp = eng3.stage_inputs(pairs)
    eng3.set_width_pruning(-1.0)
    assert eng3.width_pruning()[0] == -1.0
    off = _match(eng3, inp)
    q0, q1 = eng3.last_prune(3)
    for b, (nq, nr) in enumerate(SIZES):      # kornia without pruning: n_layers for every keypoint
        assert (q0[b, :nq] == NL).all() and (q0[b, nq:] == 0).all() and (q1[b, :nr] == NL).all() and (q1[b, nr:] == 0).all()
    eng3.set_width_pruning(WC, 384)           # on, but no side is ever above min_kpts
    on = _match(eng3, inp)
    p0, p1 = eng3.last_prune(3)
    eng3.set_width_pruning(0.0)
    again = _match(eng3, inp)
    r0, r1 = eng3.last_prune(3)
    assert np.array_equal(off[2], on[2]) and np.array_equal(off[2], again[2]) and off[2].min() > 0
    for b, (nq, nr) in enumerate(SIZES):
        k = int(off[2][b])
        for other in (on, again):
            assert np.array_equal(off[0][b, :k], other[0][b, :k]) and np.array_equal(off[1][b, :k].view(np.uint32), other[1][b, :k].view(np.uint32)), b
        assert (p0[b, :nq] == 1).all() and (p0[b, nq:] == 0).all() and (p1[b, :nr] == 1).all() and (p1[b, nr:] == 0).all()
    assert np.array_equal(r0, q0) and np.array_equal(r1, q1)


D_MODES = {"f16x2_f16_attn": FP16_LAYER3, "f16x2_f16x2_attn": F32_LAYER}


@pytest.mark.parametrize("prec", sorted(D_MODES))
def test_d_sixteen_bit_modes_on_a_bulk_grid(prec):
    pairs, inps, sd, refs = world_d()
    assert min(r["worst"] for r in refs) > D_MODES[prec]      # the precondition: every |z - tau| > ||w_i||_1 max|x64| L of this mode
    _, B, K = _grid_d()
    eng = _engine(sd, B, K, prec)
    eng.set_certify("off")
    eng.set_ffn_products(3)
    eng.set_ragged(True)                      # the block tail walks the lists whatever the previous call's padding
    inp = eng.stage_inputs(pairs)
    _match(eng, inp)                          # pruning off: the launch table of the parent's schedule
    eng.set_kernel_timing(400)
    _match(eng, inp)
    table_off = {r["name"]: int(r["launches"]) for r in eng.kernel_table()}
    lists_off = eng.debug_read("lists", 2, dtype=np.int32)
    eng.set_width_pruning(WC, MINK)
    eng.set_kernel_timing(400)
    got = _match(eng, inp)
    table = {r["name"]: int(r["launches"]) for r in eng.kernel_table()}
    eng.set_kernel_timing(0)
    lists_on = eng.debug_read("lists", 2, dtype=np.int32)      # the call's work lists as its last launches walked them: [0] tiles, [1] attention items
    assert eng.guard_status()[0] is False
    count = lambda t, pre: sum(v for k, v in t.items() if k.startswith(pre))  # noqa: E731
    assert count(table, "k_prune") == NL - 1 and count(table_off, "k_prune") == 0
    # the block tail is k_ffn128 in its walking form (third template argument), before and after, in both modes
    assert count(table, "k_ffn128<0, true, true,") == count(table_off, "k_ffn128<0, true, true,") == 2 * NL, (table, table_off)
    if prec == "f16x2_f16_attn":
        assert count(table, "k_attn_pw") == count(table_off, "k_attn_pw") > 0      # bulk attention, walking the lists' items
        # off: every cross tail but the last fuses the next self projection; on: none does -- the self projections are k_qkv launches again
        assert count(table_off, "k_ffn128<0, true, true, 1,") == NL - 1 and count(table_off, "k_qkv<false,") == 1
        assert count(table, "k_ffn128<0, true, true, 1,") == 0 and count(table, "k_qkv<false,") == NL
        assert count(table, "k_ffn128<0, true, true, 2,") == NL == count(table_off, "k_ffn128<0, true, true, 2,")   # self tail -> cross fusion stays
    p0, p1 = eng.last_prune(B)
    counts = eng.debug_read("prune_counts", 2 * B * NL, dtype=np.int32).reshape(B, 2, NL)
    tiles = [int(((np.array([[len(p.kp_q), len(p.kp_r)] for p in pairs]) + 127) // 128).sum())]
    tiles += [int(((counts[:, :, i] + 127) // 128).sum()) for i in range(NL - 1)]
    assert tiles[1] == tiles[0] and tiles[PRUNE_LAYERS[0] + 1] < tiles[PRUNE_LAYERS[0]] and tiles[-1] < tiles[PRUNE_LAYERS[0] + 1], tiles      # fewer tiles in the lists behind a pruning layer
    # the lists themselves, read from the device: rebuilt behind the last pruning layer, they hold the tiles of the FINAL counts
    final = np.array([refs[b]["r64"]["counts"][-1] for b in range(B)])
    assert int(lists_off[0]) == tiles[0] and int(lists_on[0]) == int(((final + 127) // 128).sum()) == tiles[-1] < int(lists_off[0]), (lists_on, lists_off, tiles)
    assert int(lists_on[1]) == 4 * int(((final + 255) // 256).sum()) < int(lists_off[1])
    for b, p in enumerate(pairs):
        r64 = refs[b]["r64"]
        nq, nr = len(p.kp_q), len(p.kp_r)
        assert np.array_equal(p0[b], _padded(r64["prune0"], eng.kmax)) and np.array_equal(p1[b], _padded(r64["prune1"], eng.kmax)), b
        forced = {}
        for s, pv, n in ((0, p0[b], nq), (1, p1[b], nr)):      # the GPU's own kept sets, from its prune vectors and per-layer counts
            before = [n] + [int(c) for c in counts[b, s, :NL - 2]]
            forced.update({(i, s): v for i, v in wp.kept_from_prune(pv, n, before, MINK, NL).items()})
        replay = wp.forward(sd, inps[b], "sift", NL, 0.5, WC, MINK, torch.float32, forced_keep=forced)
        _same_as_helper(eng, got, b, replay, None)
    # the mutual refusal on a context that has a certificate to calibrate
    with pytest.raises(_lib.GnError, match="pruning"):
        eng.calibrate_certify(inp)


def test_d_z_from_the_hm16_planes_with_dense_weights():
    """k_prune_z's read of the hm16 rows on all 256 columns: margin-built weights as they come (dense matchability weights, bias +10: every layer
    fires and keeps every row), headline mode, where the residual stream exists only as planes.  The z the kernel leaves of the last pruning layer
    (gn_debug_read "prune_z") against the fp64 helper's, within the very bound the decisions' margin stands on: ||w||_1 max|x64| L."""
    sd = synthetic_state_dict(0)
    p = make_pair(SEED + 30, n_q=300, n_r=289)
    r64 = wp.forward(sd, wp.sift_inputs(p), "sift", NL, 0.5, WC, MINK, torch.float64)
    eng = _engine(sd, 1, 384, "f16x2_f16_attn")
    eng.set_certify("off")
    eng.set_width_pruning(WC, MINK)
    got = _match(eng, eng.stage_inputs([p]))
    z = eng.debug_read("prune_z", 2 * eng.kmax).reshape(2, eng.kmax)
    p0, p1 = eng.last_prune(1)
    assert (p0[0, :300] == NL).all() and (p1[0, :289] == NL).all() and int(got[2][0]) > 50
    l1 = float(np.abs(sd[f"log_assignment.{NL - 2}.matchability.weight"]).sum())
    for s, n in ((0, 300), (1, 289)):
        want = r64["z"][(NL - 2, s)].numpy()
        bound = l1 * r64["xmax"][(NL - 2, s)] * FP16_LAYER3
        assert want.std() > 20 * bound                      # the rows' z differ by far more than the bound: a wrong column or plane would show
        assert np.abs(z[s, :n] - want).max() <= bound, (s, np.abs(z[s, :n] - want).max(), bound)


def test_e_256d_feature_equals_the_helper():
    pairs, _, sd, refs = world_sp()
    eng = _engine(sd, 1, 384, feature="superpoint", th=0.1)
    eng.set_width_pruning(WC, MINK)
    got = _match(eng, eng.stage_inputs(pairs))
    p0, p1 = eng.last_prune(1)
    r = refs[0]["r32"]
    assert np.array_equal(p0[0], _padded(r["prune0"], eng.kmax)) and np.array_equal(p1[0], _padded(r["prune1"], eng.kmax))
    assert p0[0].max() > 2
    _same_as_helper(eng, got, 0, r, F32_SCORE)


def test_f_estimate_report_carries_original_indices(eng3):
    pairs, _, _, refs = world_f32()
    eng3.set_width_pruning(WC, MINK)
    inp = eng3.stage_inputs(pairs)
    idx, score, n = eng3.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng3.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n, inp["dem"])
    R, t, n_inl, ok = eng3.pnp_ransac(obj, mkp, n, K_MATRIX, min_pts=MIN_MATCHES)[:4]
    for out in (eng3.estimate(inp, K_MATRIX, report=True), eng3.estimate(inp, K_MATRIX, covariance=True, report=True)):
        torch.cuda.synchronize()
        assert torch.equal(out["n_match"], n) and torch.equal(out["ok"], ok) and int(ok.sum()) >= 1
        for b in range(3):
            k = int(n[b])
            assert torch.equal(out["idx"][b, :k], idx[b, :k]) and np.array_equal(out["idx"][b, :k].cpu().numpy(), refs[b]["r32"]["idx"]), b
            if int(ok[b]):
                assert torch.equal(out["R"][b], R[b]) and torch.equal(out["t"][b], t[b]), b      # bitwise: the same gathered points through the same stage
    plain = eng3.estimate(inp, K_MATRIX)
    torch.cuda.synchronize()
    assert torch.equal(plain["n_match"], n) and all(torch.equal(plain["R"][b], R[b]) for b in range(3) if int(ok[b]))
    # sub-batch streams: the groups run on slices of the pruning buffers too (two groups: pairs 0-1 and pair 2)
    eng3.set_substreams(2)
    try:
        sub = eng3.estimate(inp, K_MATRIX, report=True)
        eng3.flush()
        torch.cuda.synchronize()
        p0, p1 = eng3.last_prune(3)
    finally:
        eng3.set_substreams(1)
    assert torch.equal(sub["n_match"], n) and torch.equal(sub["ok"], ok)
    for b in range(3):
        k, r = int(n[b]), refs[b]["r32"]
        assert torch.equal(sub["idx"][b, :k], idx[b, :k]), b
        assert np.array_equal(p0[b], _padded(r["prune0"], eng3.kmax)) and np.array_equal(p1[b], _padded(r["prune1"], eng3.kmax)), b
        if int(ok[b]):
            assert torch.equal(sub["R"][b], R[b]) and torch.equal(sub["t"][b], t[b]), b


def test_g_edges():
    pairs, _, sd, _ = world_f32()
    two = [pairs[0], make_pair(SEED + 9, n_q=90, n_r=95)]      # the second pair is never above min_kpts: never pruned
    dead = {k: np.array(v, copy=True) for k, v in sd.items()}
    dead["log_assignment.2.matchability.bias"] = np.array([-30.0], np.float32)      # layer 2 keeps nothing of the sides it sees
    eng = _engine(dead, 2, 384)
    inp = eng.stage_inputs(two)
    off = _match(eng, inp)
    eng.set_width_pruning(WC, MINK)
    on = _match(eng, inp)
    p0, p1 = eng.last_prune(2)
    assert int(off[2][0]) > 0 and int(on[2][0]) == 0                                 # this build's rule: a side with nothing left -> no match
    assert p0[0].max() == 3 and p1[0].max() == 3                                     # layers 0 (kept everybody) and 1 fired before layer 2 dropped the rest
    k = int(off[2][1])
    assert k > 0 and int(on[2][1]) == k and np.array_equal(on[0][1, :k], off[0][1, :k])
    assert np.array_equal(on[1][1, :k].view(np.uint32), off[1][1, :k].view(np.uint32))            # the other pair: bit for bit what pruning off gives
    assert (p0[1][:90] == 1).all() and (p1[1][:95] == 1).all()
    x = eng.debug_read("x", 2 * 2 * eng.kmax * 256)
    assert np.isfinite(x).all() and np.isfinite(on[1][1, :k]).all()
    # gn_get_prune: no more pairs than the last call had
    with pytest.raises(_lib.GnError, match="most recent"):
        eng.last_prune(3)
    _match(eng, eng.stage_inputs(two[:1]))
    with pytest.raises(_lib.GnError, match="most recent"):
        eng.last_prune(2)
    # argument rules of the C ABI: refused with the previous setting intact
    for bad in (1.0, 1.5, float("nan"), float("inf")):
        assert eng.lib.gn_set_width_pruning(eng.ctx, bad, 7) < 0
        assert "width_confidence" in eng.lib.gn_last_error(eng.ctx).decode()
        assert eng.width_pruning() == (pytest.approx(WC), MINK)
    eng.set_width_pruning(0.5)
    assert eng.width_pruning() == (0.5, 1536)                                        # min_kpts < 0 / None: the default
    # mutual refusal with the margin certificate, in both orders
    with pytest.raises(_lib.GnError, match="pruning"):
        eng.set_certify("flag")
    with pytest.raises(_lib.GnError, match="pruning"):
        eng.set_certify("rerun")
    eng.set_certify("off")                                                           # mode 0 is always accepted
    eng.set_width_pruning(-1.0)
    eng.set_certify("flag")
    with pytest.raises(_lib.GnError, match="certif"):
        eng.set_width_pruning(WC, MINK)
    assert eng.width_pruning()[0] == -1.0
    eng.set_width_pruning(-1.0, 5)                                                   # switching it off is always accepted
    eng.set_certify("off")
    eng.set_width_pruning(WC, MINK)


def test_g_one_kept_keypoint_runs_on():
    """A side pruned down to one keypoint still matches, as in kornia (whose fewer-than-two rule looks at the input counts); with an INPUT side of
    one keypoint the pair reports no match, pruning on or off."""
    pair, sd, r32 = world_one()
    eng = _engine(sd, 2, 384, th=0.0)
    eng.set_width_pruning(WC, MINK)
    inp = eng.stage_inputs([pair, make_pair(SEED + 21, n_q=1, n_r=95)])
    got = _match(eng, inp)
    p0, p1 = eng.last_prune(2)
    assert np.array_equal(p0[0], _padded(r32["prune0"], eng.kmax)) and np.array_equal(p1[0], _padded(r32["prune1"], eng.kmax))
    assert int((p0[0] == p0[0].max()).sum()) == 1 and (p1[0][:95] == 1).all()
    assert int(got[2][0]) == 1 and np.array_equal(got[0][0, :1], r32["idx"]) and abs(float(got[1][0, 0]) - float(r32["score"][0])) < F32_SCORE
    assert int(got[2][1]) == 0

"""The worlds of the point-pruning tests on sides above 1024 keypoints (tests/test_width_pruning_large_host.py builds them all on the CPU,
tests/test_gpu_width_pruning_large.py runs them on the GPU): the sizes at which gn_prune.hip takes the paths that the 300-keypoint worlds of
tests/test_gpu_width_pruning.py never reach -- k_prune's scan over more than one 1024-row chunk (its running base, the tail chunk), a compaction
whose kept rows cross scan chunks, 128-row tiles and 256-row attention items by many tiles, k_unprune_idx beyond its first 256-match workgroup,
work lists of slots of 9 to 17 tiles that shrink by several tiles at once, the threshold at n == min_kpts and n == min_kpts + 1, and the default
min_kpts of 1536.

Settings, margins and the "decisions are settled" precondition are those of tests/test_gpu_width_pruning.py (see its docstring): every world is
built once per process (functools.lru_cache) with its precondition and its own reason for existing asserted on the CPU result, never skipped.
If a world stops meeting its precondition (the helper or gisnav_amd.synthetic changed), choose another seed on the CPU; the bar stays.

`worst` is the smallest |z - tau| / margin that width_pruning_ref.settled returns; WORST holds the values of these seeds (CPU, deterministic).
"""
import functools

import numpy as np

import width_pruning_ref as wp
from gisnav_amd.synthetic import make_pair, make_pair_256
from gisnav_amd.weights import synthetic_state_dict

# tests/test_gpu_width_pruning.py: the same settings, margins and budgets (FP16_LAYER3 / F32_LAYER there copied from tests/test_gpu_fp64_parity.py:
# FP16_LAYER[3], headline mode on three products, and F32_LAYER, mode 5)
WC, NL = 0.99, 9
PRUNE_LAYERS = (1, 4, 6)
KEEP = {1: (0.7, 0.85), 4: (0.5, 0.7), 6: (0.5, 0.75)}
F32_MARGIN = 1e-3
F32_SCORE = 1e-5
FP16_LAYER3, F32_LAYER = 6.5e-5, 2e-5
D_MODES = {"f16x2_f16_attn": FP16_LAYER3, "f16x2_f16x2_attn": F32_LAYER}
DEFAULT_MINK = wp.DEFAULT_MIN_KPTS      # 1536: what gn_set_width_pruning takes for min_kpts < 0 / None

# smallest |z - tau| / margin per pair with these seeds (L-D: in units of ||w_i||_1 max|x64|, to be compared with the mode's L)
WORST = {"L-A": (1.76,), "L-B1": (2.7,), "L-B2": (1.4,), "L-C": (1.33, 1.32), "L-T": (30.0,), "L-S": (5.4,),
         "L-D": (2.25e-4, 1.75e-4, 1.72e-4, 1.82e-4)}


def tiles(n, rows=128):
    return (np.asarray(n) + rows - 1) // rows


def check_world(sd, inps, feature, th, mink, margin_of, need=1.0, layers_firing=2, long_list=True):
    """The preconditions on the CPU; returns per pair the fp64 / f32 runs and `worst`, the smallest |z - tau| / margin over its decisions."""
    refs = []
    for b, inp in enumerate(inps):
        r64, r32, worst = wp.settled(sd, inp, feature, WC, mink, margin_of, NL, th)
        assert worst > need, (b, worst)                                                  # every |z - tau| exceeds the margin, in both runs
        fired = {k[0] for k in r64["kept"] if len(r64["kept"][k]) < len(r64["present"][k])}
        assert min(r64["counts"][-1]) >= 2, (b, r64["counts"])                           # every side keeps at least two points
        refs.append(dict(r64=r64, r32=r32, fired=fired, worst=worst))
    assert len(set().union(*[r["fired"] for r in refs])) >= layers_firing
    if long_list:      # k_unprune_idx beyond its first workgroup (256 matches each)
        assert max(len(r["r32"]["idx"]) for r in refs) > 256 and max(len(r["r64"]["idx"]) for r in refs) > 256
    return refs


def _entering(counts, n0, side):
    """A side's count in front of every layer."""
    return [n0] + [c[side] for c in counts[:-1]]


def _world(pairs, feature, th, mink, **kw):
    inps = [wp.sift_inputs(p) if feature == "sift" else wp.sp_inputs(p) for p in pairs]
    sd, _ = wp.build_pruning_weights(inps, feature, 0, PRUNE_LAYERS, WC, mink, 100.0, KEEP)
    refs = check_world(sd, inps, feature, th, mink, lambda l, s, r: F32_MARGIN, **kw)
    return dict(pairs=pairs, inps=inps, sd=sd, refs=refs, mink=mink, feature=feature, th=th)


@functools.lru_cache(maxsize=None)
def world_la():
    """Three-chunk scan: a 2100-keypoint side, whose kept rows cross the 1024-row scan chunks and land many tiles below their sources."""
    w = _world([make_pair(21101, n_q=2100, n_r=1040)], "sift", 0.5, 1000)
    for r in (w["refs"][0]["r64"], w["refs"][0]["r32"]):
        into = [_entering(r["counts"], 2100, 0)[li] for li in PRUNE_LAYERS]
        assert sum(n > 2048 for n in into) == 1 and sum(1024 < n <= 2048 for n in into) == 2, into
    return w


@functools.lru_cache(maxsize=None)
def world_lb1():
    """Chunk edge: one row in the second scan chunk (1025) beside a side that fills the first exactly (1024)."""
    w = _world([make_pair(21200, n_q=1025, n_r=1024)], "sift", 0.5, 1000, layers_firing=1)      # (both sides are under min_kpts behind layer 1)
    assert w["refs"][0]["r32"]["counts"][0] == (1025, 1024) and max(w["refs"][0]["r32"]["counts"][PRUNE_LAYERS[0]]) < 1024
    return w


@functools.lru_cache(maxsize=None)
def world_lb2():
    """Chunk edge: one row in the third scan chunk (2049) beside a side that fills two exactly (2048)."""
    w = _world([make_pair(21201, n_q=2049, n_r=2048)], "sift", 0.5, 1000)
    c = w["refs"][0]["r32"]["counts"]
    assert c[0] == (2049, 2048) and all(1024 < n < 2048 for n in c[PRUNE_LAYERS[0]]), c
    return w


@functools.lru_cache(maxsize=None)
def world_lc():
    """The default threshold (min_kpts 1536, which the GPU test passes as None): sides of 1537 and 1536 keypoints in one two-pair batch."""
    w = _world([make_pair(21202, n_q=2100, n_r=1537), make_pair(21203, n_q=1536, n_r=1700)], "sift", 0.5, DEFAULT_MINK)
    for k in ("r64", "r32"):
        r0, r1 = w["refs"][0][k], w["refs"][1][k]
        assert r0["prune1"].min() < r0["prune1"].max()                       # the 1537 side is pruned
        assert (r1["prune0"] == 1).all() and len(r1["prune0"]) == 1536       # the 1536 side never is
        for r, n0 in ((r0, (2100, 1537)), (r1, (1536, 1700))):               # a side stops being pruned once at or below 1536
            for s in (0, 1):
                into = _entering(r["counts"], n0[s], s)
                assert all(((i, s) in r["kept"]) == (into[i] > DEFAULT_MINK) for i in range(NL - 1)), (s, into)
        assert r0["counts"][-1][1] <= DEFAULT_MINK and r0["prune1"].max() == 1 + sum(n > DEFAULT_MINK for n in _entering(r0["counts"], 1537, 1)[:NL - 1])
    assert len(w["refs"][1]["r32"]["idx"]) > 1000
    return w


@functools.lru_cache(maxsize=None)
def world_lt():
    """The threshold's edge, n == min_kpts and n == min_kpts + 1: the 100 side is never pruned, the 101 side is (then it is under 100: one layer
    prunes, and sides this small cannot hold a 256-entry match list)."""
    w = _world([make_pair(21204, n_q=101, n_r=100)], "sift", 0.5, 100, layers_firing=1, long_list=False)
    for k in ("r64", "r32"):
        r = w["refs"][0][k]
        assert (r["prune1"] == 1).all() and all(c[1] == 100 for c in r["counts"])
        assert r["prune0"].min() < r["prune0"].max() and r["counts"][-1][0] < 100
    return w


@functools.lru_cache(maxsize=None)
def world_ls():
    """The 256-d feature above one scan chunk."""
    return _world([make_pair_256(21300, n_q=1300, n_r=1030)], "superpoint", 0.1, 1000, layers_firing=1)      # (both sides are under min_kpts behind layer 1)


def grid_d():
    """The grid of tests/test_gpu_width_pruning.py's case D (4 pairs at max_kpts 4096: 256 tiles, so the block tail is k_ffn128) with sides of
    1200 to 1300 keypoints in place of 300."""
    return [make_pair(11200 + i, n_q=1300 - 23 * i, n_r=1200 - 11 * i) for i in range(4)], 4, 4096


@functools.lru_cache(maxsize=None)
def world_ld():
    """16-bit bulk grid, built as test_gpu_width_pruning.world_d builds its own: one-hot matchability weights on the pruning layers, `worst` in
    units of ||w_i||_1 max|x64| (to be compared with the mode's L)."""
    pairs, B, K = grid_d()
    mink = 1000
    inps = [wp.sift_inputs(p) for p in pairs]
    base = synthetic_state_dict(0)
    rng = np.random.default_rng(3)
    for li in PRUNE_LAYERS:
        w = np.zeros((1, 256), np.float32)
        w[0, int(rng.integers(256))] = 0.01 * float(rng.choice([-1.0, 1.0]))
        base[f"log_assignment.{li}.matchability.weight"] = w
    sd, _ = wp.build_pruning_weights(inps, "sift", 0, PRUNE_LAYERS, WC, mink, 100.0, KEEP, base=base)
    l1 = {i: float(np.abs(sd[f"log_assignment.{i}.matchability.weight"]).sum()) for i in range(NL)}
    refs = check_world(sd, inps, "sift", 0.5, mink, lambda l, s, r: l1[l] * r["xmax"][(l, s)], need=0.0)
    assert min(r["worst"] for r in refs) > max(D_MODES.values())      # every |z - tau| > ||w_i||_1 max|x64| L of either mode
    n0 = [(len(p.kp_q), len(p.kp_r)) for p in pairs]
    drops = [[(i, s) for (i, s) in r["r64"]["kept"] if len(r["r64"]["kept"][(i, s)]) < len(r["r64"]["present"][(i, s)])] for r in refs]
    twice = [(b, s) for b in range(B) for s in (0, 1) if sum(k[1] == s for k in drops[b]) >= 2]
    once = [(b, s) for b in range(B) for s in (0, 1) if sum(k[1] == s for k in drops[b]) == 1 and refs[b]["r64"]["counts"][-1][s] <= mink]
    assert twice and once, (twice, once)      # a side fires on two layers; another stops at or below min_kpts after its first firing
    c = np.array([[n0[b]] + list(refs[b]["r64"]["counts"]) for b in range(B)])      # [pair][in front of layer 0, after layer 0 .. NL - 1][side]
    assert (tiles(c[:, PRUNE_LAYERS[0]]) - tiles(c[:, PRUNE_LAYERS[0] + 1])).max() >= 2      # a slot's list shrinks by two tiles or more at once
    return dict(pairs=pairs, inps=inps, sd=sd, refs=refs, mink=mink, feature="sift", th=0.5)


WORLDS = {"L-A": world_la, "L-B1": world_lb1, "L-B2": world_lb2, "L-C": world_lc, "L-T": world_lt, "L-S": world_ls, "L-D": world_ld}

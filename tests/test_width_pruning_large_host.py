"""The worlds of tests/test_gpu_width_pruning_large.py on the CPU: every world is built here, so its "decisions are settled" precondition, its own
reason for existing (asserted inside tests/width_pruning_large_common.py) and the count patterns below are checked without a GPU.  The helper is
deterministic: equal seeds give equal `worst` values, to the digits recorded in WORST."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import width_pruning_large_common as lc  # noqa: E402

# fp64 counts (query, reference) after layers 0 / 1 / 4 / 6 / last, per pair
COUNTS = {
    "L-A": [[(2100, 1040), (1776, 878), (1151, 878), (862, 878), (862, 878)]],
    "L-B1": [[(1025, 1024), (836, 841), None, None, None]],
    "L-B2": [[(2049, 2048), (1725, 1727), (1174, 1157), (864, 870), (864, 870)]],
    "L-C": [[(2100, 1537), (1732, 1265), (1115, 1265), None, None], [(1536, 1700), (1536, 1436), None, None, None]],
    "L-T": [[(101, 100), (83, 100), (83, 100), (83, 100), (83, 100)]],
    "L-S": [[(1300, 1030), (994, 780), None, None, None]],
    "L-D": [[(1300, 1200), (1118, 1029), (719, 654), None, None], None, None, None],
}


@pytest.mark.parametrize("name", sorted(lc.WORLDS))
def test_world_is_settled_and_has_its_counts(name):
    w = lc.WORLDS[name]()      # (asserts the preconditions and the world's reason for existing)
    assert w is lc.WORLDS[name]()      # built once per process
    worst = [r["worst"] for r in w["refs"]]
    print(name, "worst", worst, "counts", [r["r64"]["counts"] for r in w["refs"]], "matches", [len(r["r32"]["idx"]) for r in w["refs"]])
    assert min(worst) > (max(lc.D_MODES.values()) if name == "L-D" else 1.0)
    assert worst == pytest.approx(list(lc.WORST[name]), rel=0.05)
    for b, want in enumerate(COUNTS[name]):
        if want is None:
            continue
        for k in ("r64", "r32"):
            c = w["refs"][b][k]["counts"]
            assert len(c) == lc.NL
            got = [c[0], c[1], c[4], c[6], c[-1]]
            assert all(g == x for g, x in zip(got, want) if x is not None), (b, k, c)
            assert all(c[i] == c[i - 1] for i in range(1, lc.NL) if i not in lc.PRUNE_LAYERS)      # rows leave on the pruning layers only


def test_ld_sides_that_stop_after_their_first_firing():
    w = lc.world_ld()
    for b, n in ((1, 997), (3, 996)):      # at or below min_kpts 1000 behind layer 1: never pruned again
        c = w["refs"][b]["r64"]["counts"]
        assert c[1][1] == n and all(x[1] == n for x in c[1:])
    sizes = np.array([(len(p.kp_q), len(p.kp_r)) for p in w["pairs"]])
    assert lc.tiles(sizes).min() >= 9 and lc.tiles(2100) == 17      # slots of 9 to 17 tiles (L-A's query side: 17)

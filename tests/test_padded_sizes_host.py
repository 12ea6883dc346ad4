"""The pairs, sizes and budgets of tests/test_gpu_fp64_padded_sizes.py on the CPU: every pair's fp64 run exists and matches, the tile counts are
the ones gn_api.hip's dispatch thresholds turn on, and the budget constants are those of tests/test_gpu_fp64_parity.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import padded_sizes_common as pc  # noqa: E402


def _src(name):
    with open(os.path.join(ROOT, "gisnav_amd", "csrc", name)) as f:
        return f.read()


def _check_pair(p, need):
    r = pc.ref64(p)
    assert r is pc.ref64(p)      # cached: the GPU cases of every mode share one run
    assert len(p.kp_q) >= 2 and len(p.kp_r) >= 2
    assert len(r["idx"]) >= need, (len(p.kp_q), len(p.kp_r), len(r["idx"]))
    assert r["best"].shape == (len(p.kp_q),) and all(r["layers"][l][s].shape == (n, 256) for l in pc.LAYERS for s, n in ((0, len(p.kp_q)), (1, len(p.kp_r))))


@pytest.mark.parametrize("P", pc.SINGLE_SIZES)
def test_single_pair_sides_and_reference(P):
    nq, nr = pc.SINGLE_SIDES[P]
    assert (nq, nr) == {128: (125, 2), 384: (384, 257), 640: (637, 513), 1152: (1149, 1025), 2176: (2173, 2049), 4096: (4093, 200)}[P]
    assert (max(nq, nr) + 127) // 128 * 128 == P      # what set_active_kpts(max(n_q, n_r)) pads to
    # the last 128-row tile of the query side is full but for three rows (P = 384: full), that of the reference side holds one keypoint (P = 128: two)
    assert (nq - 1) % 128 + 1 in (125, 128) and ((nr - 1) % 128 + 1 in (1, 2) or P == 4096)
    p = pc.single_pair(P)
    assert (len(p.kp_q), len(p.kp_r)) == (nq, nr)
    # a reference side of two keypoints cannot hold MIN_MATCHES matches: that pair is asked for a match at all (it has one true correspondence)
    _check_pair(p, pc.MIN_MATCHES if min(nq, nr) >= pc.MIN_MATCHES else 1)


@pytest.mark.parametrize("name", sorted(pc.GROUPS))
def test_group_sides_and_references(name):
    pairs, B, K, active = pc.group(name)
    assert pairs is pc.group(name)[0] and len(pairs) == B
    sizes = [(len(p.kp_q), len(p.kp_r)) for p in pairs]
    assert sizes == pc.group_sizes(name)
    assert all(max(max(s) for s in sizes) <= P <= K and P % 128 == 0 for P in active)
    for p in pairs:
        _check_pair(p, pc.MIN_MATCHES)
    rest = sizes[2:]
    if name == "8x1152":
        assert sizes[:2] == [(1149, 1025), (600, 1152)] and all(130 <= n <= 400 for s in rest for n in s)
    if name == "26x640":
        assert all(min(s) >= 600 and max(s) == 640 for s in sizes[:2])
        assert any(129 in s for s in rest) and any(127 in s for s in rest)
        assert all(130 <= n <= 300 or n in (127, 129) for s in rest for n in s)
        assert sum(min(s) >= 256 for s in sizes) >= 2      # the pairs the one-product level's 2.0 x level-2 rule is measured on
    if name == "pad_1":
        assert sizes == [(250, 240)]
    if name == "pad_8":
        assert max(max(s) for s in sizes) <= 500


def test_tile_counts_are_what_the_dispatch_thresholds_need():
    api, ffn, attn = _src("gn_api.hip"), _src("gn_ffn.hip"), _src("gn_attention.hip")
    # k_qkv from 128 tiles of 128 tokens, k_ffn128 from 256, k_attn_pw from 256 workgroups of 256 queries at P % 256 == 0 (four heads)
    assert re.search(r"bool qkv_projection_applies\([^{]*\{[^}]*T / 128 >= 128", api)
    # (the block tail's rule is written once, ffn_bulk_shape in gn_common.h; ffn_selects_128, launch_ffn_fused and tail_is_bulk all call it)
    assert re.search(r"bool ffn_bulk_shape\(int shape, int T\) \{[^}]*T % 128 == 0[^}]*shape == 0 && T / 128 >= 256", _src("gn_common.h"))
    assert re.search(r"bool ffn_selects_128\([^{]*\{[^}]*ffn_bulk_shape\(k\.ffn_shape, a\.T\)", ffn)
    assert ffn.count("ffn_bulk_shape(k.ffn_shape, a.T)") == 3 and "ffn_bulk_shape(c->knobs.ffn_shape, T)" in api and "/ 128 >= 256" not in ffn
    assert "a.npad % 256 == 0 && (long long)(a.npad / 256) * kHeads * a.BS >= 256" in attn
    assert "return (c->skinny & 3) && c->planes_mode && c->x_planes_only && T % 32 == 0 && np > 0 && ((c->skinny & 3) == 2 || T / np <= 4);" in api

    def pw(B, P):
        return P % 256 == 0 and (P // 256) * 4 * 2 * B >= 256

    assert 128 <= pc.tiles(8, 1152) == 144 < 256 and not pw(8, 1152)
    assert pc.tiles(26, 640) == 260 >= 256 > pc.tiles(25, 640) and not pw(26, 640)      # the fewest pairs that reach k_ffn128 at five tiles a side
    assert pc.tiles(8, 1024) == 128 and pw(8, 1024)
    assert [pc.tiles(8, P) for P in pc.GROUPS["pad_8"][3]] == [64, 128, 256] and [pw(8, P) for P in pc.GROUPS["pad_8"][3]] == [False, True, True]
    assert all(pc.tiles(1, P) < 128 for P in pc.SINGLE_SIZES)      # one pair never reaches the bulk kernels: 2 P / P <= 4 selects the small-grid family
    # the fused-projection self-check of a (26, 640) context runs at 26 x 640: the smallest batch with >= 256 tiles at the context's padded size
    assert (256 * 128 + 2 * 640 - 1) // (2 * 640) == 26


def test_budgets_are_those_of_the_fp64_parity_module():
    import test_gpu_fp64_padded_sizes as new
    import test_gpu_fp64_parity as old
    assert (new.F32_LAYER, new.F32_HEAD) == (old.F32_LAYER, old.F32_HEAD)
    assert new.FP16_LAYER == old.FP16_LAYER and new.FP16_HEAD == old.FP16_HEAD
    assert new.LEVEL1_OVER_LEVEL2 == old.LEVEL1_OVER_LEVEL2 and new.SAFETY == old.SAFETY
    assert new.LAYERS == old.LAYERS == pc.LAYERS and (new.HEADLINE, new.MODE5) == (old.HEADLINE, old.MODE5)
    assert old.FAMILIES["margin_built"][1] == pc.THRESHOLD
    from gisnav_amd.engine import MIN_MATCHES
    assert pc.MIN_MATCHES == MIN_MATCHES

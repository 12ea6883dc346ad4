"""GPU tests (-m gpu) of the LightGlue kernel families against a float64 reference (oracle.lightglue_sift.pose_node_match(..., dtype=float64)).

Until now the bulk grid (k_qkv, the projection fused into k_ffn128, k_attn_pw, k_ffn128 at three, two and one products, walking and one-tile work lists),
the small-grid kernels in the 16-bit modes and all of mode 5 were checked by correspondence indices or bitwise GPU-vs-GPU only; an error of ~1e-3 in
one family moves no index on margin-built weights, and the certificate's calibration would absorb it (eps is measured against the same GPU's f32).
Here:

  1. the residual stream after layers 1, 5 and 9 and the match head's best / runner-up score of every valid row, per precision mode and grid,
     against fp64 -- an absolute budget per mode and a consistency bound across the grids of one mode and level (grid families differ by summation
     order, not by arithmetic class: DESIGN 10.1); edge sides (n = 0, 1, 2, 127, 128, 129, 1024) on a bulk grid; padding that is never read;
  2. the certificate's eps against d = max |P - P_fp64| on every grid a certified call runs, and certified match lists against fp64's;
  3. the fused-projection self-check on a context whose active size was set before its first call, and on the two- and one-product block tails;
  4. a weight reload discards a calibrated eps.

The one-product level (k_ffn128<., ., ., ., 1>: a read-ahead of two j-steps, ten W2 k-tiles in flight, a launch path and translation unit of its
own) runs every case its level-2 sibling runs, on budgets of 2 x level 2's (one more independent rounding of the same relative size: sqrt 2 in
quadrature), and per bulk grid its layer error on the >= 256-keypoint pairs is held to 2.0 x the level-2 case's of the same process
(measured 1.33 - 1.64).

The same per-layer and head measures run on LightGlue for 256-d (SuperPoint) features, BASELINE configs[4]: f32, f16x2_bf16_attn and the
headline mode at block-tail levels 3, 2 and 1, on 1 x 1024, 4 x 1024, 16 x 1024 and the ragged batch, margin-built and default-init weights, against
oracle.lightglue_superpoint.match(..., dtype=float64).  Measured (largest over the grids, layer / head): f32 3.9e-7 / 2.7e-5 (margin-built),
1.8e-6 / 2.1e-5 (default-init); headline level 3 4.4e-5 / 1.1e-3, level 2 9.5e-5 / 2.4e-3, level 1 1.1e-4 / 3.4e-3 (margin-built); level 1 on
default-init weights 1.2e-3 / 1.1e-2 (level 2 7.9e-4 / 7.5e-3).

Every case asserts from the launch table (set_kernel_timing) that the intended kernel family ran.  Measured numbers go to
test_reports/fp64_parity.json (git-ignored), stamped with the digest of the loaded library.

Measured on an MI355X (per-layer: max |x - x64| / max |x64| over the valid rows of a side; head: max |P - P64| of best and runner-up), largest
over the grids: f32 6.3e-7 / 4.7e-5; mode 5 1.5e-6 / 5.4e-5; bf16 attention family 6.4e-5 / 9.9e-4; headline level 3 3.1e-5 / 5.3e-4, level 2
8.0e-5 / 1.9e-3, level 1 1.2e-4 / 1.8e-3.  The calibrated eps of level 1 (eps_one_product) against d = max |P - P_fp64| on 16 x 1024
and the ragged batch: d / eps <= 0.28 on the three weight families (margin-built d 2.1e-3 against eps 8.7e-3, mid-margin 3.2e-3 / 1.16e-2,
default-init 6.0e-3 / 2.2e-2).
"""
import json
import os

import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import make_pair, make_pair_256
from gisnav_amd.weights import default_init_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW_MARGIN = dict(ffn_out_std=4.8e-3, final_scale=4.0, matchability_bias=0.0, matchability_std=0.05)
MID_MARGIN = dict(ffn_out_std=1.2e-3, final_scale=12.0, matchability_bias=2.0, matchability_std=0.05)
HEADLINE = "f16x2_f16_attn"
MODE5 = "f16x2_f16x2_attn"
SAFETY = 4.0
FAMILIES = {"low_margin": (lambda: synthetic_state_dict(0, **LOW_MARGIN), 0.0), "mid_margin": (lambda: synthetic_state_dict(0, **MID_MARGIN), 0.01),
            "margin_built": (lambda: synthetic_state_dict(0), 0.5), "default_init": (lambda: default_init_state_dict(0), 0.0),
            # LightGlue on 256-d features (BASELINE configs[4]): k_prep_sp and the 2-D rotary encoding in front of the shared kernels
            "sp_margin_built": (lambda: synthetic_state_dict(0, feature="superpoint"), 0.1),
            "sp_default_init": (lambda: default_init_state_dict(0, feature="superpoint"), 0.0)}
LAYERS = (1, 5, 9)
# absolute budgets against fp64: per-layer relative error of the residual stream, and |dP| of the head's best / runner-up scores
F32_LAYER, F32_HEAD = 2e-5, 1e-4                  # f32 and mode 5 (test_gpu_parity.py's f32 bound; eps_f32)
BF16_LAYER = 3e-2                                 # the bf16-attention family (test_gpu_parity.py)
# the fp16-attention (headline) mode, per block-tail level: 2x the largest value measured over the grids of CASES (MI355X; the largest were on
# the ragged batch, whose few-keypoint sides average the fp16 rounding of q, k, v over few keys): level 3 layer 3.1e-5, head 5.3e-4; level 2
# layer 8.0e-5, head 1.9e-3
FP16_LAYER = {3: 6.5e-5, 2: 1.6e-4}
FP16_HEAD = {3: 1.1e-3, 2: 4e-3}
# default-init weights (nothing hand-shrunk: each block's update is large next to the residual) carry the fp16-attention mode's rounding further:
# measured for SIFT (16 x 1024 level 2 layer 7.5e-4 / head 4.9e-3, ragged level 3 8.9e-5 / 2.7e-4) and for the 256-d cases below (level 3 layer
# 1.2e-4 / head 7.3e-4 on the ragged batch, level 2 7.4e-4 / 8.0e-3), 1x1024 level 3 ~1e-5 / 6e-5 either way: the same shared kernels.  2x the
# largest; the margin-built cases keep the budgets above
FP16_LAYER_DEFAULT_INIT = {3: 2.5e-4, 2: 1.6e-3}
FP16_HEAD_DEFAULT_INIT = {3: 1.5e-3, 2: 1.6e-2}
# the one-product level: no measured constant.  It adds one rounding of the weights, independent of the activations' and of the same relative size
# (2^-12): the two add in quadrature to sqrt 2, which DESIGN 10.2 (and test_gpu_ffn_level1.py) bounds by 2.0 x level 2
for _budget in (FP16_LAYER, FP16_HEAD, FP16_LAYER_DEFAULT_INIT, FP16_HEAD_DEFAULT_INIT):
    _budget[1] = 2 * _budget[2]
LEVEL1_OVER_LEVEL2 = 2.0
NEEDS_PER_CASE = "run with the per-case tests of this module (they measure what is compared here)"
BUDGET = {"f32": (F32_LAYER, F32_HEAD), MODE5: (F32_LAYER, F32_HEAD), "bf16_attn": (BF16_LAYER, None), "f32x3_bf16_attn": (BF16_LAYER, None),
          "f16x2_bf16_attn": (BF16_LAYER, None)}
_REF = {}
_MEASURED = {}


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "fp64_parity.json")
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


def _family(name):
    make, th = FAMILIES[name]
    return make(), th


# ---------------------------------------------------------------------------------------------------------------- pairs and the fp64 reference
def _edge_pairs(ordinary=False, make=make_pair):
    """16 ragged pairs at 1024: sides of 0, 1, 2, 127, 128, 129 and 1024 keypoints among ordinary ragged ones (ordinary=True: the edge pairs
    1..7 replaced by ordinary pairs, every other pair the same).  The 0-keypoint side is a 5-keypoint cloud staged with n = 0.
    make=make_pair_256: the same sides with 256-d descriptors."""
    rs = np.random.default_rng(17)
    sizes = [(1024, 1024), (5, 900), (1, 700), (2, 640), (127, 1024), (128, 129), (129, 127), (1024, 2)]
    sizes += [(int(rs.integers(60, 1025)), int(rs.integers(60, 1025))) for _ in range(8)]
    if ordinary:
        sizes[1:8] = [(600 + 11 * i, 580 - 7 * i) for i in range(7)]
    return [make(12000 + i + (100 if ordinary and 1 <= i < 8 else 0), n_q=q, n_r=r) for i, (q, r) in enumerate(sizes)]


def _grid(name):
    """(pairs, max_batch, max_kpts) of a grid."""
    if name == "1x1024":
        return [make_pair(11000, n_q=1024, n_r=1000)], 1, 1024
    if name == "2x512":
        return [make_pair(11100 + i, n_q=512 - 37 * i, n_r=500) for i in range(2)], 2, 512
    if name == "4x512":
        return [make_pair(11200 + i, n_q=512 - 23 * i, n_r=512 - 11 * i) for i in range(4)], 4, 512
    if name == "16x1024":
        return [make_pair(11300 + i, n_q=1024 - 9 * (i % 3), n_r=1024 - 13 * (i % 4)) for i in range(16)], 16, 1024
    if name.startswith("ragged"):
        return _edge_pairs(), 16, 1024
    if name == "sp_1x1024":
        return [make_pair_256(15000, n_q=1024, n_r=1000)], 1, 1024
    if name == "sp_4x1024":
        return [make_pair_256(15100 + i, n_q=1024 - 31 * i, n_r=1024 - 17 * i) for i in range(4)], 4, 1024
    if name == "sp_16x1024":
        return [make_pair_256(15300 + i, n_q=1024 - 9 * (i % 3), n_r=1024 - 13 * (i % 4)) for i in range(16)], 16, 1024
    if name == "sp_ragged":
        return _edge_pairs(make=make_pair_256), 16, 1024
    raise KeyError(name)


def _ref64(fam, p):
    """fp64 run of one pair, cached per (weights, pair): taps layer{l-1}_{0,1} for l in LAYERS, best / runner-up of every row, match list."""
    k = (fam, len(p.kp_q), len(p.kp_r), hash(p.kp_q.tobytes()), hash(p.desc_r.tobytes()))
    if k not in _REF:
        from oracle import lightglue_sift as lg
        from oracle import lightglue_superpoint as lsp
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
        sd, th = _family(fam)
        tsd = {n: torch.from_numpy(v) for n, v in sd.items()}
        nq, nr = len(p.kp_q), len(p.kp_r)
        if nq < 2 or nr < 2:
            _REF[k] = None
            return None
        taps = {}
        tq = torch.from_numpy
        if fam.startswith("sp_"):      # (image size = keypoint extent, as the engine's default)
            _, idx = lsp.match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.kp_r), tq(p.desc_r), filter_threshold=th, taps=taps, dtype=torch.float64)
        else:
            _, _, _, idx = lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r),
                                              tq(p.angle_r), taps=taps, filter_threshold=th, dtype=torch.float64)
        P = taps["scores"][0, :nq, :nr].numpy()
        top2 = -np.partition(-P, 1, axis=1)[:, :2]
        _REF[k] = {"layers": {l: (taps[f"layer{l - 1}_0"][0].numpy(), taps[f"layer{l - 1}_1"][0].numpy()) for l in LAYERS},
                   "best": top2[:, 0].copy(), "second": top2[:, 1].copy(), "idx": idx.numpy()}
    return _REF[k]


def _refs(fam, pairs):
    return [_ref64(fam, p) for p in pairs]


# ---------------------------------------------------------------------------------------------------------------- GPU side
def _staged(eng, pairs, zero_q=()):
    inp = eng.stage_inputs(pairs)
    for b in zero_q:
        inp["n_q"][b] = 0
    return inp


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


def _ordinary(refs, nvalid):
    """the pairs whose both sides hold >= 256 keypoints (the consistency bound compares grids on these: fp16 rounding of q, k, v averages over
    the keys, so a few-keypoint side has a larger error in any grid -- mode 5, whose operands carry 22 bits, shows no such growth)"""
    return [r if r is not None and min(nvalid[b]) >= 256 else None for b, r in enumerate(refs)]


def _head_d(eng, B, np_run, refs, nvalid, th=None):
    """max |P - P64| of the best score and runner-up over the valid rows (th given: only rows within 1 of log(th) in either arithmetic, as the
    calibration measures; all rows when th is 0 or no row comes that close)."""
    best = eng.debug_read("max0", B * np_run).reshape(B, np_run)
    second = eng.debug_read("max0b", B * np_run).reshape(B, np_run)
    d_all = d_near = 0.0
    near = 0
    L = np.log(th) if th else -np.inf
    for b, r in enumerate(refs):
        if r is None:
            continue
        n = nvalid[b][0]
        db = np.abs(best[b, :n].astype(np.float64) - r["best"])
        ds = np.abs(second[b, :n].astype(np.float64) - r["second"])
        d = np.maximum(db, ds)
        assert np.isfinite(best[b, :n]).all() and np.isfinite(d).all(), b
        d_all = max(d_all, float(d.max()))
        sel = np.maximum(best[b, :n], r["best"]) >= L - 1.0
        if sel.any():
            near += int(sel.sum())
            d_near = max(d_near, float(d[sel].max()))
    return d_all, (d_near if near else d_all)


def _layer_errors(eng, B, np_run, refs, nvalid):
    return _x_errors(eng.debug_read("x", B * 2 * np_run * 256).reshape(B, 2, np_run, 256), refs, nvalid)


def _x_errors(x, refs, nvalid):
    err = 0.0
    for b, r in enumerate(refs):
        if r is None:
            continue
        for s in (0, 1):
            n = nvalid[b][s]
            a = x[b, s, :n]
            assert np.isfinite(a).all(), (b, s)
            ref = r["cur"][s]
            err = max(err, float(np.abs(a - ref).max() / np.abs(ref).max()))
    return err


def _family_check(names, prec, grid, level):
    ffn = [n for n in names if n.startswith("k_ffn128")]
    bulk = grid in ("16x1024",) or grid.startswith("ragged")
    if prec in ("f32", "bf16_attn", "f32x3_bf16_attn"):
        assert not ffn and not any(n.startswith(("k_qkv", "k_attn_pw", "k_attn_f16x2")) for n in names), names
    elif bulk and prec != MODE5:
        assert ffn and all(n.rstrip(">").split(", ")[4] == str(level) for n in ffn), names
        if prec == HEADLINE:
            assert any(n.startswith("k_attn_pw") for n in names) and any(n.startswith("k_qkv") for n in names), names
        if grid == "ragged_walk":
            assert all(n.split(", ")[2] == "true" for n in ffn), names
        if grid == "ragged_onetile":
            assert all(n.split(", ")[2] == "false" for n in ffn), names
    elif not bulk:
        assert not ffn, names
    if prec == MODE5:
        assert any(n.startswith("k_attn_f16x2") for n in names), names
        assert not any(n.startswith(("k_attn_pw", "k_attn16", "k_attn_bf16", "k_qkv", "k_attn_f32")) for n in names), names


# ---------------------------------------------------------------------------------------------------------------- 1. per-layer and head error
CASES = [("f32", "1x1024", 3), ("f32", "16x1024", 3),
         ("bf16_attn", "2x512", 3), ("bf16_attn", "16x1024", 3),
         ("f32x3_bf16_attn", "4x512", 3), ("f32x3_bf16_attn", "16x1024", 3),
         ("f16x2_bf16_attn", "1x1024", 3), ("f16x2_bf16_attn", "16x1024", 3),
         (HEADLINE, "1x1024", 3), (HEADLINE, "2x512", 3), (HEADLINE, "4x512", 3), (HEADLINE, "16x1024", 3),
         (HEADLINE, "ragged_walk", 3), (HEADLINE, "ragged_onetile", 3),
         (HEADLINE, "4x512", 2), (HEADLINE, "16x1024", 2), (HEADLINE, "ragged_walk", 2), (HEADLINE, "ragged_onetile", 2),
         (HEADLINE, "4x512", 1), (HEADLINE, "16x1024", 1), (HEADLINE, "ragged_walk", 1), (HEADLINE, "ragged_onetile", 1),
         (MODE5, "1x1024", 3), (MODE5, "4x512", 3), (MODE5, "16x1024", 3), (MODE5, "ragged_walk", 3)]


@pytest.mark.parametrize("prec,grid,level", CASES)
def test_layers_and_head_against_fp64(prec, grid, level):
    from gisnav_amd.engine import PoseEngine
    sd, th = _family("margin_built")
    pairs, B, K = _grid(grid)
    zero_q = (1,) if grid.startswith("ragged") else ()
    refs = _refs("margin_built", pairs)
    for b in zero_q:
        refs[b] = None
    nvalid = [(0 if b in zero_q else len(p.kp_q), len(p.kp_r)) for b, p in enumerate(pairs)]
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=th)
    if level != 3:
        eng.set_ffn_products(level)
    if grid.startswith("ragged"):
        eng.lib.gn_debug_set_variant(eng.ctx, 31, 2 if grid == "ragged_walk" else 3)
    inp = _staged(eng, pairs, zero_q)
    row = {}
    for nl in LAYERS:
        eng.set_num_layers(nl)
        for r in refs:
            if r is not None:
                r["cur"] = r["layers"][nl]
        _match(eng, inp)
        x = eng.debug_read("x", B * 2 * K * 256).reshape(B, 2, K, 256)
        row[f"layer{nl}_rel"] = _x_errors(x, refs, nvalid)
        row[f"layer{nl}_rel_ordinary"] = _x_errors(x, _ordinary(refs, nvalid), nvalid)
    eng.set_certify("flag")
    (idx, score, n), names = _names(eng, inp)
    _family_check(names, prec, grid, level)
    row["head_dP"], _ = _head_d(eng, B, K, refs, nvalid)
    row["head_dP_ordinary"], _ = _head_d(eng, B, K, _ordinary(refs, nvalid), nvalid)
    bulk = grid in ("16x1024",) or grid.startswith("ragged")
    if level == 1 and not bulk:
        # a small grid runs no k_ffn128 (_family_check above) and keeps three products: bitwise the level-3 setting's results in the same context
        x1 = eng.debug_read("x", B * 2 * K * 256).copy()
        eng.set_ffn_products(3)
        (idx3, score3, n3), names3 = _names(eng, inp)
        _family_check(names3, prec, grid, 3)
        assert np.array_equal(x1.view(np.uint32), eng.debug_read("x", B * 2 * K * 256).view(np.uint32))
        assert np.array_equal(n, n3) and int(n.min()) > 0, (n, n3)
        for p in range(B):
            k = int(n[p])
            assert np.array_equal(idx[p, :k], idx3[p, :k]) and np.array_equal(score[p, :k].view(np.uint32), score3[p, :k].view(np.uint32)), p
    del eng
    # (small grids keep three products whatever the setting: they are compared with the level they ran on)
    ran = level if bulk else 3
    if level == 1 and bulk:
        # one more independent rounding of the same relative size: at most 2.0 x the level-2 case of the same grid, in this process, on the pairs
        # whose sides hold >= 256 keypoints.  The head's ratio is recorded only: a maximum over ~16 k rows, which the quadrature argument does not
        # bound as a ratio -- it is held to the absolute budget below
        two = _MEASURED.get((prec, 2, f"{grid}_set2"))
        if two is None:
            pytest.fail(NEEDS_PER_CASE)
        for nl in LAYERS:
            row[f"layer{nl}_rel_ordinary_over_lvl2"] = row[f"layer{nl}_rel_ordinary"] / two[f"layer{nl}_rel_ordinary"]
        row["head_dP_over_lvl2"] = row["head_dP"] / two["head_dP"]
    _MEASURED[(prec, ran, f"{grid}_set{level}")] = row
    _report(f"layers_{prec}_lvl{level}_{grid}", row)
    if level == 1 and bulk:
        for nl in LAYERS:
            assert row[f"layer{nl}_rel_ordinary"] <= LEVEL1_OVER_LEVEL2 * two[f"layer{nl}_rel_ordinary"], (nl, row, two)
    lb, hb = (FP16_LAYER[level], FP16_HEAD[level]) if prec == HEADLINE else BUDGET[prec]
    for nl in LAYERS:
        assert row[f"layer{nl}_rel"] <= lb, (nl, row)
    if hb is not None:
        assert row["head_dP"] <= hb, row
    if grid.startswith("ragged"):
        for b, (nq, nr) in enumerate(nvalid):
            if nq < 2 or nr < 2:
                assert n[b] == 0, (b, n[b])


# LightGlue on SuperPoint's 256-d features: the same measures and per-mode budgets (the fp16-attention mode on default-init weights: the
# *_DEFAULT_INIT ones) on both weight families (no identity blocks: every block's update counts), four grids.  k_prep_sp writes the residual stream and its hm16 planes directly; it does not go through timed_launch, so the
# launch table cannot list it -- its output is checked through the layer-1 residual.
SP_CASES = [(prec, grid, level, fam) for fam in ("sp_margin_built", "sp_default_init")
            for prec, level in (("f32", 3), ("f16x2_bf16_attn", 3), (HEADLINE, 3), (HEADLINE, 2), (HEADLINE, 1))
            for grid in ("sp_1x1024", "sp_4x1024", "sp_16x1024", "sp_ragged")]


@pytest.mark.parametrize("prec,grid,level,fam", SP_CASES)
def test_superpoint_layers_and_head_against_fp64(prec, grid, level, fam):
    from gisnav_amd.engine import PoseEngine
    sd, th = _family(fam)
    pairs, B, K = _grid(grid)
    ragged = grid == "sp_ragged"
    zero_q = (1,) if ragged else ()
    refs = _refs(fam, pairs)
    for b in zero_q:
        refs[b] = None
    nvalid = [(0 if b in zero_q else len(p.kp_q), len(p.kp_r)) for b, p in enumerate(pairs)]
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=th, feature="superpoint")
    if level != 3:
        eng.set_ffn_products(level)
    inp = _staged(eng, pairs, zero_q)
    row = {}
    for nl in LAYERS:
        eng.set_num_layers(nl)
        for r in refs:
            if r is not None:
                r["cur"] = r["layers"][nl]
        _match(eng, inp)
        row[f"layer{nl}_rel"] = _layer_errors(eng, B, K, refs, nvalid)
    eng.set_certify("flag")
    (idx, score, n), names = _names(eng, inp)
    _family_check(names, prec, "ragged" if ragged else grid[3:], level)
    row["head_dP"], _ = _head_d(eng, B, K, refs, nvalid)
    del eng
    _report(f"sp_layers_{fam}_{prec}_lvl{level}_{grid}", row)
    if prec == HEADLINE:
        lb, hb = (FP16_LAYER_DEFAULT_INIT[level], FP16_HEAD_DEFAULT_INIT[level]) if fam == "sp_default_init" else (FP16_LAYER[level], FP16_HEAD[level])
    else:
        lb, hb = BUDGET[prec]
    for nl in LAYERS:
        assert row[f"layer{nl}_rel"] <= lb, (nl, row)
    if hb is not None:
        assert row["head_dP"] <= hb, row
    for b, (nq, nr) in enumerate(nvalid):
        if nq < 2 or nr < 2:
            assert n[b] == 0, (b, n[b])


def test_error_is_consistent_across_the_grids_of_one_mode_and_level():
    """Within one mode and level the largest per-grid error is <= 4x the smallest (or both <= 1e-6): the grids differ by summation order only.
    Compared on the pairs whose sides hold >= 256 keypoints (_ordinary); the few-keypoint sides are held to the absolute budget above."""
    groups = {}
    for (prec, level, grid), row in _MEASURED.items():
        groups.setdefault((prec, level), []).append((grid, row))
    if not any(len(v) >= 2 for v in groups.values()):
        pytest.fail(NEEDS_PER_CASE)
    out = {}
    for (prec, level), rows in groups.items():
        if len(rows) < 2:
            continue
        for key in ("layer9_rel_ordinary", "head_dP_ordinary"):
            vals = {g: r[key] for g, r in rows}
            lo, hi = min(vals.values()), max(vals.values())
            out[f"{prec}_lvl{level}_{key}"] = {"max_over_min": hi / max(lo, 1e-30), **vals}
            assert hi <= 4.0 * lo or hi <= 1e-6, (prec, level, key, vals)
    _report("consistency", out)


@pytest.mark.parametrize("prec,level", [pytest.param(HEADLINE, 3, id=HEADLINE), pytest.param(HEADLINE, 2, id=HEADLINE + "-lvl2"),
                                        pytest.param(HEADLINE, 1, id=HEADLINE + "-lvl1"), pytest.param(MODE5, 3, id=MODE5)])
def test_edge_pairs_do_not_touch_their_neighbours_on_the_bulk_grid(prec, level):
    """(mode 5 has one block-tail level: set_ffn_products(1) on such a context launches no `..., 1>` kernel and changes no bit)"""
    from gisnav_amd.engine import PoseEngine
    sd, th = _family("margin_built")
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=prec, state_dict=sd, filter_threshold=th)
    if level != 3:
        eng.set_ffn_products(level)
    res = {}
    for lists in (2, 3):
        eng.lib.gn_debug_set_variant(eng.ctx, 31, lists)
        for ordinary in (False, True):
            pairs = _edge_pairs(ordinary)
            (idx, score, n), names = _names(eng, _staged(eng, pairs, () if ordinary else (1,)))
            _family_check(names, prec, "ragged_walk" if lists == 2 else "ragged_onetile", level)
            res[(lists, ordinary)] = (idx, score, n)
        a, b = res[(lists, False)], res[(lists, True)]
        assert a[2][1] == 0 and a[2][2] == 0, a[2]          # a side with < 2 keypoints: no match (kornia _no_match)
        for p in [0] + list(range(8, 16)):
            k = int(a[2][p])
            assert k == int(b[2][p]) and k > 0, (p, a[2][p], b[2][p])
            assert np.array_equal(a[0][p, :k], b[0][p, :k]) and np.array_equal(a[1][p, :k].view(np.uint32), b[1][p, :k].view(np.uint32)), (lists, p)
    if prec == MODE5:
        eng.set_ffn_products(1)
        (idx, score, n), names = _names(eng, _staged(eng, _edge_pairs(), (1,)))         # (the work lists are still the one-tile form's)
        _family_check(names, prec, "ragged_onetile", 3)
        assert not any(nm.startswith("k_ffn128") and nm.rstrip(">").split(", ")[4] == "1" for nm in names), names
        a = res[(3, False)]
        assert np.array_equal(n, a[2]), (n, a[2])
        for p in range(16):
            k = int(n[p])
            assert np.array_equal(idx[p, :k], a[0][p, :k]) and np.array_equal(score[p, :k].view(np.uint32), a[1][p, :k].view(np.uint32)), p
    del eng


@pytest.mark.parametrize("grid,level", [pytest.param("4x512", 3, id="4x512"), pytest.param("16x1024", 3, id="16x1024"),
                                        pytest.param("16x1024", 2, id="16x1024-lvl2"), pytest.param("16x1024", 1, id="16x1024-lvl1")])
def test_padding_slots_are_never_read(grid, level):
    """Descriptor slots past n hold U(0, 1e3), keypoint slots +-1e4 (a keypoint-extent read would move the normalisation): bitwise the zero-padded
    results, on a small grid and on the bulk grid (ragged sides, so that every pair has padding) at every block-tail level."""
    from gisnav_amd.engine import PoseEngine
    sd, th = _family("margin_built")
    _, B, K = _grid(grid)
    pairs = [make_pair(11500 + i, n_q=K - 37 - 61 * (i % 5), n_r=K - 29 - 43 * (i % 3)) for i in range(B)]
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    if level != 3:
        eng.set_ffn_products(level)
    clean = eng.stage_inputs(pairs)
    dirty = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in clean.items()}
    g = torch.Generator(device="cpu").manual_seed(5)
    for b, p in enumerate(pairs):
        for side, n in (("q", len(p.kp_q)), ("r", len(p.kp_r))):
            d, kp = dirty["desc_" + side], dirty["kpt_" + side]
            rest = d.shape[1] - n
            if rest <= 0:
                continue
            d[b, n:] = (torch.rand(rest, d.shape[2], generator=g) * 1e3).to(d.device)
            kp[b, n:] = ((torch.rand(rest, 4, generator=g) * 2 - 1) * 1e4).to(kp.device)
    a = _match(eng, clean)
    b = _match(eng, dirty)
    _family_check(_names(eng, dirty)[1], HEADLINE, grid, level)
    del eng
    assert np.array_equal(a[2], b[2]) and a[2].min() > 15
    for p in range(B):
        k = int(a[2][p])
        assert np.array_equal(a[0][p, :k], b[0][p, :k]) and np.array_equal(a[1][p, :k].view(np.uint32), b[1][p, :k].view(np.uint32)), p


# ---------------------------------------------------------------------------------------------------------------- 2. eps on every grid
def _fresh(grid):
    if grid == "16x1024":
        return [make_pair(13000 + i, n_q=1024 - 7 * (i % 4), n_r=1024 - 11 * (i % 3)) for i in range(16)]
    if grid == "8x1024":
        return [make_pair(13000 + i, n_q=1024 - 7 * (i % 4), n_r=1024 - 11 * (i % 3)) for i in range(8)]
    if grid == "1x1024":
        return [make_pair(13000, n_q=1024, n_r=1013)]
    if grid == "2x1024":
        return [make_pair(13000 + i, n_q=1024 - 7 * i, n_r=1013) for i in range(2)]
    if grid == "16x512_active":
        return [make_pair(13100 + i, n_q=512 - 5 * (i % 7), n_r=500 - 3 * (i % 5)) for i in range(16)]
    if grid == "ragged":
        return _edge_pairs()
    raise KeyError(grid)


@pytest.mark.parametrize("name", ["margin_built", "mid_margin", "default_init"])
def test_calibrated_eps_holds_on_every_grid_a_certified_call_runs(name):
    """calibrate_certify (headline mode, 16 x 1024 sample, safety 4, automatic level) -> d = max |P - P_fp64| over the entries the calibration
    measures, on fresh pairs, on each grid: 16 x 1024, 8 pairs (what a sub-stream group of set_substreams(2) runs), one and two pairs (bucket
    remainders), 16 pairs at set_active_kpts(512), the ragged batch; each block-tail level against its own eps; mode-5 arithmetic on 1, 4 and 16
    pairs against eps_mid.  Then "rerun": the certified lists equal fp64's except in pairs counted as f32-marginal."""
    from gisnav_amd.engine import PoseEngine
    sd, th = _family(name)
    cal_pairs = [make_pair(4460 + i, n_q=1024, n_r=1000) for i in range(16)]
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_ffn_products("auto")
    eng.set_certify_ladder(True)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    eps = {3: cal["eps_three_products"], 2: cal["eps_two_products"], 1: cal["eps_one_product"]}
    rows, fails = {}, []
    for grid in ("16x1024", "8x1024", "1x1024", "2x1024", "16x512_active", "ragged"):
        pairs = _fresh(grid)
        B = len(pairs)
        zero_q = (1,) if grid == "ragged" else ()
        refs = _refs(name, pairs)
        for b in zero_q:
            refs[b] = None
        nvalid = [(0 if b in zero_q else len(p.kp_q), len(p.kp_r)) for b, p in enumerate(pairs)]
        np_run = eng.set_active_kpts(512) if grid == "16x512_active" else eng.set_active_kpts(1024)
        inp = _staged(eng, pairs, zero_q)
        eng.set_certify("flag")
        for level in (3, 2, 1):
            eng.set_ffn_products(level)
            (_, _, _), names = _names(eng, inp)
            ffn = [n for n in names if n.startswith("k_ffn128")]
            bulk = bool(ffn)         # (what the launch table says: k_ffn128 ran)
            assert (bulk == (grid in ("16x1024", "ragged"))) and all(n.rstrip(">").split(", ")[4] == str(level) for n in ffn), (grid, names)
            _, d = _head_d(eng, B, np_run, refs, nvalid, th)
            rows[f"{grid}_lvl{level}"] = {"d": d, "eps": eps[level], "d_over_eps": d / eps[level]}
            if d > eps[level]:
                fails.append((grid, level, d, eps[level]))
            if not bulk:
                break            # small grids keep three products: the two-product setting runs the same kernels
        eng.set_ffn_products("auto")
        eng.set_certify("rerun")
        eng.certify_stats(reset=True)
        idx, score, n = _match(eng, inp)
        st = eng.certify_stats()
        diff_pairs = []
        for b, r in enumerate(refs):
            got = {(int(q), int(c)) for q, c in idx[b, : n[b]]}
            want = set() if r is None else {(int(q), int(c)) for q, c in r["idx"]}
            if got != want:
                diff_pairs.append(b)
        rows[f"{grid}_rerun"] = {"pairs_differing_from_fp64": len(diff_pairs), "f32_marginal_pairs": st["f32_marginal_pairs"], "rerun_pairs": st["rerun_pairs"]}
        assert len(diff_pairs) <= st["f32_marginal_pairs"], (grid, diff_pairs, st)
    eng.set_active_kpts(1024)
    eps_mid = cal["eps_mid"]
    del eng
    # the ladder's middle level: mode-5 arithmetic (a mode-5 context on the same weights) on 1, 4 and 16 pairs
    for B in (1, 4, 16):
        pairs = _fresh("16x1024")[:B]
        refs = _refs(name, pairs)
        nvalid = [(len(p.kp_q), len(p.kp_r)) for p in pairs]
        e5 = PoseEngine(0, max_batch=B, max_kpts=1024, precision=MODE5, state_dict=sd, filter_threshold=th)
        e5.set_certify("flag")
        (_, _, _), names = _names(e5, _staged(e5, pairs))
        assert any(n.startswith("k_attn_f16x2") for n in names), names
        _, d = _head_d(e5, B, 1024, refs, nvalid, th)
        del e5
        rows[f"mode5_{B}x1024_mid"] = {"d": d, "eps": eps_mid, "d_over_eps": d / eps_mid}
        if d > eps_mid:
            fails.append((f"mode5_{B}", "mid", d, eps_mid))
    rows["calibration"] = {k: v for k, v in cal.items()}
    _report(f"eps_on_grids_{name}", rows)
    assert not fails, (fails, rows)


# ---------------------------------------------------------------------------------------------------------------- 3. fused projection proof
def test_fused_projection_self_check_after_set_active_kpts_before_the_first_call():
    """set_active_kpts(512) before the first forward call of a 16 x 1024 headline context: the self-check still proves the fusion (it runs at the
    full padded size), and results on pairs of <= 512 keypoints are bitwise those with the fusion off (knob 32 = 0)."""
    from gisnav_amd.engine import PoseEngine
    sd, th = _family("margin_built")
    pairs = [make_pair(14000 + i, n_q=512 - 3 * i, n_r=500) for i in range(16)]
    got = {}
    for fused in (1, 0):
        eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=sd, filter_threshold=th)
        eng.lib.gn_debug_set_variant(eng.ctx, 32, fused)
        assert eng.set_active_kpts(512) == 512
        inp = eng.stage_inputs(pairs)
        got[fused] = _match(eng, inp)
        if fused:
            assert eng.fused_projection_status() == 1, eng.fused_projection_status()
        del eng
    a, b = got[1], got[0]
    assert np.array_equal(a[2], b[2]) and a[2].min() > 15
    for p in range(16):
        k = int(a[2][p])
        assert np.array_equal(a[0][p, :k], b[0][p, :k]) and np.array_equal(a[1][p, :k].view(np.uint32), b[1][p, :k].view(np.uint32)), p


def test_fused_projection_is_proved_again_when_the_block_tail_level_changes():
    """gn_set_ffn_products re-arms the self-check: after set_ffn_products(2) the next call proves the two-product instantiation as well, and after
    set_ffn_products(1) the one-product instantiation."""
    from gisnav_amd.engine import PoseEngine
    sd, th = _family("margin_built")
    pairs = [make_pair(9310 + i, n_q=1024, n_r=1000) for i in range(16)]
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    inp = eng.stage_inputs(pairs)
    _match(eng, inp)
    assert eng.fused_projection_status() == 1
    for level in (2, 1):
        eng.set_ffn_products(level)
        assert eng.fused_projection_status() == 1            # (still the last check's result until the next call runs the new one)
        eng.set_kernel_timing(400)
        _match(eng, inp)
        tab = {r["name"]: int(r["launches"]) for r in eng.kernel_table()}
        eng.set_kernel_timing(0)
        assert eng.fused_projection_status() == 1, level
        fused_tail = {k: v for k, v in tab.items() if k.startswith("k_ffn128") and k.rstrip(">").split(", ")[3] in ("1", "2")}
        assert sum(fused_tail.values()) == 17 and all(k.rstrip(">").split(", ")[4] == str(level) for k in fused_tail), (level, tab)
    del eng


# ---------------------------------------------------------------------------------------------------------------- 4. reload discards eps
def test_a_weight_reload_discards_a_calibrated_eps():
    """Calibrate on margin-built weights, load the low-margin ones without recalibrating, run 16 low-margin pairs certified: every pair goes to
    exact f32 (the old eps, ~7e-4, is far below these weights' ~5e-2), so the lists equal the f32 mode's.  A stated eps survives a reload."""
    from gisnav_amd.engine import PoseEngine
    sd0, th0 = _family("margin_built")
    sd1, _ = _family("low_margin")
    cal_pairs = [make_pair(4460 + i, n_q=1024, n_r=1000) for i in range(16)]
    pairs = [make_pair(4400 + i, n_q=1024 - 13 * (i % 5), n_r=1024 - 29 * (i % 3)) for i in range(16)]
    e32 = PoseEngine(0, max_batch=16, max_kpts=1024, precision="f32", state_dict=sd1, filter_threshold=0.0)
    want = _match(e32, e32.stage_inputs(pairs))
    del e32
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=sd0, filter_threshold=0.0)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    assert eng.certify_stats()["eps_source"] == "calibrated"
    eng.load_state_dict(sd1)
    assert eng.certify_stats()["eps_source"] == "discarded"
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    got = _match(eng, eng.stage_inputs(pairs))
    st = eng.certify_stats()
    _report("reload_discards_eps", {"stale_eps": cal["eps"], **{k: st[k] for k in ("pairs", "flagged_margin", "rerun_pairs", "f32_marginal_pairs")}})
    assert st["rerun_pairs"] == st["pairs"] == 16, st
    for p in range(16):
        a = {(int(q), int(c)) for q, c in got[0][p, : got[2][p]]}
        b = {(int(q), int(c)) for q, c in want[0][p, : want[2][p]]}
        assert a == b, p
    # a stated eps is the caller's: kept across a load
    eng.set_certify("rerun", eps=1.0)
    eng.load_state_dict(sd1)
    assert eng.certify_stats()["eps_source"] == "stated"
    # and a new calibration replaces the discarded one
    eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    assert eng.certify_stats()["eps_source"] == "calibrated"
    del eng

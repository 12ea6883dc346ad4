"""LightGlue point pruning (width_confidence > 0), the parts that need no GPU:

  1. the CPU restatement (tests/width_pruning_ref.py) with pruning off IS oracle.lightglue_sift's forward, and with min_kpts >= N it gives the same
     matches and all-ones prune vectors;
  2. known answer: identity blocks keep x constant over the layers, so every z_i = w_i . x0 + b_i and the kept sets, the prune vectors and the
     remapped match indices can be worked out in numpy;
  3. the mirrors' argument rules (LightGlueMatcher, PoseNode, check_width_pruning), before any device work;
  4. gn_set_width_pruning / gn_get_width_pruning / gn_get_prune are declared in the header and exported by the built library.

kornia is not importable here: the restatement follows the public kornia 0.7.2 / cvg LightGlue source, parity with it is unpinned.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import width_pruning_ref as wp  # noqa: E402
from gisnav_amd.synthetic import make_pair, make_pair_256  # noqa: E402
from gisnav_amd.weights import synthetic_state_dict  # noqa: E402
from oracle import lightglue_sift as lg  # noqa: E402
from oracle import lightglue_superpoint as lsp  # noqa: E402


@pytest.fixture(scope="module")
def pair():
    return make_pair(31000, n_q=150, n_r=131)


def _oracle_idx(sd, p):
    tq = torch.from_numpy
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    _, _, sc, idx = lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r), tq(p.angle_r))
    return idx.numpy(), sc.numpy()[:, 0]


def test_helper_without_pruning_is_the_oracle_forward(pair):
    sd = synthetic_state_dict(0)
    want_idx, want_sc = _oracle_idx(sd, pair)
    assert len(want_idx) > 20
    off = wp.forward(sd, wp.sift_inputs(pair), width_confidence=-1.0)
    assert np.array_equal(off["idx"], want_idx) and np.array_equal(off["score"], want_sc)          # exactly: the same operations in the same order
    assert (off["prune0"] == lg.N_LAYERS).all() and (off["prune1"] == lg.N_LAYERS).all()          # kornia without pruning: n_layers everywhere
    for mk in (150, 4096):                                                                        # on, but no side is ever above min_kpts
        on = wp.forward(sd, wp.sift_inputs(pair), width_confidence=0.99, min_kpts=mk)
        assert np.array_equal(on["idx"], want_idx) and np.array_equal(on["score"], want_sc)
        assert (on["prune0"] == 1).all() and (on["prune1"] == 1).all() and not on["kept"]
    # margin-built weights bias matchability to +10: pruning at the default confidence fires (min_kpts 0) and keeps every point
    all_kept = wp.forward(sd, wp.sift_inputs(pair), width_confidence=0.99, min_kpts=0)
    assert np.array_equal(all_kept["idx"], want_idx) and (all_kept["prune0"] == lg.N_LAYERS).all() and len(all_kept["kept"]) == 2 * (lg.N_LAYERS - 1)


def test_helper_256d_without_pruning_is_the_oracle_forward():
    p = make_pair_256(31100, n_q=140, n_r=120)
    sd = synthetic_state_dict(0, feature="superpoint")
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    tq = torch.from_numpy
    sc, idx = lsp.match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.kp_r), tq(p.desc_r), filter_threshold=0.1)
    off = wp.forward(sd, wp.sp_inputs(p), "superpoint", filter_threshold=0.1, width_confidence=-1.0)
    assert len(idx) > 20 and np.array_equal(off["idx"], idx.numpy()) and np.array_equal(off["score"], sc.numpy()[:, 0])


def test_known_answer_with_identity_blocks(pair):
    """identity_blocks zeroes every ffn.3: x stays input_proj(rootsift(desc)) through all layers, so z_i = w_i . x0 + b_i."""
    sd = synthetic_state_dict(0, identity_blocks=True)
    wc, mk = 0.9, 60
    t = wp.tau(wc)
    inp = wp.sift_inputs(pair)
    x0 = [torch.nn.functional.linear(inp[k][0], torch.from_numpy(sd["input_proj.weight"]), torch.from_numpy(sd["input_proj.bias"])).numpy().astype(np.float64)
          for k in ("desc0", "desc1")]
    rng = np.random.default_rng(5)
    plan = {1: 0.7, 2: 1.0, 5: 0.5}          # layer -> fraction of the CURRENT rows to keep (1.0: the layer fires and drops nothing); others keep all
    for i in range(lg.N_LAYERS):
        sd[f"log_assignment.{i}.matchability.weight"] = rng.normal(size=(1, 256)).astype(np.float32)
        sd[f"log_assignment.{i}.matchability.bias"] = np.array([50.0], np.float32)
    # by hand: walk the layers in numpy, placing each planned bias in the middle of the gap at the planned quantile of the pooled current rows
    ind = [np.arange(len(x0[0])), np.arange(len(x0[1]))]
    prune = [np.ones(len(x0[0]), np.int32), np.ones(len(x0[1]), np.int32)]
    for i in range(lg.N_LAYERS - 1):
        w = sd[f"log_assignment.{i}.matchability.weight"][0].astype(np.float64)
        up = [s for s in (0, 1) if len(ind[s]) > mk]
        if i in plan and plan[i] < 1.0:
            u = np.sort(np.concatenate([x0[s][ind[s]] @ w for s in up]))
            j = int(round((1.0 - plan[i]) * len(u))) - 1
            assert u[j + 1] - u[j] > 1e-4                  # the decision is far from f32 rounding of z (~1e-6)
            sd[f"log_assignment.{i}.matchability.bias"] = np.array([t - 0.5 * (u[j] + u[j + 1])], np.float32)
        b = float(sd[f"log_assignment.{i}.matchability.bias"][0])
        for s in up:
            ind[s] = ind[s][x0[s][ind[s]] @ w + b > t]
            prune[s][ind[s]] += 1
    assert len(ind[0]) < 150 * 0.75 * 0.55 and min(len(ind[0]), len(ind[1])) >= 2
    got = wp.forward(sd, inp, width_confidence=wc, min_kpts=mk)
    assert np.array_equal(got["prune0"], prune[0]) and np.array_equal(got["prune1"], prune[1])
    assert got["prune0"].max() > got["prune0"].min() >= 2      # layer 0 fired for everybody, later layers dropped some
    last = {s: max(k[0] for k in got["kept"] if k[1] == s) for s in (0, 1)}
    assert all(np.array_equal(got["kept"][(last[s], s)].numpy(), ind[s]) for s in (0, 1))
    # the head on the kept rows, indices remapped by hand
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    xs = [torch.from_numpy(x0[s][ind[s]].astype(np.float32))[None] for s in (0, 1)]
    scores, _ = lg.match_assignment(tsd, lg.N_LAYERS - 1, xs[0], xs[1])
    m0, _, ms0, _ = lg.filter_matches(scores, lg.FILTER_THRESHOLD)
    m0, ms0 = m0[0].numpy(), ms0[0].numpy()
    v = m0 > -1
    want = np.stack([ind[0][v], ind[1][m0[v]]], -1)
    assert v.sum() >= 5 and np.array_equal(got["idx"], want) and (np.diff(got["idx"][:, 0]) > 0).all()
    assert np.abs(got["score"] - ms0[v]).max() < 1e-5          # (x0 went through f64 and back: same values, the helper's head is the same code)
    full = np.full(150, -1, np.int64)
    full[want[:, 0]] = want[:, 1]
    assert np.array_equal(got["matches0"].numpy(), full)       # matches0 over the ORIGINAL query keypoints, -1 for the pruned ones


def test_forced_keep_replays_decisions(pair):
    inps = [wp.sift_inputs(pair)]
    sd, half = wp.build_pruning_weights(inps, prune_layers=(1, 4), width_confidence=0.99, min_kpts=50, weight_scale=100.0, keep_range=(0.5, 0.8))
    assert all(h is not None and h > 1e-3 for h in half.values())
    a = wp.forward(sd, inps[0], width_confidence=0.99, min_kpts=50, dtype=torch.float64)
    assert set(k[0] for k in a["kept"] if len(a["kept"][k]) < len(a["present"][k])) == {1, 4}
    forced = {k: v.numpy() for k, v in a["kept"].items()}
    sd2 = dict(sd)      # other biases would decide otherwise; the replay does not ask them
    for i in (1, 4):
        sd2[f"log_assignment.{i}.matchability.bias"] = np.array([30.0], np.float32)
    b = wp.forward(sd2, inps[0], width_confidence=0.99, min_kpts=50, dtype=torch.float64, forced_keep=forced)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["prune0"], b["prune0"]) and np.array_equal(a["prune1"], b["prune1"])
    for s, pv, n in ((0, a["prune0"], 150), (1, a["prune1"], 131)):      # the per-layer kept sets follow from the final prune vector
        before = [n] + [c[s] for c in a["counts"][:-1]]
        rec = wp.kept_from_prune(pv, n, before, 50, lg.N_LAYERS)
        assert rec.keys() == {k[0] for k in a["kept"] if k[1] == s}
        assert all(np.array_equal(rec[i], a["kept"][(i, s)].numpy()) for i in rec)


def test_zero_kept_side_reports_no_match(pair):
    sd = synthetic_state_dict(0)
    sd["log_assignment.2.matchability.bias"] = np.array([-30.0], np.float32)
    r = wp.forward(sd, wp.sift_inputs(pair), width_confidence=0.99, min_kpts=0)
    assert len(r["idx"]) == 0 and r["counts"][-1] == (0, 0) and (r["prune0"] == 3).all()      # layers 0 and 1 kept everybody, layer 2 nobody


def test_mirror_argument_rules():
    from gisnav_amd.engine import check_width_pruning
    from gisnav_amd.matcher import LightGlueMatcher
    from gisnav_amd.pose_node import PoseNode
    sd = synthetic_state_dict(0)
    m = LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": 0.99, "pruning_min_kpts": 1024}, state_dict=sd)
    assert m._width_conf == pytest.approx(0.99) and m._prune_min_kpts == 1024 and "pruning_min_kpts" not in m.params
    assert LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": 0.5}, state_dict=sd)._prune_min_kpts is None
    assert LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": -1}, state_dict=sd)._width_conf == -1.0
    LightGlueMatcher("sift", params={"depth_confidence": 0, "width_confidence": 0.9}, state_dict=sd, precision="f16x2_f16_attn", certify=False)
    with pytest.raises(ValueError, match="certify=False"):
        LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": 0.9}, state_dict=sd, precision="f16x2_f16_attn")
    for bad in ({"depth_confidence": 0.95, "width_confidence": -1}, {"depth_confidence": 0.95, "width_confidence": 0.99}, {}):
        with pytest.raises(NotImplementedError):
            LightGlueMatcher("sift", params=bad, state_dict=sd)
    for wc in (1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            check_width_pruning(wc)
        with pytest.raises(ValueError):
            LightGlueMatcher("sift", params={"depth_confidence": -1, "width_confidence": wc}, state_dict=sd)
    for wc in (-1.0, 0.0, 0.5, 0.99, np.float32(0.9)):
        check_width_pruning(wc)
        check_width_pruning(wc, 0)
    with pytest.raises(ValueError):
        check_width_pruning(0.9, -1)
    with pytest.raises(TypeError):
        check_width_pruning(0.9, 10.5)
    with pytest.raises(TypeError):
        check_width_pruning("0.9")
    # PoseNode refuses before it creates an engine (no device here)
    with pytest.raises(ValueError, match="certify=False"):
        PoseNode(sd, width_confidence=0.99, precision="f16x2_f16_attn")
    with pytest.raises(ValueError):
        PoseNode(sd, width_confidence=1.0)
    with pytest.raises(ValueError):
        PoseNode(sd, width_confidence=0.9, pruning_min_kpts=-5)


def test_symbols_declared_and_exported():
    from gisnav_amd import build, _lib
    hdr = open(os.path.join(ROOT, "include", "gisnav_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gn_set_width_pruning", "gn_get_width_pruning", "gn_get_prune"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in include/gisnav_amd.h"
        assert hasattr(raw, name), f"{name} is not exported by the built library"
        assert name in _lib.SIGNATURES

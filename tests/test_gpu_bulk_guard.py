"""GPU tests (-m gpu) of the fp16 range guard (ovf_track / ovf_commit, gn_common.h) in the BULK kernels: k_ffn128 at its three sites (the post-GELU
hidden value, the published residual rows, the q | k | V^T of the fused projection), k_qkv and k_attn_pw, on every block-tail level.

tests/test_gpu_round3.py raises the guard on 2 x 256 contexts, which run the small-grid kernels (gn_gemm_p2, gn_ffn, gn_skinny).  Levels 2 and 1 of
k_ffn128 publish fp16 high terms only: nothing carries what a saturated high term lost, so on the grid the benchmark runs the guard is the only thing
between an out-of-range activation and finite garbage.  Here, 4 x 512 with the bulk kernels forced (test_gpu_round6._forced_headline), the
fp16-attention mode, synthetic_state_dict(0) plus one change that leaves fp16's range (65504) at one site and leaves the f32 oracle's matches alone:

  * hidden: layer 3's ffn.1 (LayerNorm) weight and bias x 1e5, ffn.3's weight x 1e-5 -- the post-GELU hidden value reaches ~3e5;
  * stream: layer 3's self-block ffn.3 weight and bias x 1e8 -- the residual stream reaches ~1.8e6 from layer 4 on (f32 itself loses the later
    updates there: no arithmetic is a fair reference, the case is flag-only);
  * qk:     q x 1e6 and k x 1e-6 in every Wqkv (test_gpu_round3.py's construction) -- the scores are unchanged, q no longer fits fp16.

Per change and level in (3, 2, 1): guard "flag" reports the guard raised, zero matches and ok == 0 everywhere, and the context then runs the unmodified
weights with the guard silent and the bits of a fresh context; guard "sync" (hidden, qk) counts one fallback and returns match lists within 2 % symmetric
difference of the oracle's; unmodified weights leave the guard silent.  Whenever the guard is silent the lists must be within 2 % of the oracle's.
Under set_certify("rerun") with level 1's calibrated eps the certificate does not vouch for a pair of a call whose guard word is raised.
"""
import numpy as np
import pytest
import torch

from conftest import oracle_match
from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import synthetic_state_dict
from tests.test_gpu_round6 import HEADLINE, SAFETY, _forced_headline

pytestmark = pytest.mark.gpu
B, K = 4, 512
LEVELS = (3, 2, 1)
_CACHE = {}


def _pairs():
    if "pairs" not in _CACHE:
        _CACHE["pairs"] = [make_pair(77200 + i, n_q=512 - 31 * i, n_r=500) for i in range(B)]
    return _CACHE["pairs"]


def _weights(change):
    sd = dict(synthetic_state_dict(0))
    if change == "hidden":
        for blk in ("self_attn", "cross_attn"):
            for leaf in ("ffn.1.weight", "ffn.1.bias"):
                sd[f"transformers.3.{blk}.{leaf}"] = sd[f"transformers.3.{blk}.{leaf}"] * np.float32(1.0e5)
            sd[f"transformers.3.{blk}.ffn.3.weight"] = sd[f"transformers.3.{blk}.ffn.3.weight"] * np.float32(1.0e-5)
    elif change == "stream":
        for leaf in ("ffn.3.weight", "ffn.3.bias"):
            sd[f"transformers.3.self_attn.{leaf}"] = sd[f"transformers.3.self_attn.{leaf}"] * np.float32(1.0e8)
    elif change == "qk":
        for i in range(9):
            for leaf, shape in (("weight", (4, 64, 3, 256)), ("bias", (4, 64, 3))):
                key = f"transformers.{i}.self_attn.Wqkv.{leaf}"
                w = sd[key].copy().reshape(shape)
                w[:, :, 0] *= np.float32(1.0e6); w[:, :, 1] *= np.float32(1.0e-6)
                sd[key] = w.reshape(sd[key].shape)
    else:
        assert change == "plain", change
    return sd


def _oracle(change):
    """The f32 oracle's match lists of the four pairs on one weight set, computed once."""
    if ("oracle", change) not in _CACHE:
        tsd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _weights(change).items()}
        refs = [oracle_match(tsd, p)[3].numpy() for p in _pairs()]
        assert all(len(r) > 50 for r in refs), [len(r) for r in refs]
        _CACHE[("oracle", change)] = refs
    return _CACHE[("oracle", change)]


def _close_to_oracle(idx, n, change):
    for b, oidx in enumerate(_oracle(change)):
        got = {(int(q), int(c)) for q, c in idx[b, : int(n[b])]}
        want = {(int(q), int(c)) for q, c in oidx}
        assert len(got ^ want) <= 0.02 * len(want), (change, b, len(got ^ want), len(want))


class _Forced:
    """A 4 x 512 fp16-attention context on the bulk kernels and one block-tail level (the knobs are put back when it goes)."""

    def __init__(self, sd, level, guard="flag"):
        from gisnav_amd.engine import PoseEngine
        self.eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, guard=guard)
        self.level = level

    def __enter__(self):
        _forced_headline(self.eng, True)
        self.eng.set_ffn_products(self.level)
        return self.eng

    def __exit__(self, *exc):
        _forced_headline(self.eng, False)
        del self.eng


def _run(eng, inp):
    eng.set_kernel_timing(400)
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table()]
    eng.set_kernel_timing(0)
    return idx.cpu().numpy().copy(), score.cpu().numpy().copy(), n.cpu().numpy().copy(), names


def _bulk_ran(names, level, only=True):
    """k_ffn128<ABL, COMP, LOOP, QKV, PROD> on this level (only=True: on no other), k_qkv and k_attn_pw are in the launch table."""
    lv = [n.rstrip(">").split(", ")[4] for n in names if n.startswith("k_ffn128")]
    assert str(level) in lv and (not only or all(v == str(level) for v in lv)), names
    assert any(n.startswith("k_qkv") for n in names) and any(n.startswith("k_attn_pw") for n in names), names


def _fresh(level):
    """Unmodified weights on a fresh context: (idx, score, n, guard status)."""
    if ("fresh", level) not in _CACHE:
        with _Forced(_weights("plain"), level) as eng:
            idx, score, n, names = _run(eng, eng.stage_inputs(_pairs()))
            st = eng.guard_status()
        _bulk_ran(names, level)
        _CACHE[("fresh", level)] = (idx, score, n, st)
    return _CACHE[("fresh", level)]


def _same_bits(a, b):
    assert np.array_equal(a[2], b[2]), (a[2], b[2])
    for p in range(B):
        k = int(a[2][p])
        assert np.array_equal(a[0][p, :k], b[0][p, :k]) and np.array_equal(a[1][p, :k].view(np.uint32), b[1][p, :k].view(np.uint32)), p


@pytest.mark.parametrize("level", LEVELS)
def test_unmodified_weights_leave_the_guard_silent_and_match_the_oracle(level):
    idx, score, n, st = _fresh(level)
    assert st == (False, 0), st
    assert int(n.min()) > 50, n
    _close_to_oracle(idx, n, "plain")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("change", ["hidden", "stream", "qk"])
def test_guard_flag_reports_no_match_and_the_context_recovers(change, level):
    pairs = _pairs()
    with _Forced(_weights(change), level) as eng:
        inp = eng.stage_inputs(pairs)
        idx, score, n, names = _run(eng, inp)
        raised, _ = eng.guard_status()
        _bulk_ran(names, level)
        if not raised and change != "stream":          # a case whose guard stays silent must still be right
            _close_to_oracle(idx, n, change)
        assert raised, (change, level, n.tolist())
        assert (n == 0).all(), n
        out = eng.estimate(inp, K_MATRIX)
        torch.cuda.synchronize()
        assert eng.guard_status()[0]
        assert (out["ok"].cpu().numpy() == 0).all() and (out["n_match"].cpu().numpy() == 0).all(), (out["ok"], out["n_match"])
        # the same context on the unmodified weights: guard silent, the bits of a fresh context
        eng.load_state_dict(_weights("plain"))
        again = _run(eng, inp)
        assert not eng.guard_status()[0]
        _bulk_ran(again[3], level)
    _same_bits(again, _fresh(level))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("change", ["hidden", "qk"])
def test_guard_sync_counts_one_fallback_and_returns_the_oracles_matches(change, level):
    with _Forced(_weights(change), level, guard="sync") as eng:
        idx, score, n, names = _run(eng, eng.stage_inputs(_pairs()))
        st = eng.guard_status()
    _bulk_ran(names, level, only=False)               # (the launch table holds the fallback's kernels as well)
    _close_to_oracle(idx, n, change)                  # raised: the re-run's lists; silent: the fast kernels' -- right either way
    assert st[1] == 1, st


def test_certificate_does_not_vouch_for_a_call_whose_guard_word_is_raised():
    """Level 1, eps calibrated on the unmodified weights (the hidden change leaves the f32 scores alone; a sample that leaves the fp16 range cannot be
    calibrated on, and a reload discards a calibrated eps: it is stated again).  "flag": every pair carries flag 2 (fp16 range); "rerun": every pair
    is re-run in exact f32 and the lists are an exact-f32 context's."""
    pairs = _pairs()
    hidden = _weights("hidden")
    from gisnav_amd.engine import PoseEngine
    e32 = PoseEngine(0, max_batch=B, max_kpts=K, precision="f32", state_dict=hidden)
    want = _run(e32, e32.stage_inputs(pairs))
    del e32
    _close_to_oracle(want[0], want[2], "hidden")
    with _Forced(_weights("plain"), 1) as eng:
        cal = eng.calibrate_certify(eng.stage_inputs([make_pair(77260 + i, n_q=500, n_r=490) for i in range(B)]), safety=SAFETY)
        assert 0.0 < cal["eps"] < 0.1, cal
        inp = eng.stage_inputs(pairs)
        eng.load_state_dict(hidden)
        eng.set_certify("flag", eps=cal["eps"])
        idx, score, n, names = _run(eng, inp)
        _bulk_ran(names, 1)
        assert eng.guard_status()[0]
        flags = eng.uncertain(B)
        assert (flags == 2).all(), flags.tolist()
        assert (n == 0).all(), n
        eng.set_certify("rerun", eps=cal["eps"])
        eng.certify_stats(reset=True)
        got = _run(eng, inp)
        st = eng.certify_stats()
    assert st["pairs"] == B and st["flagged_fp16_range"] == B and st["rerun_pairs"] == B, st
    assert np.array_equal(got[2], want[2]) and all(np.array_equal(got[0][p, : got[2][p]], want[0][p, : want[2][p]]) for p in range(B)), (got[2], want[2])

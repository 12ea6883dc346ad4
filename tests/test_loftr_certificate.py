"""LoFTR's coarse-match certificate, on the CPU: the rule and `get_coarse_match` restated in numpy on a confidence
matrix, the proof checked on the oracle's own matrices, hand-built corner cases, and the wrapper's argument checks.

The rule (thr = 0.2, border = 2, eps = the bound on |conf_fast - conf_f32| entry-wise).  A cell is interior when it lies at least `border`
cells from every edge of the coarse grid.  A pair is flagged when
  (a) an interior row has best >= thr - eps and best - runner-up <= 2 eps, or
  (b) the same for an interior column (best and runner-up over ALL L rows), or
  (c) an interior row's best lies within eps of thr.
The runner-up counts multiplicity (a tie has gap 0)."""
import numpy as np
import pytest
import torch

from oracle import loftr as lf

THR, BORDER = 0.2, 2
_cache = {}


def interior(hc, wc, border=BORDER):
    y, x = np.divmod(np.arange(hc * wc), wc)
    return (y >= border) & (y < hc - border) & (x >= border) & (x < wc - border)


def top2(conf, axis):
    """(best, runner-up counting multiplicity) along `axis`."""
    s = np.sort(conf, axis=axis)
    return np.take(s, -1, axis=axis), np.take(s, -2, axis=axis)


def flagged(conf, hc, wc, eps, thr=THR, border=BORDER):
    inn = interior(hc, wc, border)
    rb, rs = top2(conf, 1)
    cb, cs = top2(conf, 0)
    a = inn & (rb >= thr - eps) & (rb - rs <= 2 * eps)
    b = inn & (cb >= thr - eps) & (cb - cs <= 2 * eps)
    c = inn & (np.abs(rb - thr) <= eps)
    return bool(a.any() or b.any() or c.any())


def coarse_match(conf, hc, wc, thr=THR, border=BORDER):
    """get_coarse_match: (i_ids, j_ids), ascending i, the first j of a row's mask."""
    inn = interior(hc, wc, border)
    mask = (conf > thr) & inn[:, None] & inn[None, :] & (conf == conf.max(1, keepdims=True)) & (conf == conf.max(0, keepdims=True))
    i = np.nonzero(mask.any(1))[0]
    return i, mask.argmax(1)[i]


def _oracle_conf(seed, h, w):
    key = (seed, h, w)
    if key not in _cache:
        if "sd" not in _cache:
            _cache["sd"] = lf.synthetic_state_dict(0)
        taps = {}
        out = lf.loftr_forward(_cache["sd"], *lf.synthetic_pair(seed, h, w), taps=taps, fine=False)
        conf = taps["conf_matrix"][0].numpy()
        i, j = coarse_match(conf, h // 8, w // 8)
        assert np.array_equal(i, out["i_ids"].numpy()) and np.array_equal(j, out["j_ids"].numpy())      # the restatement is the oracle's
        _cache[key] = conf
    return _cache[key]


@pytest.mark.parametrize("h,w", [(64, 96), (128, 160)])
def test_unflagged_means_identical_match_lists(h, w):
    """Q = the oracle's f32 confidence matrix, P = Q + uniform noise in +-eps: whenever P passes the certificate at eps, P and Q have the
    same match list.  Over the grid of eps both outcomes occur (else the statement would be empty)."""
    hc, wc = h // 8, w // 8
    outcomes = set()
    for seed in range(1, 7):
        q = _oracle_conf(seed, h, w).astype(np.float64)
        qi, qj = coarse_match(q, hc, wc)
        assert len(qi) > 0
        rs = np.random.default_rng(100 + seed)
        for eps in np.logspace(-5, -1, 13):
            p = q + rs.uniform(-eps, eps, q.shape)
            f = flagged(p, hc, wc, eps)
            outcomes.add(f)
            if not f:
                pi, pj = coarse_match(p, hc, wc)
                assert np.array_equal(pi, qi) and np.array_equal(pj, qj), (seed, eps)
    assert outcomes == {True, False}


def _quiet(hc=6, wc=7):
    """A matrix that passes at eps = 1e-3: every row and column has one clear entry far from thr."""
    L = hc * wc
    conf = np.full((L, L), 1e-4)
    conf[np.arange(L), (np.arange(L) * 5 + 3) % L] = 0.6        # (5 and L = 42 are coprime: a permutation)
    assert not flagged(conf, hc, wc, 1e-3)
    return conf, hc, wc


def test_a_tie_flags():
    conf, hc, wc = _quiet()
    i = 2 * wc + 3                                               # interior
    assert interior(hc, wc)[i]
    j = int(conf[i].argmax())
    conf[i, (j + 1) % conf.shape[1]] = conf[i, j]                # two equal bests in one interior row
    assert flagged(conf, hc, wc, 0.0) and flagged(conf, hc, wc, 1e-3)


def test_best_within_eps_of_thr_flags():
    conf, hc, wc = _quiet()
    i = 3 * wc + 2
    j = int(conf[i].argmax())
    for v in (THR + 5e-4, THR - 5e-4):
        c = conf.copy()
        c[i, j] = v
        assert flagged(c, hc, wc, 1e-3) and not flagged(c, hc, wc, 1e-4)


def test_a_near_tie_in_border_rows_and_columns_does_not_flag():
    conf, hc, wc = _quiet()
    inn = interior(hc, wc)
    bi = [1, wc + 1]                                             # row 0 and column 1 of the grid: border cells
    bj = [int(np.nonzero(~inn)[0][-1]), int(np.nonzero(~inn)[0][-2])]
    assert not inn[bi].any() and not inn[bj].any()
    conf[bi[0]] = 1e-4
    conf[:, bj[0]] = 1e-4
    conf[:, bj[1]] = 1e-4
    conf[bi[0], bj[0]] = 0.5
    conf[bi[0], bj[1]] = 0.5 + 1e-6                              # a near-tie in a border row, in border columns ...
    conf[bi[1], bj[0]] = 0.5 - 1e-6                              # ... and in a border column
    assert not flagged(conf, hc, wc, 1e-3)
    assert flagged(conf, hc, wc, 1e-3, border=0)                 # (the same matrix without the exemption is flagged)


def test_rerun_needs_split_arithmetic_and_modes_are_checked():
    from gisnav_amd import _lib
    from gisnav_amd.loftr import LoFTR
    sd = {"x": torch.zeros(1)}
    with pytest.raises(_lib.GnError, match="split_fp16"):
        LoFTR(state_dict=sd, arithmetic="exact_f32", certify="rerun")
    with pytest.raises(_lib.GnError, match="certify"):
        LoFTR(state_dict=sd, arithmetic="split_fp16", certify="sometimes")
    with pytest.raises(_lib.GnError, match="certify_eps"):
        LoFTR(state_dict=sd, arithmetic="split_fp16", certify="flags", certify_eps=1.5)
    for ok in (dict(), dict(certify=False), dict(certify="flags"), dict(certify="flags", arithmetic="split_fp16"), dict(certify="rerun", arithmetic="split_fp16", certify_eps=1e-3)):
        assert LoFTR(state_dict=sd, **ok)._ctx is None

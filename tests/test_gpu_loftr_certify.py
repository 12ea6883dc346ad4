"""LoFTR's coarse-match certificate on the MI355X (gn_loftr_set_certify / gn_loftr_calibrate_certify, `LoFTR(certify=...)`).
No CPU oracle forward: the references are an exact-f32 context, an uncertified split-fp16 context and fp64 numpy on the GPU's own "sim".

Shapes: 64x96 B = 2 (L = 96 < 128, Lp = 128: rows_per = 3, every column split used), 136x200 B = 3 (L = 425, Lp = 512: L no multiple of 128 or
256, a ragged last column split), 256x336 B = 2 (L = 1344 > 1280: the row kernels' 256 x kLfU loop runs a second trip).  All pairs are
`synthetic_pair(seed, h, w)` on `synthetic_state_dict(0)`.  The rule is restated in tests/test_loftr_certificate.py.

Measured figures go to test_reports/loftr_certify.json (git-ignored), stamped with the loaded library's digest."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import loftr as lf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, BORDER = 0.2, 2
TEMPERATURE = float(np.float32(0.1))        # the kernels' temperature is the f32 number 0.1f
KEYS = ("keypoints0", "keypoints1", "confidence", "i_ids", "j_ids")
SHAPES = {(64, 96): [[1, 2]], (136, 200): [[1, 2, 3], [4, 5, 6]], (256, 336): [[1, 2]]}
_cache = {}


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "loftr_certify.json")
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


# ---- the rule, in numpy (tests/test_loftr_certificate.py checks this restatement against the proof)
def _interior(hc, wc):
    y, x = np.divmod(np.arange(hc * wc), wc)
    return (y >= BORDER) & (y < hc - BORDER) & (x >= BORDER) & (x < wc - BORDER)


def _top2(conf, axis):
    s = np.sort(conf, axis=axis)
    return np.take(s, -1, axis=axis), np.take(s, -2, axis=axis)


def _flagged(stats, eps):
    inn, rb, rs, cb, cs = stats
    return bool((inn & (((rb >= THR - eps) & (rb - rs <= 2 * eps)) | ((cb >= THR - eps) & (cb - cs <= 2 * eps)) | (np.abs(rb - THR) <= eps))).any())


def _critical_eps(stats):
    """The smallest eps that flags (the flag is monotone in eps), by bisection to 1e-4 relative."""
    lo, hi = 0.0, 1.0
    assert _flagged(stats, hi)
    if _flagged(stats, lo):
        return 0.0
    while hi - lo > 1e-4 * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if _flagged(stats, mid) else (mid, hi)
    return hi


# ---- inputs and matchers
def _sd():
    if "sd" not in _cache:
        _cache["sd"] = lf.synthetic_state_dict(0)
    return _cache["sd"]


def _batch(seeds, h, w, noise=0.01, scale=None):
    key = ("batch", tuple(seeds), h, w, noise, None if scale is None else tuple(scale))
    if key not in _cache:
        ps = [lf.synthetic_pair(s, h, w, noise=noise) for s in seeds]
        if scale is not None:
            ps = [(a * k, b * k) for (a, b), k in zip(ps, scale)]
        _cache[key] = {"image0": torch.stack([p[0] for p in ps])[:, None].cuda(), "image1": torch.stack([p[1] for p in ps])[:, None].cuda()}
    return _cache[key]


def _matcher(**kw):
    from gisnav_amd.loftr import LoFTR
    return LoFTR(state_dict=_sd(), **kw).to("cuda:0").eval()


def _segments(m, batch):
    """Per pair, the five outputs cut to the pair's count, on the host."""
    seg = m.match_segments(batch["image0"], batch["image1"])
    out = []
    for b, n in enumerate(seg["n_host"]):
        ij = seg["ij"][b, :n].cpu()
        out.append({"keypoints0": seg["keypoints0"][b, :n].cpu(), "keypoints1": seg["keypoints1"][b, :n].cpu(), "confidence": seg["confidence"][b, :n].cpu(),
                    "i_ids": ij[:, 0].clone(), "j_ids": ij[:, 1].clone()})
    return out, seg.get("uncertain")


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


def _reference(arithmetic, seeds, h, w, fine=True, **kw):
    """The outputs of an uncertified context of `arithmetic`, per pair; computed once per batch."""
    key = ("ref", arithmetic, tuple(seeds), h, w, fine, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = _segments(_matcher(arithmetic=arithmetic, fine=fine), _batch(seeds, h, w, **kw))[0]
    return _cache[key]


def _mode1(h, w, seeds):
    """One mode-1 call on a split-fp16 context: the GPU's vectors, fp64 conf statistics from its own "sim", and each pair's critical eps."""
    key = ("mode1", h, w, tuple(seeds))
    if key in _cache:
        return _cache[key]
    B, hc, wc = len(seeds), h // 8, w // 8
    L = hc * wc
    Lp = (L + 127) // 128 * 128
    m = _matcher(arithmetic="split_fp16", certify="flags", certify_eps=1e-3)
    _, unc = _segments(m, _batch(seeds, h, w))
    assert unc is not None and unc.shape == (B,) and unc.dtype == torch.bool
    sim = m.debug_read("sim", B * Lp * Lp).reshape(B, Lp, Lp)[:, :L, :L].astype(np.float64) / TEMPERATURE
    vec = {n: m.debug_read(n, B * Lp).reshape(B, Lp)[:, :L].astype(np.float64) for n in ("crow", "ccol", "crow2", "ccol2")}
    pairs = []
    for b in range(B):
        s = sim[b]
        e0 = np.exp(s - s.max(0, keepdims=True)); e1 = np.exp(s - s.max(1, keepdims=True))
        conf = (e0 / e0.sum(0, keepdims=True)) * (e1 / e1.sum(1, keepdims=True))
        rb, rs = _top2(conf, 1)
        cb, cs = _top2(conf, 0)
        stats = (_interior(hc, wc), rb, rs, cb, cs)
        pairs.append({"stats": stats, "eps_star": _critical_eps(stats), "conf": conf})
    _cache[key] = {"matcher": m, "vec": vec, "pairs": pairs}
    return _cache[key]


def _eps_star(h, w, seed):
    for seeds in SHAPES[(h, w)]:
        if seed in seeds:
            return _mode1(h, w, seeds)["pairs"][seeds.index(seed)]["eps_star"]
    raise KeyError(seed)


CALLS = [(h, w, tuple(seeds)) for (h, w), batches in SHAPES.items() for seeds in batches]


@pytest.mark.parametrize("h,w,seeds", CALLS)
def test_runner_ups_against_fp64(h, w, seeds):
    """crow2 / ccol2 against the fp64 second-largest (multiplicity counted) of conf recomputed from the GPU's "sim".  The bar is e1 = the largest
    relative error of the EXISTING maxima crow / ccol against the same fp64 matrix (code this feature does not touch): 2 e1 + 1e-7."""
    r = _mode1(h, w, list(seeds))
    rel = lambda got, ref: float(np.max(np.abs(got - ref) / ref))  # noqa: E731
    e1 = e2 = 0.0
    for b, p in enumerate(r["pairs"]):
        _, rb, rs, cb, cs = p["stats"]
        e1 = max(e1, rel(r["vec"]["crow"][b], rb), rel(r["vec"]["ccol"][b], cb))
        e2 = max(e2, rel(r["vec"]["crow2"][b], rs), rel(r["vec"]["ccol2"][b], cs))
        assert (r["vec"]["crow2"][b] <= r["vec"]["crow"][b]).all() and (r["vec"]["ccol2"][b] <= r["vec"]["ccol"][b]).all()
    print(f"{h}x{w} seeds {seeds}: e1 {e1:.3e} runner-ups {e2:.3e}")
    _report(f"runner_ups_{h}x{w}_{'_'.join(map(str, seeds))}", {"e1": e1, "e2": e2})
    assert e2 <= 2 * e1 + 1e-7


@pytest.mark.parametrize("h,w,seeds", CALLS)
def test_flags_follow_the_rule(h, w, seeds):
    """Each pair's critical eps* from the fp64 conf of its own "sim": eps*/1.25 leaves it unflagged, 1.25 eps* flags it (one call per eps on
    the context of the mode-1 run: eps is a device word, so these are replays of one graph)."""
    r = _mode1(h, w, list(seeds))
    m, batch = r["matcher"], _batch(list(seeds), h, w)
    stars = [p["eps_star"] for p in r["pairs"]]
    print(f"{h}x{w} seeds {seeds}: eps* {[f'{e:.3e}' for e in stars]}")
    _report(f"eps_star_{h}x{w}_{'_'.join(map(str, seeds))}", stars)
    assert min(stars) > 1e-3
    for b, es in enumerate(stars):
        for eps, want in ((es / 1.25, False), (es * 1.25, True)):
            m.set_certify_eps(eps)
            unc = m.match_segments(batch["image0"], batch["image1"])["uncertain"]
            expect = [bool(eps >= 1.25 * e) for e in stars]
            decided = [eps >= 1.25 * e or eps <= e / 1.25 for e in stars]
            assert bool(unc[b]) == want, (b, eps, es)
            assert all(bool(unc[k]) == expect[k] for k in range(len(stars)) if decided[k]), (eps, stars, unc)
    m.set_certify_eps(1e-3)


RERUN = [((64, 96), [1, 2], 3.5e-2, [2]), ((136, 200), [4, 2, 6], 4e-2, [2]), ((256, 336), [1, 2], 4.2e-2, [1])]


@pytest.mark.parametrize("shape,seeds,eps,flagged_seeds", RERUN, ids=["64x96", "136x200", "256x336"])
def test_rerun_replaces_exactly_the_flagged_pairs(shape, seeds, eps, flagged_seeds):
    h, w = shape
    stars = [_eps_star(h, w, s) for s in seeds]
    # the chosen eps is at least a factor 1.25 away from every pair's eps* (the GPU's own, from test 2's fp64 matrices)
    assert all(eps >= 1.25 * e or eps <= e / 1.25 for e in stars), (eps, stars)
    want = [s in flagged_seeds for s in seeds]
    assert want == [eps >= e for e in stars], (eps, stars)
    batch = _batch(seeds, h, w)
    differs = False
    for fine in (True, False):
        f32, split = _reference("exact_f32", seeds, h, w, fine), _reference("split_fp16", seeds, h, w, fine)
        results = {}
        for graph in (True, False):
            m = _matcher(arithmetic="split_fp16", certify="rerun", certify_eps=eps, fine=fine, graph=graph)
            out, unc = _segments(m, batch)
            assert [bool(u) for u in unc] == want
            assert m.certify_stats() == {"pairs": len(seeds), "flagged": sum(want), "rerun_certificate": sum(want), "rerun_guard": 0}
            for b, flag in enumerate(want):
                assert _same(out[b], f32[b] if flag else split[b]), (fine, graph, b, flag)
                differs = differs or (flag and not _same(out[b], split[b]))
            results[graph] = out
            if graph:
                # eps is read from device memory: changing it between two calls of one context (one captured graph) takes effect
                m.set_certify_eps(min(stars) / 2)
                out0, unc0 = _segments(m, batch)
                assert not unc0.any() and all(_same(out0[b], split[b]) for b in range(len(seeds)))
                m.set_certify_eps(max(stars) * 2)
                out1, unc1 = _segments(m, batch)
                assert unc1.all() and all(_same(out1[b], f32[b]) for b in range(len(seeds)))
                assert m.certify_stats() == {"pairs": 3 * len(seeds), "flagged": sum(want) + len(seeds), "rerun_certificate": sum(want) + len(seeds), "rerun_guard": 0}
        assert all(_same(results[True][b], results[False][b]) for b in range(len(seeds)))
    assert differs, "no flagged pair differs from its split result in any bit: the test cannot tell a re-run from none"


def _fp64_conf_from(m, batch, B, L, Lp):
    m.match_segments(batch["image0"], batch["image1"])
    sim = m.debug_read("sim", B * Lp * Lp).reshape(B, Lp, Lp)[:, :L, :L].astype(np.float64) / TEMPERATURE
    e0 = np.exp(sim - sim.max(1, keepdims=True)); e1 = np.exp(sim - sim.max(2, keepdims=True))
    return (e0 / e0.sum(1, keepdims=True)) * (e1 / e1.sum(2, keepdims=True))


def test_calibration():
    from gisnav_amd import _lib
    h, w, seeds = 136, 200, [1, 2, 3]
    L, Lp = 425, 512
    batch = _batch(seeds, h, w)
    m = _matcher(arithmetic="split_fp16", certify="rerun")
    with pytest.raises(_lib.GnError, match="eps"):                     # a shape without an eps raises under certify
        m(batch)
    cal = m.calibrate_certify(batch["image0"], batch["image1"])
    assert cal["eps"] == max(np.float32(1e-5), np.float32(4.0) * np.float32(cal["d_max"]))
    ref = float(np.abs(_fp64_conf_from(_matcher(arithmetic="split_fp16"), batch, 3, L, Lp) - _fp64_conf_from(_matcher(arithmetic="exact_f32"), batch, 3, L, Lp)).max())
    print(f"d_max {cal['d_max']:.3e} (fp64 from the two sims: {ref:.3e}) eps {cal['eps']:.3e}")
    _report("calibration_136x200", {"d_max": cal["d_max"], "d_max_fp64": ref, "eps": cal["eps"]})
    assert 0.5 * ref <= cal["d_max"] <= 2 * ref
    out = m(batch)
    assert out["keypoints0"].shape[0] > 100
    # a calibration belongs to its weights: loading a tensor discards it, and the certified call fails until the sample is measured again
    name = "loftr_coarse.layers.0.norm1.bias"
    arr = np.ascontiguousarray(_sd()[name].numpy(), dtype=np.float32)
    assert m.lib.gn_loftr_load_tensor(m._ctx, name.encode(), arr.ctypes.data_as(C.c_void_p), (C.c_int64 * 1)(arr.shape[0]), 1) == 0
    with pytest.raises(_lib.GnError, match="calibrate"):
        m(batch)
    again = m.calibrate_certify(batch["image0"], batch["image1"])
    assert again == cal                                                 # (the same weights, the same sample: the same bits)
    assert torch.equal(m(batch)["keypoints1"], out["keypoints1"])
    # a sample that leaves fp16's range trips the guard: there is no split-arithmetic result to bound
    hot = _batch(seeds, h, w, scale=[1.0, 3.0e5, 1.0])
    with pytest.raises(_lib.GnError, match="guard"):
        m.calibrate_certify(hot["image0"], hot["image1"])


def test_sound_at_the_calibrated_eps():
    """128x160, noise 0.1, seeds 1-6 as one call: at the calibrated eps every unflagged pair has exact f32's (i, j) list (mode 1) and with the
    re-run all six have (mode 2).  At most 2 of the 6 may be flagged, else the statement would be empty."""
    h, w, seeds = 128, 160, [1, 2, 3, 4, 5, 6]
    batch = _batch(seeds, h, w, noise=0.1)
    f32 = _reference("exact_f32", seeds, h, w, noise=0.1)
    ids = lambda o: (o["i_ids"], o["j_ids"])  # noqa: E731
    eq = lambda a, b: torch.equal(a["i_ids"], b["i_ids"]) and torch.equal(a["j_ids"], b["j_ids"])  # noqa: E731
    m1 = _matcher(arithmetic="split_fp16", certify="flags")
    cal = m1.calibrate_certify(batch["image0"], batch["image1"])
    out1, unc1 = _segments(m1, batch)
    print(f"calibrated eps {cal['eps']:.3e} (d_max {cal['d_max']:.3e}); flagged {[bool(u) for u in unc1]}; matches {[len(o['i_ids']) for o in f32]}")
    _report("soundness_128x160_noise0.1", {"eps": cal["eps"], "d_max": cal["d_max"], "flagged": int(unc1.sum())})
    assert min(len(ids(o)[0]) for o in f32) > 0
    assert int(unc1.sum()) <= 2
    for b in range(6):
        if not unc1[b]:
            assert eq(out1[b], f32[b]), b
    m2 = _matcher(arithmetic="split_fp16", certify="rerun")
    m2.calibrate_certify(batch["image0"], batch["image1"])
    out2, unc2 = _segments(m2, batch)
    assert torch.equal(unc1, unc2)
    assert all(eq(out2[b], f32[b]) for b in range(6))


def test_guard_and_certificate_together():
    """[seed 1 x 3e5, seed 5] at 128x160, eps 4.5e-2: the first pair leaves fp16's range and comes back f32-identical through the guard, seed 5
    (eps* 8.7e-2 on the oracle) passes the certificate and stays split; the re-run is the guard's in the counters."""
    h, w, seeds, scale = 128, 160, [1, 5], [3.0e5, 1.0]
    batch = _batch(seeds, h, w, scale=scale)
    f32, split = _reference("exact_f32", seeds, h, w, scale=tuple(scale)), _reference("split_fp16", seeds, h, w, scale=tuple(scale))
    m = _matcher(arithmetic="split_fp16", certify="rerun", certify_eps=4.5e-2)
    out, unc = _segments(m, batch)
    assert _same(out[0], f32[0]) and len(out[0]["i_ids"]) > 0
    assert _same(out[1], split[1]) and len(out[1]["i_ids"]) > 0
    assert [bool(u) for u in unc] == [False, False]
    assert m.certify_stats() == {"pairs": 2, "flagged": 0, "rerun_certificate": 0, "rerun_guard": 1}
    assert int(m.debug_read("ovf_trips", 1)[0]) == 1

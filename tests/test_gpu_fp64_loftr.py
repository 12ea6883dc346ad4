"""GPU tests (-m gpu) of LoFTR stage by stage against a float64 reference (oracle/loftr.py's stage entry points on float64 weights).

tests/test_loftr.py holds the GPU to the f32 oracle at 2e-5 .. 2e-4 of max |ref| -- 30 to 400 times the f32 oracle's own distance from fp64
(3.5e-7 .. 1.7e-6 on the features, tests/test_oracle_fp64.py), and the errors of ~20 convolutions and 8 encoder layers compound before the
last taps are compared.  Here every stage's fp64 reference starts from the GPU's OWN input to that stage, so each stage's error is its own:

  stem + layer1 (images -> x1) | layer2 + layer3 (GPU x1 -> x3) | layer3_outconv (GPU x3 -> x3_out) | FPN head (GPU x1, GPU x3_out -> the
  224-row x2 tap, whose padding channels 196..223 must be exactly 0, and x1_out; the GPU keeps no layer2 output, so layer2 is recomputed in
  fp64 from GPU x1) | coarse transformer (GPU x3_out + pe -> tok, valid rows) | coarse matching (GPU tok -> sim, row / column maxima of conf,
  confidence, ids) | fine level (GPU x1_out, tok, ids -> ftok windows of the M matches, keypoints1).

Measure: max |g - r| / max |r| over valid elements (keypoints1: absolute px).  ONE budget per stage for both arithmetics -- the split-fp16
one is documented as f32-accurate -- at about 4 x the largest exact_f32 value measured on an MI355X over every case here.  Coarse ids must
equal fp64's on every cell whose fp64 decision margin (conf against the 0.2 threshold, row and column maximum against the runner-up) is more
than 4 x the stage's measured conf error; the excluded cells are counted in the report.

Cases: 32x32 (L = 16 below k_lf_col_stats' 32 splits; no match, so the fine level runs with M = 0), 64x64 / 64x72 (L = 64 / 72 either side
of k_lf_kv_partial's 64-token chunk rule), 96x128 (L = 192: one chunk), 136x200 (L = 425, Lp = 512: ragged last chunk, 1/2-resolution width
100), 512x64 and 64x1024 (mostly empty 32-column conv tiles, 8-column coarse rows), each on the synthetic pair, the pair times 2^-6 and
2^-10 (dark: most activations then sit where the split's low fp16 term is subnormal), the pair times 2^7 (bright, below the split path's
overflow guard) and on a second weight set whose transformer updates are not small next to the residual; 480x640 (configs[1]) once per
arithmetic.  Measured numbers go to test_reports/fp64_loftr.json (git-ignored), stamped with the loaded library's digest.

Measured on an MI355X, largest over the cases (exact_f32 / split_fp16): see DESIGN.md 9 and STAGE_BUDGET below.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import loftr as lf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(32, 32), (64, 64), (64, 72), (96, 128), (136, 200), (512, 64), (64, 1024)]
INPUTS = {"synthetic": (0, 1.0), "dark6": (0, 2.0 ** -6), "dark10": (0, 2.0 ** -10), "bright7": (0, 2.0 ** 7), "weights1": (1, 1.0)}
CASES = [(h, w, inp, ar) for (h, w) in SMALL for inp in INPUTS for ar in ("exact_f32", "split_fp16")]
CASES += [(480, 640, "synthetic", ar) for ar in ("exact_f32", "split_fp16")]
# per-stage budgets (relative to max |fp64|; keypoints1 in px), both arithmetics: about 4 x the largest exact_f32 value measured on an MI355X
# over CASES (exact_f32 / split_fp16 maxima: x1 1.1e-6 / 9.0e-7, x3 1.6e-6 / 1.5e-6, x3_out 1.2e-6 / 8.9e-7, x2 3.9e-6 / 3.8e-6, x1_out
# 6.6e-6 / 5.7e-6, tok 4.8e-7 / 4.9e-7, sim 9.6e-7 / 5.7e-7, crow / ccol 3.2e-5 / 3.8e-5, confidence 4.6e-6 / 2.3e-6, ftok 1.0e-6 / 7.6e-7,
# keypoints1 4.8e-5 / 3.4e-5 px; no coarse cell excluded, no id differs).  x2 and x1_out include layer2's f32 error (recomputed in fp64 from
# GPU x1); crow / ccol are the dual softmax's maxima, whose exponent is sim / 0.1.
STAGE_BUDGET = {"x1": 4.5e-6, "x3": 6.5e-6, "x3_out": 5e-6, "x2": 1.6e-5, "x1_out": 2.6e-5, "tok": 2e-6, "sim": 4e-6, "crow": 1.3e-4, "ccol": 1.3e-4,
                "confidence": 2e-5, "ftok": 4e-6, "keypoints1_px": 2e-4}
TEMPERATURE, THR, BORDER = 0.1, 0.2, 2
_SD = {}
_REF1 = {}


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "fp64_loftr.json")
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


def _threads():
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))


def _weights(seed):
    """(float32 state dict for the GPU, float64 copy for the reference), per module"""
    if seed not in _SD:
        sd = lf.synthetic_state_dict(0) if seed == 0 else lf.synthetic_state_dict(1, mlp_out_gain=1.0)
        _SD[seed] = (sd, lf.cast_state_dict(sd, torch.float64))
    return _SD[seed]


def _images(h, w, inp):
    seed = 2 if (h, w) != (480, 640) else 1
    i0, i1 = lf.synthetic_pair(seed, h, w)
    scale = INPUTS[inp][1]
    return (i0 * scale).contiguous(), (i1 * scale).contiguous()


def _nchw64(a, n, h, w, c, creal=None):
    """GPU NHWC f32 rows -> (n, creal, h, w) float64"""
    t = torch.from_numpy(np.ascontiguousarray(a.reshape(n, h, w, c)[..., : (creal or c)])).permute(0, 3, 1, 2).double()
    return t.contiguous()


def _rel(g, r):
    g = np.asarray(g, np.float64)
    r = np.asarray(r, np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if r.size == 0:
        return 0.0
    assert np.isfinite(g).all()
    return float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300))


def _ref_layer1(h, w, inp):
    """fp64 stem + layer1 from the images: shared by both arithmetics (cached per module)"""
    key = (h, w, inp)
    if key not in _REF1:
        _, sd64 = _weights(INPUTS[inp][0])
        i0, i1 = _images(h, w, inp)
        with torch.inference_mode():
            _, x1 = lf.backbone_layer1(sd64, torch.stack([i0, i1]).double()[:, None])
        _REF1[key] = x1.permute(0, 2, 3, 1).numpy().copy()
    return _REF1[key]


def _gpu_run(model, i0, i1, h, w):
    out = model({"image0": i0[None, None].cuda(), "image1": i1[None, None].cuda()}, with_ids=True)
    out = {k: v.cpu() for k, v in out.items()}
    h2, w2, h4, w4, hc, wc = h // 2, w // 2, h // 4, w // 4, h // 8, w // 8
    L = hc * wc
    Lp = (L + 127) // 128 * 128
    rd = model.debug_read
    taps = {"x1": rd("x1", 2 * h2 * w2 * 128), "x3": rd("x3", 2 * L * 256), "x3_out": rd("x3_out", 2 * L * 256), "x2": rd("x2", 2 * h4 * w4 * 224),
            "x1_out": rd("x1_out", 2 * h2 * w2 * 128), "tok": rd("tok", 2 * Lp * 256).reshape(2, Lp, 256), "sim": rd("sim", Lp * Lp).reshape(Lp, Lp),
            "crow": rd("crow", Lp), "ccol": rd("ccol", Lp), "ftok": rd("ftok", 2 * Lp * 25 * 128).reshape(2, Lp, 25, 128)}
    return out, taps


def _margins(conf, hc, wc):
    """fp64 decision margin of every cell i of image0: how far conf would have to move to change whether / where i matches"""
    L = conf.shape[0]
    yi, xi = np.arange(L) // wc, np.arange(L) % wc
    inside = (yi >= BORDER) & (yi < hc - BORDER) & (xi >= BORDER) & (xi < wc - BORDER)
    marg = np.full(L, np.inf)
    if L < 2:
        return marg
    jstar = conf.argmax(1)
    best = conf[np.arange(L), jstar]
    row2 = np.partition(conf, L - 2, axis=1)[:, L - 2]
    for i in np.nonzero(inside)[0]:
        if best[i] <= THR:
            marg[i] = THR - best[i]                                  # no entry of the row clears the threshold
            continue
        col = conf[:, jstar[i]].copy()
        col[i] = -np.inf
        marg[i] = min(best[i] - THR, best[i] - row2[i], abs(best[i] - col.max()))
    return marg


@pytest.mark.parametrize("h,w,inp,arith", CASES)
def test_loftr_stages_against_fp64_from_their_own_gpu_input(h, w, inp, arith):
    from gisnav_amd.loftr import LoFTR
    _threads()
    sd, sd64 = _weights(INPUTS[inp][0])
    i0, i1 = _images(h, w, inp)
    h2, w2, h4, w4, hc, wc = h // 2, w // 2, h // 4, w // 4, h // 8, w // 8
    L = hc * wc
    m = LoFTR(state_dict=sd, arithmetic=arith).to("cuda:0").eval()
    out, g = _gpu_run(m, i0, i1, h, w)
    if arith == "split_fp16" and inp == "bright7":
        # the guard must not have tripped (a tripped call is repeated on the exact kernels: x1 would then be the exact build's, bit for bit)
        ex = LoFTR(state_dict=sd, arithmetic="exact_f32").to("cuda:0").eval()
        _, ge = _gpu_run(ex, i0, i1, h, w)
        assert not np.array_equal(ge["x1"], g["x1"])
        del ex
    del m
    err, info = {}, {}
    with torch.inference_mode():
        # stem + layer1 from the images
        err["x1"] = _rel(g["x1"].reshape(2, h2, w2, 128), _ref_layer1(h, w, inp))
        # layer2 + layer3 from GPU x1
        gx1 = _nchw64(g["x1"], 2, h2, w2, 128)
        x2_64, x3_64 = lf.backbone_layer23(sd64, gx1)
        err["x3"] = _rel(g["x3"].reshape(2, hc, wc, 256), x3_64.permute(0, 2, 3, 1).numpy())
        # layer3_outconv from GPU x3
        x3o_64 = lf.layer3_outconv(sd64, _nchw64(g["x3"], 2, hc, wc, 256))
        err["x3_out"] = _rel(g["x3_out"].reshape(2, hc, wc, 256), x3o_64.permute(0, 2, 3, 1).numpy())
        # FPN head from GPU x1 (layer2 recomputed from it) and GPU x3_out
        gx3o = _nchw64(g["x3_out"], 2, hc, wc, 256)
        x2o_64, x1o_64 = lf.fpn_head(sd64, gx1, x2_64, gx3o)
        gx2 = g["x2"].reshape(2, h4, w4, 224)
        assert not np.any(gx2[..., 196:]), "padding channels of the FPN's 1/4 map are not zero"
        err["x2"] = _rel(gx2[..., :196], x2o_64.permute(0, 2, 3, 1).numpy())
        err["x1_out"] = _rel(g["x1_out"].reshape(2, h2, w2, 128), x1o_64.permute(0, 2, 3, 1).numpy())
        # coarse transformer from GPU x3_out (valid rows: padded rows L..Lp-1 carry LayerNorm biases by design)
        f0, f1 = lf.coarse_transformer(sd64, gx3o)
        err["tok"] = _rel(g["tok"][:, :L], torch.cat([f0, f1]).numpy())
        # coarse matching from GPU tok
        t0 = torch.from_numpy(g["tok"][0, :L].copy()).double()[None]
        t1 = torch.from_numpy(g["tok"][1, :L].copy()).double()[None]
        ct = {}
        b_ids, i_ids, j_ids, mconf, mk0, mk1 = lf.coarse_matching(t0, t1, (hc, wc), (hc, wc), 8, taps=ct)
        sim64, conf64 = ct["sim_matrix"][0].numpy(), ct["conf_matrix"][0].numpy()
        err["sim"] = _rel(g["sim"][:L, :L], sim64 * TEMPERATURE)         # the GPU's matrix is <f0, f1> / C before the temperature
        err["crow"] = _rel(g["crow"][:L], conf64.max(1))
        err["ccol"] = _rel(g["ccol"][:L], conf64.max(0))
        gi, gj = out["i_ids"].numpy(), out["j_ids"].numpy()
        M = len(gi)
        err["confidence"] = _rel(out["confidence"].numpy(), conf64[gi, gj]) if M else 0.0
        e_conf = max(err["crow"], err["ccol"], err["confidence"]) * max(float(conf64.max()), 1e-300)
        marg = _margins(conf64, hc, wc)
        keep = marg > 4.0 * e_conf
        want = {int(i): int(j) for i, j in zip(i_ids, j_ids)}
        got = {int(i): int(j) for i, j in zip(gi, gj)}
        bad = [i for i in np.nonzero(keep)[0] if want.get(int(i)) != got.get(int(i))]
        info.update(L=L, M=M, M_fp64=len(want), excluded_cells=int((~keep).sum()), id_mismatch=len(bad))
        assert not bad, ("coarse ids differ from fp64 on decided cells", bad[:10])
        assert torch.equal(out["keypoints0"], torch.stack([torch.from_numpy(gi % wc), torch.from_numpy(gi // wc)], 1).float() * 8)
        # fine level from GPU x1_out, tok and ids
        if (h, w) == (32, 32):
            assert M == 0 and len(want) == 0
        gb = torch.zeros(M, dtype=torch.long)
        ti, tj = torch.from_numpy(gi), torch.from_numpy(gj)
        k0c = torch.stack([ti % wc, ti // wc], 1).double() * 8
        k1c = torch.stack([tj % wc, tj // wc], 1).double() * 8
        ft = {}
        _, k1f = lf.fine_level(sd64, _nchw64(g["x1_out"], 2, h2, w2, 128), t0, t1, gb, ti, tj, k0c, k1c, taps=ft)
        ff0, ff1 = ft["fine_windows"]
        err["ftok"] = _rel(np.concatenate([g["ftok"][0, :M], g["ftok"][1, :M]]), torch.cat([ff0, ff1]).numpy()) if M else 0.0
        err["keypoints1_px"] = float((out["keypoints1"].double() - k1f).abs().max()) if M else 0.0
    _report(f"{arith}_{h}x{w}_{inp}", {**err, **info})
    over = {k: (v, STAGE_BUDGET[k]) for k, v in err.items() if not v <= STAGE_BUDGET[k]}
    assert not over, over


@pytest.mark.parametrize("arith", ["exact_f32", "split_fp16"])
def test_loftr_conv_tilings_are_bitwise_equal(arith):
    """lf_conv picks rows per wave (RPW) from a cost model whose per-workgroup overhead developer knob 42 (bits 8 and up, 1/100 units) sets.
    Every output's sum does not depend on RPW: each lane accumulates its own pixel in one accumulator over channel slices -> taps -> channel
    steps in the same order whatever the tile height, from the same halo values, through the same epilogue (k_lf_conv, k_lf_conv_h).  So a large
    overhead (RPW 4 at stride 1, 2 at stride 2) and a small one (RPW 1 on small grids) give the default's bits, every tap and output."""
    from gisnav_amd.loftr import LoFTR
    sd, _ = _weights(0)
    h, w = 136, 200
    i0, i1 = _images(h, w, "synthetic")
    res = {}
    for knob in (0, 100000 << 8, 1 << 8):
        m = LoFTR(state_dict=sd, arithmetic=arith).to("cuda:0").eval()        # (a new matcher per knob; the knob is its own, nothing to restore)
        m.debug_variant(42, knob)
        res[knob] = _gpu_run(m, i0, i1, h, w)
        del m
    base_out, base_taps = res[0]
    assert base_out["keypoints0"].shape[0] > 100
    for knob in (100000 << 8, 1 << 8):
        o, t = res[knob]
        for k in base_out:
            assert torch.equal(base_out[k], o[k]), (knob, k)
        for k in base_taps:
            assert np.array_equal(base_taps[k].view(np.uint32), t[k].view(np.uint32)), (knob, k)

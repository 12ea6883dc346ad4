"""LightGlue(features="superpoint") -- the matcher of BASELINE.json configs[4] (256-d descriptors, 2-D positional encoding, no
input projection).  The golden fixtures tests/golden/lightglue_sp_*.npz come from THIRD-PARTY code
(transformers' LightGlueForKeypointMatching on CPU, tests/golden/make_superpoint_golden.py), not from the repo's oracle: the CPU
test pins the oracle to them, the GPU tests pin the HIP path to them and to the oracle.

Tolerances: correspondence indices identical; scores |d| <= 1e-5 (f32 mode) / 5e-3 (bf16-attention modes); final descriptors
rel 2e-5 (f32 mode)."""
import os

import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import K_MATRIX, make_pair_256
from gisnav_amd.weights import synthetic_state_dict
from oracle import lightglue_superpoint as lsp

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["lightglue_sp_seed0_n200_640x480", "lightglue_sp_seed0_n384_1920x1080"]


@pytest.fixture(scope="module")
def sd_sp():
    return synthetic_state_dict(0, feature="superpoint")


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_transformers_generated_fixture(name, sd_sp):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    tsd = {k: torch.from_numpy(v) for k, v in sd_sp.items()}
    taps = {}
    sc, idx = lsp.match(tsd, torch.from_numpy(g["kp_q"]), torch.from_numpy(g["desc_q"]), torch.from_numpy(g["kp_r"]), torch.from_numpy(g["desc_r"]),
                        hw0=(int(g["h"]), int(g["w"])), hw1=(int(g["h"]), int(g["w"])), taps=taps)
    assert np.array_equal(idx.numpy(), g["idx"])
    assert np.abs(sc.numpy()[:, 0] - g["scores"]).max() < 2e-5
    x = torch.cat([taps["layer8_0"], taps["layer8_1"]], 0).numpy()
    assert np.abs(x - g["x_final"]).max() < 2e-5 * np.abs(g["x_final"]).max()


def test_weight_layout_of_the_superpoint_variant(sd_sp):
    from gisnav_amd.weights import expected_shapes
    shp = expected_shapes(feature="superpoint")
    assert "input_proj.weight" not in sd_sp and sd_sp["posenc.Wr.weight"].shape == (32, 2) == shp["posenc.Wr.weight"]
    for k, v in shp.items():
        assert sd_sp[k].shape == v, k


# ------------------------------------------------------------------ HIP path (GPU)
@pytest.fixture(scope="module")
def engines(sd_sp):
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from gisnav_amd.engine import PoseEngine
    return {prec: PoseEngine(0, max_batch=4, max_kpts=384, precision=prec, state_dict=sd_sp, filter_threshold=0.1, feature="superpoint")
            for prec in ("f32", "f16x2_bf16_attn")}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x2_bf16_attn"])
@pytest.mark.parametrize("name", FIXTURES)
def test_superpoint_matcher_against_transformers_fixture(engines, name, prec):
    eng = engines[prec]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    dev = eng.device
    n = len(g["kp_q"])
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kq = np.zeros((1, n, 4), np.float32); kq[0, :, :2] = g["kp_q"]
    kr = np.zeros((1, n, 4), np.float32); kr[0, :, :2] = g["kp_r"]
    nn = torch.tensor([n], dtype=torch.int32, device=dev)
    eng.set_image_size((float(g["w"]), float(g["h"])), (float(g["w"]), float(g["h"])))
    idx, score, n_match = eng.match(f(g["desc_q"][None]), f(kq), nn, f(g["desc_r"][None]), f(kr), nn)
    torch.cuda.synchronize()
    k = int(n_match[0])
    assert k == len(g["idx"]) and np.array_equal(idx[0, :k].cpu().numpy(), g["idx"])
    assert np.abs(score[0, :k].cpu().numpy() - g["scores"]).max() < (1e-5 if prec == "f32" else 5e-3)
    if prec == "f32":
        x = eng.debug_read("x", 4 * 2 * 384 * 256).reshape(4, 2, 384, 256)
        assert np.abs(x[0, :, :n] - g["x_final"]).max() < 2e-5 * np.abs(g["x_final"]).max()
    eng.set_image_size(None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x2_bf16_attn"])
def test_superpoint_ragged_batch_extent_sizes_and_pose(engines, sd_sp, prec):
    """Ragged batch, image size = keypoint extent (hw None, kornia's fallback) and the pose stage behind the 256-d matcher."""
    eng = engines[prec]
    tsd = {k: torch.from_numpy(v) for k, v in sd_sp.items()}
    pairs = [make_pair_256(60 + i, n_q=384 - 23 * i, n_r=370 - 11 * i, h=480, w=640) for i in range(3)]
    inp = eng.stage_inputs(pairs)
    idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    out = eng.estimate(inp, K_MATRIX)
    torch.cuda.synchronize()
    for b, p in enumerate(pairs):
        sc, oidx = lsp.match(tsd, torch.from_numpy(p.kp_q), torch.from_numpy(p.desc_q), torch.from_numpy(p.kp_r), torch.from_numpy(p.desc_r))
        k = int(n_match[b])
        assert k == len(oidx) > 100 and np.array_equal(idx[b, :k].cpu().numpy(), oidx.numpy())
        assert int(out["ok"][b]) == 1 and np.linalg.norm(out["R"][b].cpu().numpy() - p.R_gt) < 2e-2


@pytest.mark.gpu
def test_superpoint_matcher_object_drop_in(sd_sp):
    """gisnav_amd.LightGlueMatcher("superpoint") with kornia's call signature, hw given."""
    from gisnav_amd.matcher import LightGlueMatcher
    from oracle import lightglue_sift as lg
    tsd = {k: torch.from_numpy(v) for k, v in sd_sp.items()}
    p = make_pair_256(70, n_q=300, n_r=280, h=1080, w=1920)
    m = LightGlueMatcher("superpoint", params={"filter_threshold": 0.1, "depth_confidence": -1, "width_confidence": -1}, state_dict=sd_sp, max_kpts=384).to("cuda:0").eval()
    tq = torch.from_numpy
    laf_q = lg.laf_from_center_scale_ori(tq(p.kp_q)[None], torch.ones(1, 300, 1, 1), torch.zeros(1, 300, 1))
    laf_r = lg.laf_from_center_scale_ori(tq(p.kp_r)[None], torch.ones(1, 280, 1, 1), torch.zeros(1, 280, 1))
    dists, idx = m(tq(p.desc_q).cuda(), tq(p.desc_r).cuda(), laf_q.cuda(), laf_r.cuda(), hw1=(1080, 1920), hw2=(1080, 1920))
    sc, oidx = lsp.match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.kp_r), tq(p.desc_r), hw0=(1080, 1920), hw1=(1080, 1920))
    assert idx.dtype == torch.int64 and dists.shape == (len(oidx), 1) and torch.equal(idx.cpu(), oidx)


# ------------------------------------------------------------------ SuperPoint extractor (conv backbone)
def _test_image(seed, h, w):
    rs = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 0.45 + 0.2 * np.sin(xx / 9.0 + 0.3 * seed) * np.cos(yy / 7.0)
    for _ in range(60):
        cx, cy, s_, a = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(2.0, 9.0), rs.uniform(-0.4, 0.4)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s_ * s_))
    img += 0.03 * rs.normal(size=(h, w))
    return np.clip(img, 0, 1).astype(np.float32)


def test_superpoint_oracle_equals_transformers_model():
    """oracle/superpoint.py against transformers' SuperPointForKeypointDetection with the same (seeded random) weights: keypoints,
    scores and descriptors identical -- the extractor's oracle IS pinned to third-party code."""
    from transformers.models.superpoint.configuration_superpoint import SuperPointConfig
    from transformers.models.superpoint.modeling_superpoint import SuperPointForKeypointDetection
    from oracle import superpoint as osp
    sd = osp.synthetic_state_dict(0)
    hf = SuperPointForKeypointDetection(SuperPointConfig(max_keypoints=300)).eval()
    hf.load_state_dict(sd, strict=True)
    img = torch.from_numpy(_test_image(1, 120, 160))
    kp, sc, d = osp.detect_and_describe(sd, img, 300)
    with torch.inference_mode():
        out = hf(img[None, None].repeat(1, 3, 1, 1))
    n = int(out.mask[0].sum())
    assert n == len(kp) == 300
    assert torch.equal(kp, torch.round(out.keypoints[0, :n] * torch.tensor([160.0, 120.0])))      # the model returns relative coordinates
    assert torch.equal(sc, out.scores[0, :n]) and float((d - out.descriptors[0, :n]).abs().max()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x2_bf16_attn"])
@pytest.mark.parametrize("seed,shape,k", [(2, (120, 160), 300), (3, (240, 320), 512), (4, (136, 200), 2048)])
def test_superpoint_extractor_against_oracle(seed, shape, k, prec):
    """HIP SuperPoint against the oracle: encoder features and score map to f32 rounding, the keypoint SET identical up to last-bit
    score ties (>= 99 %), descriptors of the common keypoints within 1e-4 -- with the exact-f32 MFMA convolutions of an f32 context
    and with the split-fp16 convolutions (each operand as two fp16 terms, three products, f32 accumulation) of an f16x2 context."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    sd = osp.synthetic_state_dict(0)
    eng = PoseEngine(0, max_batch=1, max_kpts=128, precision=prec, feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=k, state_dict=sd)
    img = _test_image(seed, *shape)
    taps = {}
    okp, osc, od = osp.detect_and_describe(sd, torch.from_numpy(img), k, taps=taps)
    kpt, score, desc, n = sp.detect_and_describe_device(img[None])
    torch.cuda.synchronize()
    h, w = shape[0] // 8, shape[1] // 8
    enc = sp._eng.debug_read("sp_enc", h * w * 128).reshape(h, w, 128)
    ref_enc = taps["block3"][0].permute(1, 2, 0).numpy()
    assert np.abs(enc - ref_enc).max() < 2e-5 * np.abs(ref_enc).max()
    smap = sp._eng.debug_read("sp_nms", shape[0] * shape[1]).reshape(shape)
    ref_map = taps["scores"][0].numpy()
    assert np.abs(smap - ref_map).max() < 1e-5
    assert ((smap > 0) != (ref_map > 0)).mean() < 1e-4          # NMS decisions: identical except where two scores tie to the last bit
    m = int(n[0])
    assert abs(m - len(okp)) <= max(2, len(okp) // 100)
    got = {(float(x), float(y)): i for i, (x, y) in enumerate(kpt[0, :m, :2].cpu().numpy())}
    ref = {(float(x), float(y)): i for i, (x, y) in enumerate(okp.numpy())}
    common = set(got) & set(ref)
    assert len(common) >= 0.99 * len(ref)
    gi = np.array([got[c] for c in common]); ri = np.array([ref[c] for c in common])
    assert np.abs(score[0].cpu().numpy()[gi] - osc.numpy()[ri]).max() < 1e-5
    assert np.abs(desc[0].cpu().numpy()[gi] - od.numpy()[ri]).max() < 1e-4
    sc = score[0, :m].cpu().numpy()
    assert (np.diff(sc) <= 0).all()                             # sorted by descending score
    assert np.abs(np.linalg.norm(desc[0, :m].cpu().numpy(), axis=1) - 1).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("seed,shape,k", [(2, (120, 160), 300), (3, (240, 320), 512)])
def test_superpoint_fp16_arithmetic_is_a_tolerance_mode(seed, shape, k):
    """gn_sp_set_arithmetic(GN_SP_FP16): ONE fp16 product per block (the 16-bit-operand arithmetic BASELINE configs[4] names) is not
    f32-accurate and is not asserted to be: encoder features within 2e-3 of the oracle's, >= 95 % of its keypoints, descriptors of the
    common keypoints within 2e-2 (cosine > 0.999); the measured figures go to the parity report.  The f32-accurate modes are the
    ones test_superpoint_extractor_against_oracle holds to 1e-5."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    sd = osp.synthetic_state_dict(0)
    with pytest.raises(RuntimeError):
        SuperPoint(engine=PoseEngine(0, max_batch=1, max_kpts=128, precision="f32", feature="superpoint"), arithmetic="fp16")
    eng = PoseEngine(0, max_batch=1, max_kpts=128, precision="f16x2_bf16_attn", feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=k, state_dict=sd, arithmetic="fp16")
    img = _test_image(seed, *shape)
    taps = {}
    okp, osc, od = osp.detect_and_describe(sd, torch.from_numpy(img), k, taps=taps)
    kpt, score, desc, n = sp.detect_and_describe_device(img[None])
    torch.cuda.synchronize()
    h, w = shape[0] // 8, shape[1] // 8
    enc = sp._eng.debug_read("sp_enc", h * w * 128).reshape(h, w, 128)
    ref_enc = taps["block3"][0].permute(1, 2, 0).numpy()
    enc_err = float(np.abs(enc - ref_enc).max() / np.abs(ref_enc).max())
    m = int(n[0])
    got = {(float(x), float(y)): i for i, (x, y) in enumerate(kpt[0, :m, :2].cpu().numpy())}
    ref = {(float(x), float(y)): i for i, (x, y) in enumerate(okp.numpy())}
    common = set(got) & set(ref)
    gi = np.array([got[c] for c in common]); ri = np.array([ref[c] for c in common])
    d_err = float(np.abs(desc[0].cpu().numpy()[gi] - od.numpy()[ri]).max())
    cos = float((desc[0].cpu().numpy()[gi] * od.numpy()[ri]).sum(1).min())
    print(f"fp16 SuperPoint {shape}: encoder rel err {enc_err:.2e}, keypoints in common {len(common)} / {len(ref)}, descriptor max err {d_err:.2e}, min cosine {cos:.6f}")
    assert enc_err < 2e-3 and len(common) >= 0.95 * len(ref) and d_err < 2e-2 and cos > 0.999


@pytest.mark.gpu
def test_superpoint_plus_lightglue_pixels_to_pose(sd_sp):
    """configs[4] end to end at reduced size: SuperPoint on a frame and on a shifted copy of it, LightGlue(superpoint) on the result
    (identity-block weights: mutual nearest neighbours of the descriptors), matches must be the shift."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    sd_m = synthetic_state_dict(0, feature="superpoint", identity_blocks=True)
    # random-weight descriptors are barely discriminative (any two have cosine ~0.99), so the soft assignment is flat: threshold 0 = pure mutual NN
    eng = PoseEngine(0, max_batch=1, max_kpts=512, precision="f32", state_dict=sd_m, filter_threshold=0.0, feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=512, state_dict=osp.synthetic_state_dict(0))
    big = _test_image(9, 256, 336)
    a, b = big[8:248, 8:328], big[16:256, 0:320]                # scene point (Y, X): a -> (Y - 8, X - 8), b -> (Y - 16, X); 8-aligned shift -> identical cell phase
    kpt, score, desc, n = sp.detect_and_describe_device(np.stack([a, b]))
    nd = torch.as_tensor(n, device=eng.device)
    eng.set_image_size((320.0, 240.0), (320.0, 240.0))
    idx, sc, nm = eng.match(desc[0:1], kpt[0:1], nd[0:1], desc[1:2], kpt[1:2], nd[1:2])
    torch.cuda.synchronize()
    k = int(nm[0])
    assert k > 50
    pa = kpt[0, idx[0, :k, 0], :2].cpu().numpy(); pb = kpt[1, idx[0, :k, 1], :2].cpu().numpy()
    d = pa - pb
    good = (np.abs(d[:, 0] + 8) < 0.5) & (np.abs(d[:, 1] - 8) < 0.5)            # (x, y) of a minus (x, y) of b
    assert good.mean() > 0.8, (k, good.mean())


@pytest.mark.gpu
def test_superpoint_split_convolutions_fall_back_when_activations_leave_fp16_range():
    """f16x2 contexts run the convolutions on split-fp16 operands; an activation >= 65504 raises the guard word and the pass is
    repeated with the exact-f32 instruction: the result must be what an f32 context computes, not inf / NaN."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).copy() for k, v in osp.synthetic_state_dict(0).items()}
    first = sorted(k for k in sd if k.endswith(".weight") and sd[k].ndim == 4 and sd[k].shape[1] == 1)[0]      # the 1 -> 64 layer
    sd[first] = sd[first] * 3.0e6                                                                                 # its ReLU outputs overflow fp16
    sd[first.replace(".weight", ".bias")] = sd[first.replace(".weight", ".bias")] * 3.0e6
    img = _test_image(5, 120, 160)
    res = {}
    for prec in ("f32", "f16x2_bf16_attn"):
        eng = PoseEngine(0, max_batch=1, max_kpts=128, precision=prec, feature="superpoint")
        sp = SuperPoint(engine=eng, max_keypoints=256, state_dict=sd)
        assert eng.sp_split_trips() == 0
        kpt, score, desc, n = sp.detect_and_describe_device(img[None])
        torch.cuda.synchronize()
        res[prec] = (kpt[0, :int(n[0])].cpu().numpy(), score[0, :int(n[0])].cpu().numpy(), desc[0, :int(n[0])].cpu().numpy(), int(n[0]))
        # the guard's counter (gn_debug_read("sp_split_trips")): exactly one trip per pass that tripped, none in an f32 context
        assert eng.sp_split_trips() == (0 if prec == "f32" else 1)
        again = sp.detect_and_describe_device(img[None])
        torch.cuda.synchronize()
        assert eng.sp_split_trips() == (0 if prec == "f32" else 2)
        assert torch.equal(again[0], kpt) and torch.equal(again[1], score) and torch.equal(again[2], desc) and int(again[3][0]) == int(n[0])
    a, b = res["f32"], res["f16x2_bf16_attn"]
    assert a[3] == b[3] > 0 and np.isfinite(b[2]).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])               # the SAME exact-f32 kernels ran


def test_oracle_reproduces_the_transformers_extractor_fixture_at_1080p():
    """configs[4]'s frame size: oracle/superpoint.py on the seeded 1920x1080 frame gives the keypoints / scores / descriptors that
    transformers' SuperPointForKeypointDetection produced (tests/golden/make_superpoint_extractor_golden.py)."""
    import hashlib
    import sys
    sys.path.insert(0, GOLD)
    from make_superpoint_extractor_golden import superpoint_test_image
    from oracle import superpoint as osp
    z = np.load(os.path.join(GOLD, "superpoint_extractor_seed7_1920x1080.npz"))
    u8 = superpoint_test_image(int(z["seed"]), int(z["h"]), int(z["w"]))
    assert hashlib.sha256(u8.tobytes()).hexdigest() == str(z["image_sha256"])
    kp, sc, d = osp.detect_and_describe(osp.synthetic_state_dict(0), torch.from_numpy(u8.astype(np.float32) * np.float32(1.0 / 255.0)), int(z["k"]))
    assert np.array_equal(kp.numpy().astype(np.int16), z["keypoints"])
    assert np.abs(sc.numpy() - z["scores"]).max() < 1e-6 and np.abs(d.numpy()[::4] - z["desc_every4"]).max() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1080, 1920), (1, 480, 1920), (3, 136, 200)])
def test_superpoint_split_kernels_against_the_f32_activation_path_and_simple_nms(shape):
    """The split-fp16 extractor's shipped kernels (knob 34 = 2: hm16 activation records staged by LDS-DMA, k_sp_conv_s16 for the 3 x 3 layers,
    k_sp_conv_s for the 1 x 1 layers) against k_sp_conv<., 1, ...> on f32 activations (knob 34 = 0, the path of frames beyond 8 Mpixel): the same
    terms and products, summed slice by slice instead of tap by tap -- score map within 1e-5 (f32 rounding), NMS support differing on < 1e-4 of the
    pixels, >= 99 % of the keypoints in common (last-bit ties).  sp_nms (k_sp_nms_fused) equals oracle simple_nms of the GPU's own score map
    bitwise at every pixel, on either path.  k_sp_select streaming its candidate list equals the register-cached form.  And the shipped form is
    repeatable run to run at the bench's frame size -- the first epilogue of these kernels was not (a packed `v_pk_fma_f32` with the scale in an
    SGPR pair returned garbage for one quad of lanes in about one tile per 10^4 with 16 waves per CU: DESIGN 12.4); the arithmetic is scalar now
    and this test repeats the pass."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    eng = PoseEngine(0, max_batch=1, max_kpts=128, precision="f16x2_f16_attn", feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=1024, state_dict=osp.synthetic_state_dict(0))
    img = torch.from_numpy(np.random.default_rng(11).random(shape, dtype=np.float32)).cuda()
    npx = shape[0] * shape[1] * shape[2]

    def run(conv):
        assert eng.lib.gn_debug_set_variant(eng.ctx, 34, conv) == 0
        out = sp.detect_and_describe_device(img)
        torch.cuda.synchronize()
        return (eng.debug_read("sp_scores", npx).copy(), eng.debug_read("sp_nms", npx).copy(), [o.cpu().numpy().copy() if hasattr(o, "cpu") else np.asarray(o) for o in out])

    try:
        f32a = run(0)
        s16 = run(2)
        assert np.abs(s16[0] - f32a[0]).max() < 1e-5
        assert ((s16[1] > 0) != (f32a[1] > 0)).mean() < 1e-4
        n_a, n_16 = f32a[2][3], s16[2][3]
        for b in range(shape[0]):
            ka = {(float(x), float(y)) for x, y in f32a[2][0][b, : int(n_a[b]), :2]}
            kb = {(float(x), float(y)) for x, y in s16[2][0][b, : int(n_16[b]), :2]}
            assert len(ka & kb) >= 0.99 * len(ka)
        for what, got in (("knob 34 = 0", f32a), ("knob 34 = 2", s16)):
            with torch.inference_mode():
                want = osp.simple_nms(torch.from_numpy(got[0].reshape(shape)), osp.NMS_RADIUS).numpy()
            assert np.array_equal(got[1].reshape(shape).view(np.uint32), want.view(np.uint32)), f"{what}: sp_nms differs from simple_nms(GPU scores)"
            assert int((got[1] > 0).sum()) > 100
        eng.lib.gn_debug_set_variant(eng.ctx, 40, 1)      # k_sp_select streaming its candidate list (frames with more than 40 960 candidates) = the register-cached form
        try:
            streamed = run(2)
        finally:
            eng.lib.gn_debug_set_variant(eng.ctx, 40, 0)
        assert all(np.array_equal(a, b) for a, b in zip(s16[2], streamed[2]))
        for _ in range(6 if shape[1] >= 480 else 2):
            again = run(2)
            assert np.array_equal(s16[0], again[0]) and np.array_equal(s16[1], again[1]), "knob 34 = 2: the pass is not repeatable"
            assert all(np.array_equal(a, b) for a, b in zip(s16[2], again[2]))
    finally:
        eng.lib.gn_debug_set_variant(eng.ctx, 34, 2)


# max |scores(k_sp_conv_h, the retired form) - scores(exact f32)| on the image of the test below, measured at the last commit that had the kernel
# (profiles/sp_retire.json "fp16_score_bar": 3.5627e-3; the shipped k_sp_conv_h16 measures 4.0251e-3), x 1.25
SCORE_BAR = 1.25 * 3.5626888275146484e-3


@pytest.mark.gpu
def test_superpoint_fp16_kernel_of_round5_against_the_one_it_replaces():
    """GN_SP_FP16 at the bench's frame size (2 x 1080 x 1920, seed 12): k_sp_conv_h16 + fp16 activations through every layer against the same context's
    exact-f32 arithmetic (sp_set_arithmetic) on the same image -- a tolerance mode (every layer rounds its activations to fp16).  Keypoints: >= 95 %
    of the exact ones in common (the bar of test_superpoint_fp16_arithmetic_is_a_tolerance_mode).  Score map: max |fp16 - exact| <= SCORE_BAR = 1.25 x
    what the retired k_sp_conv_h (the form this kernel replaced) measured against exact f32 on this image; the quarter covers the fp16-ulp
    differences that two summation orders propagate through twelve layers.  profiles/sp_retire.json ("fp16_score_bar") records the retired form's
    figure, the shipped form's own and the bar.  And the pass is repeatable run to run."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    eng = PoseEngine(0, max_batch=1, max_kpts=128, precision="f16x2_f16_attn", feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=1024, state_dict=osp.synthetic_state_dict(0), arithmetic="fp16")
    shape = (2, 1080, 1920)
    img = torch.from_numpy(np.random.default_rng(12).random(shape, dtype=np.float32)).cuda()
    npx = shape[0] * shape[1] * shape[2]

    def run(arithmetic):
        eng.sp_set_arithmetic(SuperPoint.ARITHMETIC[arithmetic])
        out = sp.detect_and_describe_device(img)
        torch.cuda.synchronize()
        return eng.debug_read("sp_scores", npx).copy(), [o.cpu().numpy().copy() if hasattr(o, "cpu") else np.asarray(o) for o in out]

    try:
        exact, new = run("exact_f32"), run("fp16")
        err = float(np.abs(exact[0] - new[0]).max())
        print(f"fp16 SuperPoint {shape}: max |scores(fp16) - scores(exact f32)| = {err:.6e} (bar {SCORE_BAR:.6e})")
        assert err <= SCORE_BAR
        for b in range(shape[0]):
            ka = {(float(x), float(y)) for x, y in exact[1][0][b, : int(exact[1][3][b]), :2]}
            kb = {(float(x), float(y)) for x, y in new[1][0][b, : int(new[1][3][b]), :2]}
            assert len(ka & kb) >= 0.95 * len(ka), (len(ka & kb), len(ka))
        for _ in range(6):
            again = run("fp16")
            assert np.array_equal(new[0], again[0]) and all(np.array_equal(a, b) for a, b in zip(new[1], again[1]))
    finally:
        eng.sp_set_arithmetic(SuperPoint.ARITHMETIC["fp16"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1080, 1920), (3, 248, 328), (1, 64, 40)])
def test_first_convolution_fused_into_the_second_gives_the_same_bits(shape):
    """Round 6: in the split-fp16 mode the network's first convolution (1 -> 64) is evaluated inside the halo staging of the second
    (k_sp_conv_s16<true, true, true>: the 0.53 GB-per-1080p-frame map between them is never written).  Same fma chain, same fp16 split, same LDS
    positions as k_sp_conv1 + LDS-DMA staging: score map, NMS map, keypoints, scores and descriptors are IDENTICAL to the two-launch form (knob 46 = 0)
    -- at the bench's frame size, at a size with ragged tiles on both axes, and at one smaller than a tile -- and repeatable."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.superpoint import SuperPoint
    from oracle import superpoint as osp
    eng = PoseEngine(0, max_batch=1, max_kpts=128, precision="f16x2_f16_attn", feature="superpoint")
    sp = SuperPoint(engine=eng, max_keypoints=512, state_dict=osp.synthetic_state_dict(0))
    img = torch.from_numpy(np.random.default_rng(21).random(shape, dtype=np.float32)).cuda()
    npx = shape[0] * shape[1] * shape[2]

    def run(fuse):
        eng.lib.gn_debug_set_variant(eng.ctx, 46, fuse)
        out = sp.detect_and_describe_device(img)
        torch.cuda.synchronize()
        return (eng.debug_read("sp_scores", npx).copy(), eng.debug_read("sp_nms", npx).copy(), [o.cpu().numpy().copy() if hasattr(o, "cpu") else np.asarray(o) for o in out])

    try:
        two = run(0)
        one = run(1)
        again = run(1)
    finally:
        eng.lib.gn_debug_set_variant(eng.ctx, 46, 1)
    assert np.array_equal(two[0].view(np.uint32), one[0].view(np.uint32)), "score map differs"
    assert np.array_equal(two[1].view(np.uint32), one[1].view(np.uint32))
    for a, b, c in zip(two[2], one[2], again[2]):
        assert np.array_equal(a, b) and np.array_equal(b, c)
    assert float(one[0].max()) > 0.0

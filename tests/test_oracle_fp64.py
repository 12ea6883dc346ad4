"""The float64 reference (oracle.lightglue_sift.pose_node_match(..., dtype=torch.float64)) that tests/test_gpu_fp64_parity.py measures the GPU
kernels against: the same code as the f32 oracle on float64 weights and inputs.  CPU only."""
import os

import numpy as np
import torch

from conftest import oracle_match
from gisnav_amd.synthetic import make_pair


def test_fp64_reference_taps_are_float64_and_within_1e5_of_the_f32_oracle(state_dict_t):
    from oracle import lightglue_sift as lg
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    tq = torch.from_numpy
    for p in (make_pair(40, n_q=300, n_r=280), make_pair(41, n_q=257, n_r=129)):
        t32, t64 = {}, {}
        r32 = oracle_match(state_dict_t, p, taps=t32)
        r64 = lg.pose_node_match(state_dict_t, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q),
                                 tq(p.kp_r), tq(p.desc_r), tq(p.size_r), tq(p.angle_r), taps=t64, dtype=torch.float64)
        keys = [f"layer{i}_{s}" for i in range(9) for s in (0, 1)] + ["scores"]
        for k in keys:
            assert t64[k].dtype == torch.float64, k
            a, b = t32[k].double().numpy(), t64[k].numpy()
            assert a.shape == b.shape, k
            rel = np.abs(a - b).max() / np.abs(b).max()
            assert rel <= 1e-5, (k, rel)
        assert t64["scores"].shape == (1, len(p.kp_q) + 1, len(p.kp_r) + 1)
        assert r64[2].dtype == torch.float64
        assert np.array_equal(r32[3].numpy(), r64[3].numpy()) and len(r64[3]) > 15


def test_loftr_stage_entry_points_compose_to_the_whole_model_bitwise():
    """tests/test_gpu_fp64_loftr.py feeds each stage of oracle/loftr.py its own input: chained on the oracle's own outputs, the entry points
    are the whole model, bit for bit."""
    from oracle import loftr as lf
    sd = lf.synthetic_state_dict(0)
    h, w = 96, 128
    i0, i1 = lf.synthetic_pair(3, h, w)
    taps = {}
    ref = lf.loftr_forward(sd, i0, i1, taps=taps)
    with torch.inference_mode():
        _, x1 = lf.backbone_layer1(sd, torch.stack([i0, i1])[:, None])
        x2, x3 = lf.backbone_layer23(sd, x1)
        x3_out = lf.layer3_outconv(sd, x3)
        x2_out, x1_out = lf.fpn_head(sd, x1, x2, x3_out)
        f0, f1 = lf.coarse_transformer(sd, x3_out)
        b, i, j, conf, k0, k1 = lf.coarse_matching(f0, f1, (h // 8, w // 8), (h // 8, w // 8), 8)
        k0f, k1f = lf.fine_level(sd, x1_out, f0, f1, b, i, j, k0, k1)
    for name, t in (("x1", x1), ("x3", x3), ("x3_out", x3_out), ("x2_out", x2_out), ("x1_out", x1_out)):
        assert torch.equal(t, taps[name]), name
    assert torch.equal(f0, taps["loftr_coarse.7"][0]) and torch.equal(f1, taps["loftr_coarse.7"][1])
    assert torch.equal(i, ref["i_ids"]) and torch.equal(j, ref["j_ids"]) and torch.equal(conf, ref["confidence"]) and len(i) > 20
    assert torch.equal(k0f, ref["keypoints0"]) and torch.equal(k1f, ref["keypoints1"])


def test_loftr_fp64_reference_is_float64_and_within_f32_rounding_of_the_f32_oracle():
    """oracle.loftr.loftr_forward(..., dtype=torch.float64): every tap float64, within f32 rounding of the f32 run (measured 3.5e-7 .. 1.7e-6 on
    the features, 1.7e-5 on the dual-softmax matrix), the same coarse correspondences, fine keypoints within 1e-3 px.  The border-only 32 x 32
    pair (no match) runs its fine level on empty windows in float64 too."""
    from oracle import loftr as lf
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    sd = lf.synthetic_state_dict(0)
    for h, w, seed in ((96, 128, 3), (136, 200, 2), (32, 32, 1)):
        i0, i1 = lf.synthetic_pair(seed, h, w)
        t32, t64 = {}, {}
        r32 = lf.loftr_forward(sd, i0, i1, taps=t32)
        r64 = lf.loftr_forward(sd, i0, i1, taps=t64, dtype=torch.float64)
        for k, bound in (("x1", 1e-5), ("x2", 1e-5), ("x3", 1e-5), ("x3_out", 1e-5), ("x2_out", 1e-5), ("x1_out", 1e-5), ("loftr_coarse.7", 1e-5),
                         ("sim_matrix", 1e-5), ("conf_matrix", 1e-4), ("fine_windows", 1e-5)):
            a, b = t32[k], t64[k]
            if isinstance(a, tuple):
                a, b = torch.cat(a), torch.cat(b)
            assert b.dtype == torch.float64 and a.shape == b.shape, k
            if b.numel():
                assert float((a.double() - b).abs().max() / b.abs().max()) <= bound, k
        for k in ("confidence", "keypoints0", "keypoints1", "keypoints1_c"):
            assert r64[k].dtype == torch.float64, k
        assert torch.equal(r32["i_ids"], r64["i_ids"]) and torch.equal(r32["j_ids"], r64["j_ids"])
        assert len(r64["i_ids"]) > (20 if h > 32 else -1)
        if len(r64["i_ids"]):
            assert float((r32["confidence"].double() - r64["confidence"]).abs().max()) <= 1e-4
            assert float((r32["keypoints1"].double() - r64["keypoints1"]).abs().max()) <= 1e-3
        assert torch.equal(r32["keypoints0"].double(), r64["keypoints0"])


def test_superpoint_lightglue_fp64_reference_is_float64_and_within_1e5_of_the_f32_oracle():
    """oracle.lightglue_superpoint.match(..., dtype=torch.float64) -- the reference of the 256-d cases in tests/test_gpu_fp64_parity.py -- with the
    keypoint extent and with a stated image size (the size tensors follow dtype)."""
    from gisnav_amd.synthetic import make_pair_256
    from gisnav_amd.weights import synthetic_state_dict
    from oracle import lightglue_superpoint as lsp
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(0, feature="superpoint").items()}
    tq = torch.from_numpy
    for p, hw in ((make_pair_256(40, n_q=300, n_r=280, h=480, w=640), None), (make_pair_256(41, n_q=257, n_r=129, h=480, w=640), (480, 640))):
        t32, t64 = {}, {}
        r32 = lsp.match(sd, tq(p.kp_q), tq(p.desc_q), tq(p.kp_r), tq(p.desc_r), hw0=hw, hw1=hw, taps=t32)
        r64 = lsp.match(sd, tq(p.kp_q), tq(p.desc_q), tq(p.kp_r), tq(p.desc_r), hw0=hw, hw1=hw, taps=t64, dtype=torch.float64)
        for k in [f"layer{i}_{s}" for i in range(9) for s in (0, 1)] + ["scores"]:
            assert t64[k].dtype == torch.float64, k
            a, b = t32[k].double().numpy(), t64[k].numpy()
            assert a.shape == b.shape, k
            assert np.abs(a - b).max() / np.abs(b).max() <= 1e-5, k
        assert r64[0].dtype == torch.float64 and np.array_equal(r32[1].numpy(), r64[1].numpy()) and len(r64[1]) > 15


def _superpoint_chain(sd, img, k, dtype):
    """oracle/superpoint.py's stage entry points chained on their own outputs, in `dtype`"""
    from oracle import superpoint as osp
    sd = osp.cast_state_dict(sd, dtype)
    t = {}
    with torch.inference_mode():
        x = img.to(dtype)[None, None]
        for i in range(8):
            x = t[f"layer{i}"] = osp.conv_layer(sd, i, x)
        t["layer8"] = osp.conv_layer(sd, 8, x)
        t["logits"] = osp.conv_layer(sd, 9, t["layer8"])
        t["cell_scores"] = osp.cell_scores(t["logits"])
        t["scores"] = osp.simple_nms(t["cell_scores"], osp.NMS_RADIUS)
        kp, sc, idx = osp.select(t["scores"], k)
        t["layer10"] = osp.conv_layer(sd, 10, x)
        t["raw_dmap"] = osp.conv_layer(sd, 11, t["layer10"])
        d = osp.sample_descriptors(kp, t["raw_dmap"])
    return kp, sc, d, idx, t


def _in_select_order(kp, sc, d, w):
    """extract_keypoints leaves the list in raster order when it holds no more than k candidates (torch.topk only runs beyond k): the same rows, score
    descending then raster index ascending"""
    idx = (kp[:, 1] * w + kp[:, 0]).long()
    order = sorted(range(len(kp)), key=lambda i: (-float(sc[i]), int(idx[i])))
    return kp[order], sc[order], d[order]


SP_TAPS = [f"layer{i}" for i in range(9)] + ["layer10", "logits", "raw_dmap", "cell_scores", "scores"]


def test_superpoint_stage_entry_points_compose_to_the_whole_model_bitwise():
    """tests/test_gpu_fp64_superpoint.py feeds each stage of oracle/superpoint.py its own input: chained on the oracle's own f32 outputs, the entry
    points are detect_and_describe, bit for bit -- every tap, and (the test image's candidate scores are distinct, asserted) keypoints, scores and
    descriptors in order, with fewer candidates than k and with more."""
    from oracle import superpoint as osp
    from test_superpoint import _test_image
    sd = osp.synthetic_state_dict(0)
    for seed, (h, w), k in ((4, (136, 200), 2048), (4, (136, 200), 300), (2, (64, 40), 300)):
        img = torch.from_numpy(_test_image(seed, h, w))
        taps = {}
        kp, sc, d = _in_select_order(*osp.detect_and_describe(sd, img, k, taps=taps), w)
        ckp, csc, cd, cidx, ct = _superpoint_chain(sd, img, k, torch.float32)
        for name in SP_TAPS:
            assert torch.equal(taps[name], ct[name]), name
        allsc = osp.select(ct["scores"], -1)[1]
        assert len(torch.unique(allsc)) == len(allsc) > 0, "the test image has tied candidate scores"
        assert (len(allsc) > k) == (k == 300 and h == 136)
        assert len(kp) == min(k, len(allsc))
        assert torch.equal(kp, ckp) and torch.equal(sc, csc) and torch.equal(d, cd)
        assert torch.equal(cidx, (ckp[:, 1] * w + ckp[:, 0]).long())


def test_superpoint_fp64_reference_is_float64_and_within_1e5_of_the_f32_oracle():
    """detect_and_describe(..., dtype=torch.float64): every tap float64 and within 1e-5 of the f32 run (convolutions relative to max |fp64|, the
    softmax scores absolute), the same keypoints in the same order on the tie-free test image; the chained fp64 entry points give the same."""
    from oracle import superpoint as osp
    from test_superpoint import _test_image
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    sd = osp.synthetic_state_dict(0)
    for seed, (h, w), k in ((4, (136, 200), 300), (2, (64, 40), 300), (3, (16, 520), 300)):
        img = torch.from_numpy(_test_image(seed, h, w))
        t32, t64 = {}, {}
        kp32, sc32, d32 = osp.detect_and_describe(sd, img, k, taps=t32)
        kp64, sc64, d64 = osp.detect_and_describe(sd, img, k, taps=t64, dtype=torch.float64)
        (kp32, sc32, d32), (kp64, sc64, d64) = _in_select_order(kp32, sc32, d32, w), _in_select_order(kp64, sc64, d64, w)
        for name in SP_TAPS + ["dmap"]:
            a, b = t32[name], t64[name]
            assert b.dtype == torch.float64 and a.dtype == torch.float32 and a.shape == b.shape, name
            err = float((a.double() - b).abs().max())
            if name not in ("cell_scores", "scores"):
                err /= float(b.abs().max())
            assert err <= 1e-5, (name, err)
        assert kp64.dtype == sc64.dtype == d64.dtype == torch.float64
        assert len(kp64) > 0 and torch.equal(kp32.double(), kp64)
        assert float((sc32.double() - sc64).abs().max()) <= 1e-5 and float((d32.double() - d64).abs().max()) <= 1e-5
        ckp, csc, cd, _, ct = _superpoint_chain(sd, img, k, torch.float64)
        assert all(ct[name].dtype == torch.float64 for name in SP_TAPS)
        assert torch.equal(ckp, kp64) and torch.equal(csc, sc64) and torch.equal(cd, d64)


def test_superpoint_select_is_the_transformers_set_on_distinct_scores_and_ordered_on_ties():
    """select(nms, k): the set extract_keypoints (the transformers pin) returns whenever the scores are distinct; on tied scores -- where torch.topk's
    order is unspecified -- score descending, then raster index ascending, the order k_sp_select documents."""
    from oracle import superpoint as osp
    g = torch.Generator().manual_seed(5)
    for h, w, k in ((24, 40, 10), (24, 40, 200), (24, 40, 5000), (16, 16, 7)):
        m = torch.rand(1, h, w, generator=g) * 0.02                   # about 3 / 4 of the pixels above the 0.005 threshold
        assert len(torch.unique(m)) == m.numel()
        kp, sc, idx = osp.select(m, k)
        ekp, esc = osp.extract_keypoints(m, k)
        n_cand = int(((m[0] > osp.KEYPOINT_THRESHOLD)[osp.BORDER:, osp.BORDER:]).sum())
        assert len(kp) == min(k, n_cand) == len(ekp)
        assert {(float(x), float(y), float(s)) for (x, y), s in zip(kp, sc)} == {(float(x), float(y), float(s)) for (x, y), s in zip(ekp, esc)}
        assert bool((sc[:-1] > sc[1:]).all()) and bool((kp >= osp.BORDER).all())
    # ties: three score levels over a 16 x 24 map, far border pixels included (never tested against the far border), near borders excluded
    m = torch.zeros(1, 16, 24)
    m[0, 2:, 2:] = torch.tensor([0.25, 0.5, 0.004])[torch.randint(0, 3, (14, 22), generator=g)]
    want = sorted(((-float(m[0, y, x]), y * 24 + x) for y in range(4, 16) for x in range(4, 24) if m[0, y, x] > 0.005))
    for k in (1, 17, len(want) - 1, len(want), len(want) + 5):
        kp, sc, idx = osp.select(m, k)
        assert [(-float(s), int(i)) for s, i in zip(sc, idx)] == want[:k]
        assert torch.equal(kp, torch.stack([idx % 24, idx // 24], 1).float())

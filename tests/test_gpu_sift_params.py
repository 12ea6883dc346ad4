"""SIFT with cv2.SIFT_create's nOctaveLayers / contrastThreshold / edgeThreshold / sigma on the device (gn_sift_set_params) against the unchanged
oracle: every keypoint field and every descriptor value bit for bit, whatever path a pyramid level takes (fused blur, two-launch blur,
single-workgroup tail)."""
import ctypes as CT
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_params_common as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=1, max_kpts=128, precision="f32")


def _sift(eng, params, **kw):
    from gisnav_amd.sift import SIFT
    nl, ct, et, sg = params
    return SIFT(engine=eng, max_keypoints=4096, nOctaveLayers=nl, contrastThreshold=ct, edgeThreshold=et, sigma=sg, **kw)


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else None


@pytest.mark.parametrize("params,shape", C.PARITY_CASES, ids=_ids)
def test_parity_with_the_oracle_for_non_default_parameters(eng, params, shape):
    o = C.oracle(shape, params)
    assert len(o["kp"]) >= 10 and C.keyset(o) != C.keyset(C.oracle(shape, C.DEFAULT))      # the case exercises its parameters
    C.assert_bit_equal(_sift(eng, params).detect_and_compute_device(C.image(shape)), o)


def test_parity_at_the_frame_size(eng):
    """480 x 640: k_sift_tail takes octaves 4-8 and the fused-blur tile table differs."""
    params, key = (4, 0.02, 8.0, 1.4), ((480, 640), 3, 500, 120)
    o = C.oracle(key[0], params, *key[1:])
    assert len(o["kp"]) > 100
    C.assert_bit_equal(_sift(eng, params).detect_and_compute_device(C.image(*key)), o)


@pytest.mark.parametrize("params", [(5, 0.03, 12.0, 1.6), (2, 0.04, 10.0, 1.6)], ids=_ids)
def test_batch_equals_image_by_image(eng, params):
    imgs = np.stack([C.ridge_image(20 + b, 97, 131, 60, 30) for b in range(3)])         # odd sides: unaligned rows, partial tiles
    s = _sift(eng, params)
    singles = [tuple(t.cpu().numpy().copy() for t in s.detect_and_compute_device(im)) for im in imgs]
    kpt, resp, octv, desc, n = s.detect_and_compute_batch_device(imgs)
    assert min(len(sk[0]) for sk in singles) > 20
    for b in range(3):
        sk, sr, so, sd = singles[b]
        assert n[b] == len(sk)
        assert np.array_equal(kpt[b, : n[b]].cpu().numpy().view(np.int32), sk.view(np.int32))
        assert np.array_equal(resp[b, : n[b]].cpu().numpy().view(np.int32), sr.view(np.int32))
        assert np.array_equal(octv[b, : n[b]].cpu().numpy(), so)
        assert np.array_equal(desc[b, : n[b]].cpu().numpy().view(np.int32), sd.view(np.int32))


def _raw_call(e, img, cap=4096):
    """gn_sift_detect_and_compute with whatever parameters the context holds (no SIFT object in between)."""
    import torch
    from gisnav_amd import _lib
    from gisnav_amd.engine import _ptr
    t = torch.as_tensor(np.array(img), device=e.device)                         # (a writable copy: the shared image is read-only)
    kpt = torch.zeros((cap, 4), dtype=torch.float32, device=e.device); resp = torch.zeros((cap,), dtype=torch.float32, device=e.device)
    octv = torch.zeros((cap,), dtype=torch.int32, device=e.device); desc = torch.zeros((cap, 128), dtype=torch.float32, device=e.device)
    n = CT.c_int32(0)
    _lib.check(e.ctx, e.lib.gn_sift_detect_and_compute(e.ctx, _ptr(t), img.shape[0], img.shape[1], cap, _ptr(kpt), _ptr(resp), _ptr(octv), _ptr(desc),
                                                       CT.byref(n), e._stream()), "gn_sift_detect_and_compute")
    return n.value, b"".join(x.cpu().numpy().tobytes() for x in (kpt, resp, octv, desc))


def test_default_parameters_are_the_untold_context_and_state_is_per_object(eng):
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.sift import SIFT
    img = C.image(C.LARGE)
    fresh = PoseEngine(0, max_batch=1, max_kpts=128, precision="f32")
    want = _raw_call(fresh, img)                                                     # never told
    assert want[0] == 78
    assert fresh.lib.gn_sift_set_params(fresh.ctx, 3, 0.04, 10.0, 1.6) == 0
    assert _raw_call(fresh, img) == want
    assert fresh.lib.gn_sift_set_params(fresh.ctx, 4, 0.02, 8.0, 1.4) == 0
    assert _raw_call(fresh, img)[0] == 109
    assert fresh.lib.gn_sift_set_params(fresh.ctx, 3, 0.04, 10.0, 1.6) == 0
    assert _raw_call(fresh, img) == want                                             # and back
    C.assert_bit_equal(SIFT(engine=fresh, max_keypoints=4096).detect_and_compute_device(img), C.oracle(C.LARGE, C.DEFAULT))
    a, b = SIFT(engine=eng, max_keypoints=4096), SIFT(engine=eng, max_keypoints=4096, contrastThreshold=0.01)
    for _ in range(2):
        assert len(a.detect_and_compute_device(img)[0]) == 78 and len(b.detect_and_compute_device(img)[0]) == 179


def test_results_do_not_depend_on_the_path_a_level_takes(eng):
    """nOctaveLayers = 1: 23 / 45 / 91 taps -- the fused launch, the two-launch form, no tail -- and octaves narrower than the kernel radius
    (BORDER_REFLECT_101 folded more than once)."""
    params = (1, 0.04, 10.0, 1.6)
    C.assert_bit_equal(_sift(eng, params).detect_and_compute_device(C.image(C.SMALL)), C.oracle(C.SMALL, params))


def test_argument_errors_through_the_c_abi(eng):
    from gisnav_amd import _lib
    lib, ctx = eng.lib, eng.ctx
    assert lib.gn_sift_set_params(ctx, 2, 0.03, 7.0, 1.3) == 0
    bad = [(0, 0.04, 10.0, 1.6), (6, 0.04, 10.0, 1.6), (3, 0.04, 10.0, 0.9), (3, 0.04, 10.0, 2.5), (3, 0.04, 0.0, 1.6), (3, float("nan"), 10.0, 1.6)]
    for args in bad:
        assert lib.gn_sift_set_params(ctx, *args) == -1                              # GN_ERR_ARG
        msg = lib.gn_last_error(ctx)
        assert msg and b"gn_sift_set_params" in msg
        nl, ct, et, sg = CT.c_int(0), CT.c_double(0), CT.c_double(0), CT.c_double(0)
        assert lib.gn_sift_get_params(ctx, CT.byref(nl), CT.byref(ct), CT.byref(et), CT.byref(sg)) == 0
        assert (nl.value, ct.value, et.value, sg.value) == (2, 0.03, 7.0, 1.3)      # what was in effect before the call
    with pytest.raises(_lib.GnError):
        _lib.check(ctx, lib.gn_sift_set_params(ctx, 0, 0.04, 10.0, 1.6), "gn_sift_set_params")
    assert lib.gn_sift_set_params(ctx, 3, 0.04, 10.0, 1.6) == 0


def test_pose_node_forwards_sift_params(state_dict_np):
    from gisnav_amd import wire
    from gisnav_amd.pose_node import PoseNode
    from gisnav_amd.synthetic import K_MATRIX
    img = C.image(C.LARGE)
    cam = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    msg = wire.OrthoStereoImage(query_sift=b"", reference=wire.ImageMsg(np.array(img), wire.Stamp(3, 0)),
                                dem=wire.ImageMsg(np.zeros_like(img), wire.Stamp(3, 0)))
    for kw, want in (({"sift_params": {"contrastThreshold": 0.01}}, 179), ({}, 78)):
        node = PoseNode(state_dict_np, max_kpts=512, precision="f32", **kw)
        assert node.estimate(cam, msg) is None and node._cached_n_r == want          # the reference side is cached at the first message

"""Shared by tests/test_sift_params_host.py and tests/test_gpu_sift_params.py: the blob + ridge test image, the parameter rows with the
keypoint counts the oracle gives for them, and the oracle chain (computed once per (image, parameters) and shared)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import sift as osift  # noqa: E402

DEFAULT = (3, 0.04, 10.0, 1.6)
SMALL, LARGE = (96, 128), (200, 264)
# (nOctaveLayers, contrastThreshold, edgeThreshold, sigma) -> keypoints after sort_and_dedup at 96 x 128 and at 200 x 264
COUNTS = {
    (3, 0.04, 10.0, 1.6): (52, 78),
    (3, 0.04, 2.0, 1.6): (15, 49),
    (3, 0.04, 4.0, 1.6): (40, 66),
    (3, 0.04, 30.0, 1.6): (52, 82),      # at 96 x 128: the same set as the default
    (3, 0.01, 10.0, 1.6): (82, 179),
    (3, 0.09, 10.0, 1.6): (14, 15),
    (2, 0.04, 10.0, 1.6): (56, 74),
    (4, 0.04, 10.0, 1.6): (56, 80),
    (5, 0.03, 12.0, 1.6): (69, 91),
    (1, 0.04, 10.0, 1.6): (47, 79),
    (3, 0.04, 10.0, 1.2): (46, 71),
    (3, 0.04, 10.0, 2.0): (55, 84),
    (4, 0.02, 8.0, 1.4): (65, 109),
}
NON_DEFAULT = [p for p in COUNTS if p != DEFAULT]
# every cell whose keypoint set differs from the default's
PARITY_CASES = [(p, shape) for p in NON_DEFAULT for shape in (SMALL, LARGE) if not (p == (3, 0.04, 30.0, 1.6) and shape == SMALL)]


def blob_image(seed, h=240, w=320, n=150):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w))
    for _ in range(n):
        cx, cy, s, a = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 9), rng.uniform(-80, 80)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(128 + img + rng.normal(0, 2, (h, w)), 0, 255).astype(np.uint8)


def ridge_image(seed, h, w, n_blobs, n_ridges):
    """blob_image is isotropic (edgeThreshold never fires on it): anisotropic Gaussian ridges on top."""
    rng = np.random.default_rng(1000 + seed)
    img = blob_image(seed, h, w, n=n_blobs).astype(float)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_ridges):
        cx, cy, th = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0, np.pi)
        sl, ss, a = rng.uniform(6, 14), rng.uniform(1.5, 3.5), rng.uniform(-70, 70)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img += a * np.exp(-u ** 2 / (2 * sl ** 2) - v ** 2 / (2 * ss ** 2))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(shape, seed=3, n_blobs=100, n_ridges=60):
    img = ridge_image(seed, shape[0], shape[1], n_blobs, n_ridges)
    img.setflags(write=False)
    return img


def oracle_of(img, params):
    """build_pyramids -> detect(pyramids=) -> sort_and_dedup -> compute, as oracle.sift.detect_and_compute composes them."""
    nl, ct, et, sg = params
    pyr = osift.build_pyramids(img, nl, sg)
    kpts = osift.sort_and_dedup(osift.detect(img, nl, ct, et, sg, pyramids=pyr))
    desc = osift.compute(pyr[0], kpts)
    F = np.float32
    g = lambda name, dt: np.array([k[name] for k in kpts], dt)  # noqa: E731
    kp = np.stack([g("x", F), g("y", F)], 1) if kpts else np.zeros((0, 2), F)
    out = dict(kp=kp, size=g("size", F), angle=g("angle", F), response=g("response", F), octave=g("octave", np.int32), desc=desc)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, params, seed=3, n_blobs=100, n_ridges=60):
    return oracle_of(image(shape, seed, n_blobs, n_ridges), params)


def keyset(o):
    """The keypoint set as bit patterns (position, size, angle, packed octave)."""
    return set(zip(o["kp"][:, 0].view(np.int32).tolist(), o["kp"][:, 1].view(np.int32).tolist(), o["size"].view(np.int32).tolist(),
                   o["angle"].view(np.int32).tolist(), o["octave"].tolist()))


def assert_bit_equal(got, o):
    """got = (kpt_xysa, response, octave, desc) device tensors or arrays; o = oracle dict.  No tolerance, nothing left out."""
    k, r, oc, d = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in got)
    assert len(k) == len(o["kp"])
    assert np.array_equal(np.ascontiguousarray(k[:, :2]).view(np.int32), o["kp"].view(np.int32))
    assert np.array_equal(np.ascontiguousarray(k[:, 2]).view(np.int32), o["size"].view(np.int32))
    assert np.array_equal(np.ascontiguousarray(k[:, 3]).view(np.int32), o["angle"].view(np.int32))
    assert np.array_equal(r.view(np.int32), o["response"].view(np.int32))
    assert np.array_equal(oc, o["octave"])
    assert np.array_equal(d.view(np.int32), o["desc"].view(np.int32))

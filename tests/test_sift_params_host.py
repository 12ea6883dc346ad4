"""SIFT parameters (nOctaveLayers, contrastThreshold, edgeThreshold, sigma), host side: the oracle's keypoint counts for the rows the GPU tests
compare against, the range checks of SIFT(...) / PoseNode(sift_params=...) before any context exists, and the two C ABI symbols."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_params_common as C  # noqa: E402

ROOT = C.ROOT


@pytest.mark.parametrize("params", list(C.COUNTS), ids=lambda p: "-".join(str(v) for v in p))
def test_oracle_keypoint_counts_of_the_parameter_rows(params):
    """Re-derived from the unchanged oracle: a later oracle edit that empties a case is caught here, not on the GPU."""
    small, large = C.oracle(C.SMALL, params), C.oracle(C.LARGE, params)
    assert (len(small["kp"]), len(large["kp"])) == C.COUNTS[params]
    if params != C.DEFAULT:      # the precondition of the parity test: a keypoint set of its own, except the one cell that has none
        for shape, o in ((C.SMALL, small), (C.LARGE, large)):
            differs = C.keyset(o) != C.keyset(C.oracle(shape, C.DEFAULT))
            assert differs == ((params, shape) in C.PARITY_CASES)
            assert len(o["kp"]) >= 10


def test_range_errors_are_raised_before_a_context_exists(monkeypatch):
    from gisnav_amd import engine, pose_node, sift

    def no_engine(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(engine.PoseEngine, "__init__", no_engine)
    bad = [dict(nOctaveLayers=0), dict(nOctaveLayers=6), dict(nOctaveLayers=2.5), dict(nOctaveLayers=float("inf")), dict(nOctaveLayers="3"), dict(sigma=0.9), dict(sigma=2.5), dict(sigma=float("nan")),
           dict(edgeThreshold=0.0), dict(edgeThreshold=-1.0), dict(edgeThreshold=float("inf")), dict(contrastThreshold=float("nan")),
           dict(contrastThreshold=-0.01), dict(contrastThreshold=float("inf")), dict(nfeatures=-1), dict(nfeatures=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            sift.SIFT(**kw)
        with pytest.raises(ValueError):
            pose_node.PoseNode({}, sift_params=kw)
    with pytest.raises(ValueError):
        pose_node.PoseNode({}, sift_params={"contrast": 0.01})                  # not one of cv2's keyword names
    with pytest.raises(ValueError):
        pose_node.PoseNode({}, extractor=lambda ref: None, sift_params={"contrastThreshold": 0.01})
    # the accepted corners reach the engine (which this test has replaced)
    for kw in (dict(nOctaveLayers=1, sigma=1.0), dict(nOctaveLayers=5, sigma=2.4, contrastThreshold=0.0, edgeThreshold=1e-3), dict(nfeatures=100)):
        assert sift.check_sift_params(**kw)[1:] == (kw.get("nOctaveLayers", 3), kw.get("contrastThreshold", 0.04), kw.get("edgeThreshold", 10.0), kw.get("sigma", 1.6))
        with pytest.raises(AssertionError, match="context was created"):
            sift.SIFT(**kw)


def test_nfeatures_sets_the_cap_and_the_parameters_belong_to_the_object():
    from gisnav_amd import sift

    class Eng:                      # no device: only the constructor's bookkeeping is looked at
        pass
    a = sift.SIFT(engine=Eng(), max_keypoints=4096, nfeatures=300, contrastThreshold=0.01)
    b = sift.SIFT(engine=a._eng)
    assert a._max == 300 and b._max == 8192
    assert a._params == [3, 0.01, 10.0, 1.6] and b._params == [3, 0.04, 10.0, 1.6]


def test_symbols_declared_and_exported():
    from gisnav_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gisnav_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gn_sift_set_params", "gn_sift_get_params"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in include/gisnav_amd.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES
    assert "with OpenCV's defaults" not in hdr

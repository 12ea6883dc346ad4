"""iterations_count above 16 in the PnP stage, the parts that need no GPU (DESIGN.md "RANSAC beyond 16 hypotheses"; the GPU side is
tests/test_gpu_ransac_iterations.py).

  1. tests/golden/pnp_ransac_iters.npz holds what the oracle returns: scene A at 17 and 64, scene B at 16 and 17, scene D at 10 and 64 are derived
     again here (188 oracle hypotheses), scenes and results; the round-boundary counts are in the fixture;
  2. the header declares gn_set_ransac / gn_get_ransac / gn_ransac_last_counts and GN_RANSAC_MAX_ITERATIONS, the built library exports them with
     the argument types _lib.py declares;
  3. the Python layers refuse a bad count before any device work and pass a good one on.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from gisnav_amd.synthetic import K_MATRIX
from oracle import pnp_ransac as pr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ransac_iters_golden as gen  # noqa: E402

G = np.load(gen.OUT)


@pytest.mark.parametrize("name,counts", [("A", (17, 64)), ("B", (16, 17)), ("D", (10, 64))])
def test_fixture_rows_are_what_the_oracle_returns(name, counts):
    obj, img = gen.scene(*gen.SCENES[name])
    assert np.array_equal(obj, G[f"{name}_obj"]) and np.array_equal(img, G[f"{name}_img"])
    assert np.array_equal(G["K"], K_MATRIX)
    for c in counts:
        i = int(np.nonzero(G[f"{name}_counts"] == c)[0][0])
        ok, n_inl, R, t, niters, inl = gen.run(lambda k: pr.solve_pnp_ransac(obj, img, K_MATRIX, k), pr, c)
        assert (ok, n_inl, niters) == (int(G[f"{name}_ok"][i]), int(G[f"{name}_ninl"][i]), int(G[f"{name}_niters"][i])), (name, c)
        assert np.array_equal(R, G[f"{name}_R"][i]) and np.array_equal(t, G[f"{name}_t"][i])
        assert np.array_equal(np.nonzero(G[f"{name}_inl"][i])[0], inl)


def test_fixture_covers_the_round_boundaries_and_the_listed_facts():
    R = int(G["round"])
    assert R == gen.ROUND == 64
    src = open(os.path.join(HERE, "..", "gisnav_amd", "csrc", "gn_common.h")).read()
    assert re.search(r"#define GN_RANSAC_ROUND\s+%d\b" % R, src)                       # the kernels' round size is the fixture's
    for name in ("A", "B"):
        assert {R - 1, R, R + 1, 2 * R + 1} <= set(G[f"{name}_counts"].tolist())
    ninl = lambda name: dict(zip(G[f"{name}_counts"].tolist(), G[f"{name}_ninl"].tolist()))  # noqa: E731
    a, b = ninl("A"), ninl("B")
    assert [a[c] for c in (10, 16, 17)] == [0, 0, 0] and all(a[c] == 30 for c in (63, 64, 65, 129, 144, 145, 146, 300, 4096))
    assert (b[16], b[17]) == (6, 7) and all(b[c] == 8 for c in (63, 64, 65, 128, 129)) and b[300] == 120
    assert int(G["A_niters"][-1]) == 145 and int(G["B_niters"][-1]) == 447
    assert not G["C_ok"].any() and ninl("D") == {10: 26, 64: 30} and ninl("E") == {10: 0, 17: 0, 64: 36, 300: 36}
    solved = {c: [i for i in range(8) if G[f"P{i}_ok"][list(G[f"P{i}_counts"]).index(c)]] for c in (10, 100, 300)}
    assert solved == {10: [1, 3, 4, 5], 100: [0, 1, 3, 4, 5, 6, 7], 300: list(range(8))}
    assert int(G["clean_ok"][0]) == 1 and int(G["clean_niters"][0]) < R                # the clean scene stops inside the first round
    assert os.path.getsize(gen.OUT) < 100 * 1024


def test_symbols_are_declared_exported_and_bound():
    from gisnav_amd import _lib, build
    header = open(os.path.join(HERE, "..", "include", "gisnav_amd.h")).read()
    assert re.search(r"#define GN_RANSAC_MAX_ITERATIONS\s+4096\b", header) and _lib.GN_RANSAC_MAX_ITERATIONS == 4096
    for decl in (r"int gn_set_ransac\(gn_ctx\* ctx, int iterations_count, float reproj_error_px, double confidence\);",
                 r"int gn_get_ransac\(const gn_ctx\* ctx, int\* iterations_count, float\* reproj_error_px, double\* confidence\);",
                 r"int gn_ransac_last_counts\(gn_ctx\* ctx, int B, int32_t\* niters_host, int32_t\* evaluated_host, void\* stream\);"):
        assert re.search(decl, header), decl
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = {"gn_set_ransac": [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double],
            "gn_get_ransac": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), _lib.c_f32p, _lib.c_f64p],
            "gn_ransac_last_counts": [ctypes.c_void_p, ctypes.c_int, _lib.c_i32p, _lib.c_i32p, ctypes.c_void_p]}
    lib = _lib.load()
    for name, args in want.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    # the argument checks that need no context
    assert lib.gn_set_ransac(None, 10, 8.0, 0.99) < 0 and lib.gn_get_ransac(None, None, None, None) < 0
    assert lib.gn_ransac_last_counts(None, 1, None, None, None) < 0


def test_python_layers_refuse_a_bad_count_before_any_device_work():
    from gisnav_amd import wire
    from gisnav_amd.engine import check_ransac_iterations
    from gisnav_amd.loftr import _iterations_kw
    from gisnav_amd.pose import compute_pose
    from gisnav_amd.pose_node import PoseNode
    from gisnav_amd.vo import twist_pose
    assert check_ransac_iterations(1) == 1 and check_ransac_iterations(np.int64(4096)) == 4096
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="1..4096"):
            check_ransac_iterations(bad)
    for bad in (10.0, "10", True, None):
        with pytest.raises(TypeError):
            check_ransac_iterations(bad)
    info = wire.CameraInfo(k=K_MATRIX.reshape(9))
    pts = np.zeros((3, 2), np.float32)                                               # < 4 points: "no pose" before any device work
    assert compute_pose(info, pts, pts, None, ransac_iterations=300) is None
    assert compute_pose(info, pts, pts, None) is None
    with pytest.raises(ValueError):
        compute_pose(info, pts, pts, None, ransac_iterations=0)
    with pytest.raises(ValueError):
        PoseNode({}, ransac_iterations=5000)                                         # (refused before a context is created)
    with pytest.raises(ValueError):
        twist_pose(None, K_MATRIX, np.zeros((40, 2)), None, np.zeros((40, 2)), None, ransac_iterations=0)
    assert _iterations_kw(None) == {} and _iterations_kw(300) == {"iterations": 300}
    with pytest.raises(ValueError):
        _iterations_kw(4097)

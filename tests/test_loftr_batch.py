"""Batched LoFTR (gn_loftr_create_batch / gn_loftr_match_batch, `LoFTR` on (B, 1, H, W) inputs, `loftr_pose_batch`): a pair's result does not
depend on B, on its place in the batch or on its neighbours, BIT FOR BIT -- so every comparison against a single-pair call is `torch.equal`;
against the oracle the bars are those of `test_loftr_hip_against_oracle` (ids identical, confidence 2e-4, fine keypoints 2e-3 px).

Inputs (oracle match counts): A 128x160 seed 1 (154), Z 128x160 constant 0.5 (0), C 128x160 seed 2 shifted (24, 16) (131), D 136x200 seed 2
(228), E 136x200 seed 5 shifted (24, 16) (199).  At 128x160 L = 320, Lp = 384; at 136x200 L = 425, Lp = 512 (L no multiple of 128).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import loftr as lf

KEYS = ("keypoints0", "keypoints1", "confidence", "i_ids", "j_ids")
_cache = {}


def _sd():
    if "sd" not in _cache:
        _cache["sd"] = lf.synthetic_state_dict(0)
    return _cache["sd"]


def _pair(name):
    """(image0, image1) on the CPU; "A*" is A scaled by 3e5 (past fp16's range inside the backbone)."""
    if name not in _cache:
        if name == "A":
            p = lf.synthetic_pair(1, 128, 160)
        elif name == "Z":
            p = (torch.full((128, 160), 0.5), torch.full((128, 160), 0.5))
        elif name == "C":
            p = lf.synthetic_pair(2, 128, 160, shift=(24, 16))
        elif name == "D":
            p = lf.synthetic_pair(2, 136, 200)
        elif name == "E":
            p = lf.synthetic_pair(5, 136, 200, shift=(24, 16))
        elif name == "A*":
            p = tuple(t * 3.0e5 for t in _pair("A"))
        else:
            raise KeyError(name)
        _cache[name] = p
    return _cache[name]


def _oracle(name):
    key = ("oracle", name)
    if key not in _cache:
        _cache[key] = lf.loftr_forward(_sd(), *_pair(name))
    return _cache[key]


def _matcher(**kw):
    from gisnav_amd.loftr import LoFTR
    return LoFTR(state_dict=_sd(), **kw).to("cuda:0").eval()


def _batch(names):
    return {"image0": torch.stack([_pair(n)[0] for n in names])[:, None].cuda(), "image1": torch.stack([_pair(n)[1] for n in names])[:, None].cuda()}


def _single(name, **kw):
    """The outputs of a single-pair call on `name`, from a single-pair matcher of its own per (size, settings); computed once."""
    key = ("single", name, tuple(sorted(kw.items())))
    if key not in _cache:
        mk = ("matcher", _pair(name)[0].shape, tuple(sorted(kw.items())))
        if mk not in _cache:
            _cache[mk] = _matcher(**kw)
        i0, i1 = _pair(name)
        out = _cache[mk]({"image0": i0.cuda(), "image1": i1.cuda()}, with_ids=True)
        _cache[key] = {k: v.cpu() for k, v in out.items()}
    return _cache[key]


def _assert_batch_equals_singles(out, names, singles):
    out = {k: v.cpu() for k, v in out.items()}
    counts = [int(s["keypoints0"].shape[0]) for s in singles]
    assert out["keypoints0"].shape[0] == sum(counts), (out["keypoints0"].shape, counts)
    assert torch.equal(out["batch_indexes"], torch.repeat_interleave(torch.arange(len(names)), torch.tensor(counts)))
    off = 0
    for b, (name, s) in enumerate(zip(names, singles)):
        assert int((out["batch_indexes"] == b).sum()) == counts[b], (name, b)
        for k in KEYS:
            assert torch.equal(out[k][off:off + counts[b]], s[k]), (name, b, k)
        off += counts[b]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("arithmetic", ["exact_f32", "split_fp16"])
def test_batch_equals_single_bitwise(arithmetic, graph):
    """[A, Z, C] (odd B: six sequences, an empty pair in the middle) and [D, E]; then the same context again with the order permuted (a replay
    of its graph) and with B = 2 < max_pairs = 3."""
    kw = dict(arithmetic=arithmetic, graph=graph)
    single = lambda n: _single(n, **kw)  # noqa: E731
    assert single("Z")["keypoints0"].shape[0] == 0 and single("A")["keypoints0"].shape[0] > 100 and single("C")["keypoints0"].shape[0] > 100
    m = _matcher(**kw)
    for names in (["A", "Z", "C"], ["C", "A", "Z"], ["C", "A"]):
        _assert_batch_equals_singles(m(_batch(names), with_ids=True), names, [single(n) for n in names])
        assert m._pairs == 3                                                      # one context: not re-created for the smaller batch
    m2 = _matcher(**kw)
    _assert_batch_equals_singles(m2(_batch(["D", "E"]), with_ids=True), ["D", "E"], [single("D"), single("E")])


@pytest.mark.gpu
def test_second_pair_of_a_batch_against_the_oracle():
    out = {k: v.cpu() for k, v in _matcher()(_batch(["D", "E"]), with_ids=True).items()}
    ref = _oracle("E")
    sel = out["batch_indexes"] == 1
    assert int(sel.sum()) == len(ref["i_ids"]) == 199
    assert torch.equal(out["i_ids"][sel], ref["i_ids"]) and torch.equal(out["j_ids"][sel], ref["j_ids"])
    assert torch.equal(out["keypoints0"][sel], ref["keypoints0"])
    dc = float((out["confidence"][sel] - ref["confidence"]).abs().max())
    dk = float((out["keypoints1"][sel] - ref["keypoints1"]).abs().max())
    print(f"confidence {dc:.3e} keypoints1 {dk:.3e}")
    assert dc < 2e-4 and dk < 2e-3


@pytest.mark.gpu
def test_truncation_is_per_pair():
    names = ["A", "C"]
    out = {k: v.cpu() for k, v in _matcher(max_matches=40)(_batch(names), with_ids=True).items()}
    assert torch.equal(out["batch_indexes"], torch.repeat_interleave(torch.arange(2), torch.tensor([40, 40])))
    for b, n in enumerate(names):
        ref, s = _oracle(n), _single(n, max_matches=40)
        assert len(ref["i_ids"]) > 40
        assert torch.equal(out["i_ids"][40 * b:40 * b + 40], ref["i_ids"][:40]) and torch.equal(out["j_ids"][40 * b:40 * b + 40], ref["j_ids"][:40])
        for k in KEYS:
            assert torch.equal(out[k][40 * b:40 * b + 40], s[k]), (n, k)


@pytest.mark.gpu
def test_range_guard_is_per_pair():
    """Split fp16, [A, 3e5 A, C]: only the middle pair leaves fp16's range and is repeated on the exact kernels (its bits are the exact-f32
    context's); its neighbours keep their split-arithmetic bits, and the next in-range batch on the same context is split arithmetic again."""
    m = _matcher(arithmetic="split_fp16")
    names = ["A", "A*", "C"]
    singles = [_single("A", arithmetic="split_fp16"), _single("A*", arithmetic="exact_f32"), _single("C", arithmetic="split_fp16")]
    out = m(_batch(names), with_ids=True)
    assert int(m.debug_read("ovf_trips", 1)[0]) == 1                              # pairs, not calls: one of the three was repeated
    _assert_batch_equals_singles(out, names, singles)
    mid = out["batch_indexes"].cpu() == 1
    assert int(mid.sum()) > 0 and bool(torch.isfinite(out["keypoints1"].cpu()[mid]).all()) and bool(torch.isfinite(out["confidence"].cpu()[mid]).all())
    # the two arithmetics are told apart by their bits (else the checks above and below say nothing about which one ran)
    assert not all(torch.equal(_single("A", arithmetic="split_fp16")[k], _single("A", arithmetic="exact_f32")[k]) for k in KEYS)
    names = ["C", "A", "A"]
    _assert_batch_equals_singles(m(_batch(names), with_ids=True), names, [_single(n, arithmetic="split_fp16") for n in names])
    assert int(m.debug_read("ovf_trips", 1)[0]) == 1                              # nothing was repeated this time


@pytest.mark.gpu
def test_coarse_only_batch():
    names = ["A", "C"]
    out = _matcher(fine=False)(_batch(names), with_ids=True)
    singles = [_single(n, fine=False) for n in names]
    _assert_batch_equals_singles(out, names, singles)
    assert torch.equal(singles[0]["keypoints1"] % 8, torch.zeros_like(singles[0]["keypoints1"]))      # (on the 1/8 grid: no fine level ran)


@pytest.mark.gpu
def test_c_abi_batch_entry_points():
    """gn_loftr_create + gn_loftr_match are the max_pairs = 1 / B = 1 calls of the batched code: the same bits as gn_loftr_match_batch(B = 1) on a
    max_pairs = 2 context; B outside 1 .. max_pairs is GN_ERR_ARG with a message; gn_loftr_cap is the mirror's `_cap`."""
    GN_ERR_ARG = -1                              # include/gisnav_amd.h
    m2 = _matcher()
    m2._ensure(128, 160, 2)
    lib, cap = m2.lib, m2._cap(128, 160)
    assert lib.gn_loftr_cap(m2._ctx) == cap == 320
    i0, i1 = (t.cuda().contiguous() for t in _pair("A"))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = lambda: (torch.zeros((cap, 2), device="cuda"), torch.zeros((cap, 2), device="cuda"), torch.zeros((cap,), device="cuda"),  # noqa: E731
                    torch.zeros((cap, 2), dtype=torch.int32, device="cuda"))
    ctx1 = C.c_void_p()
    assert lib.gn_loftr_create(0, 128, 160, cap, 1, C.byref(ctx1)) == 0
    try:
        assert lib.gn_loftr_cap(ctx1) == cap
        for name, arr in _sd().items():
            if name.endswith("num_batches_tracked") or name == "pos_encoding.pe":
                continue
            arr = np.ascontiguousarray(arr.detach().cpu().numpy() if hasattr(arr, "detach") else arr, dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*(arr.shape if arr.ndim else (1,)))
            assert lib.gn_loftr_load_tensor(ctx1, name.encode(), arr.ctypes.data_as(C.c_void_p), shape, max(arr.ndim, 1)) == 0, name
        a, n_a = bufs(), C.c_int32(-1)
        assert lib.gn_loftr_match(ctx1, p(i0), p(i1), p(a[0]), p(a[1]), p(a[2]), p(a[3]), C.byref(n_a), stream) == 0
        torch.cuda.synchronize()
    finally:
        lib.gn_loftr_destroy(ctx1)
    b, n_b, nd = bufs(), (C.c_int32 * 1)(-1), torch.zeros((1,), dtype=torch.int32, device="cuda")
    assert lib.gn_loftr_match_batch(m2._ctx, 1, p(i0), p(i1), p(b[0]), p(b[1]), p(b[2]), p(b[3]), p(nd), n_b, stream) == 0
    n = int(n_a.value)
    assert n == int(n_b[0]) == int(nd.cpu()[0]) == _single("A")["keypoints0"].shape[0] and n > 100
    for x, y in zip(a, b):
        assert torch.equal(x[:n].cpu(), y[:n].cpu())
    assert torch.equal(a[1][:n].cpu(), _single("A")["keypoints1"])
    for bad in (0, 3):
        assert lib.gn_loftr_match_batch(m2._ctx, bad, p(i0), p(i1), p(b[0]), p(b[1]), p(b[2]), p(b[3]), None, None, stream) == GN_ERR_ARG
        assert len(lib.gn_loftr_last_error(m2._ctx)) > 0


@pytest.mark.gpu
def test_batched_poses_equal_single_poses():
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.loftr import loftr_pose, loftr_pose_batch
    from gisnav_amd.synthetic import K_MATRIX
    h, w = 240, 320
    flat = torch.full((h, w), 0.5)
    pairs = [lf.synthetic_pair(7, h, w), (flat, flat), lf.synthetic_pair(8, h, w)]
    dem = (10 + 8 * np.sin(np.arange(h)[:, None] / 30.0) * np.cos(np.arange(w)[None, :] / 45.0)).astype(np.uint8)
    m = _matcher()
    eng = PoseEngine(0, max_batch=3, max_kpts=2048, precision="f32")
    f = torch.stack([p[0] for p in pairs]).cuda()
    t = torch.stack([p[1] for p in pairs]).cuda()
    for cov in (False, True):
        got = loftr_pose_batch(m, eng, f, t, [dem] * 3, K_MATRIX, return_covariance=cov)
        assert len(got) == 3
        m1 = _cache.setdefault("pose_single_matcher", _matcher())
        for b in range(3):
            want = loftr_pose(m1, eng, pairs[b][0].cuda(), pairs[b][1].cuda(), dem, K_MATRIX, return_covariance=cov)
            assert (want is None) == (got[b] is None), b
            if want is None:
                continue
            assert np.array_equal(got[b][0], want[0]) and np.array_equal(got[b][1], want[1]) and got[b][2] == want[2], b
            if cov:
                assert (want[3] is None) == (got[b][3] is None) and (want[3] is None or np.array_equal(got[b][3], want[3])), b
        assert got[1] is None and got[0] is not None and got[2] is not None


def test_mismatched_batches_are_refused_before_any_device_call():
    """No GPU needed: the mirror compares the shapes before it looks for a device (a matcher that was never moved to one gets this far)."""
    from gisnav_amd import _lib
    from gisnav_amd.loftr import LoFTR
    m = LoFTR(state_dict={"x": torch.zeros(1)})
    a = torch.zeros(3, 1, 64, 96)
    for other in (torch.zeros(2, 1, 64, 96), torch.zeros(3, 1, 64, 104), torch.zeros(3, 64, 104), torch.zeros(64, 96)):
        with pytest.raises(_lib.GnError, match="one batch size"):
            m({"image0": a, "image1": other})
    with pytest.raises(_lib.GnError, match="expected"):
        m({"image0": torch.zeros(3, 2, 64, 96), "image1": torch.zeros(3, 2, 64, 96)})
    assert LoFTR._batch_shape(a, torch.zeros(3, 64, 96)) == (3, 64, 96) and LoFTR._batch_shape(torch.zeros(64, 96), torch.zeros(1, 1, 64, 96)) == (1, 64, 96)
    assert m._ctx is None and m.lib is None

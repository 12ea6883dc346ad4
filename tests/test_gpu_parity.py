"""Parity tests proper (-m gpu): every check goes through the C ABI of libgisnav_amd.so and compares
with the oracle on the same seeded inputs, with the committed golden fixtures, or -- at BASELINE.json's
full size -- through size-independent properties.

Stated tolerances:
  * correspondence indices: bit-exact (f32 mode, and bf16-attention mode on the seeded fixtures);
  * match scores: |d| <= 1e-5;  residual stream per layer: max rel 2e-5 (f32), 3e-2 (bf16 attention);
  * EPnP minimal solver, per RANSAC hypothesis: ||dR||_F, ||dt|| <= 1e-8 (measured ~1e-12);
  * pose (R, t), planar (flat DEM) and non-planar scenes alike: RANSAC inlier COUNT identical,
    ||dR||_F <= 1e-8 and ||dt||/||t|| <= 1e-8 (measured 1e-13..1e-16: both sides run the LM refinement
    to the same fixed point).
"""
import os

import numpy as np
import pytest
import torch

from conftest import oracle_match
from gisnav_amd.synthetic import K_MATRIX, make_pair

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def eng256(state_dict_np, dev):
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=4, max_kpts=256, precision="f32", state_dict=state_dict_np)


@pytest.fixture(scope="module")
def eng256_bf16(state_dict_np, dev):
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=4, max_kpts=256, precision="bf16_attn", state_dict=state_dict_np)


@pytest.fixture(scope="module")
def eng256_x3(state_dict_np, dev):
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=4, max_kpts=256, precision="f32x3_bf16_attn", state_dict=state_dict_np)


@pytest.fixture(scope="module")
def eng256_h2(state_dict_np, dev):
    from gisnav_amd.engine import PoseEngine
    return PoseEngine(0, max_batch=4, max_kpts=256, precision="f16x2_bf16_attn", state_dict=state_dict_np)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------ kernels in isolation
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (256, 384, 512), (1024, 768, 256), (128, 512, 128)])
def test_gemm_f32_mfma_against_fp64(eng256, dev, M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(dev); W = torch.randn(N, K, generator=g).to(dev); b = torch.randn(N, generator=g).to(dev)
    Y = eng256.debug_gemm(A, W, b)
    ref = (A.double() @ W.double().T + b.double()).cpu().numpy()
    assert _rel(Y.cpu().numpy(), ref) < 2e-6
    assert _rel(eng256.debug_gemm(A, W, None).cpu().numpy(), ref - b.double().cpu().numpy()) < 2e-6


@pytest.mark.parametrize("planes", [0, 1])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (1024, 768, 256), (4096, 512, 512)])
def test_gemm_f32x3_split_is_f32_accurate(eng256_x3, eng256, dev, M, N, K, planes):
    """The 3 x bf16 split GEMM (6 partial products, f32 accumulate) must be at least as close to fp64 as the
    exact-f32 MFMA GEMM up to a factor 2, with weights split on the fly (planes=0) or pre-split (planes=1)."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(dev); W = (torch.randn(N, K, generator=g) * 0.05).to(dev); b = torch.randn(N, generator=g).to(dev)
    ref = (A.double() @ W.double().T + b.double()).cpu().numpy()
    e32 = _rel(eng256.debug_gemm(A, W, b).cpu().numpy(), ref)
    eng256_x3.lib.gn_debug_set_variant(eng256_x3.ctx, 2, planes)
    y = eng256_x3.debug_gemm(A, W, b)
    y2 = eng256_x3.debug_gemm(A, W, b)
    eng256_x3.lib.gn_debug_set_variant(eng256_x3.ctx, 2, 0)
    ex3 = _rel(y.cpu().numpy(), ref)
    assert ex3 < 2e-6 and ex3 < 2 * e32 + 1e-7, (ex3, e32)
    assert torch.equal(y, y2)                                  # bitwise repeatable


@pytest.mark.parametrize("planes,wstd,astd", [(0, 0.05, 1.0), (1, 0.05, 1.0), (14, 0.05, 1.0), (19, 1e-3, 1.0), (14, 0.05, 30.0), (1, 0.05, 1e-2)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (1024, 768, 256), (4096, 512, 512)])
def test_gemm_f16x2_split_is_f32_accurate(eng256_h2, eng256, dev, M, N, K, planes, wstd, astd):
    """The 2 x fp16 split GEMM (3 partial products, f32 accumulate) against fp64, next to the exact-f32 MFMA GEMM:
    weights split on the fly (planes=0), pre-split unscaled (1) or pre-split with a 2^(planes-1) scale as the
    library does at load time; small weights, large and small activations (fp16 subnormal pieces)."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=g) * astd).to(dev); W = (torch.randn(N, K, generator=g) * wstd).to(dev)
    b = (torch.randn(N, generator=g) * wstd * astd).to(dev)
    ref = (A.double() @ W.double().T + b.double()).cpu().numpy()
    e32 = _rel(eng256.debug_gemm(A, W, b).cpu().numpy(), ref)
    eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 2, planes)
    y = eng256_h2.debug_gemm(A, W, b)
    y2 = eng256_h2.debug_gemm(A, W, b)
    eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 2, 0)
    eh2 = _rel(y.cpu().numpy(), ref)
    # activations below ~2^-4 have fp16-SUBNORMAL residual terms (absolute resolution 2^-25): the split is then good to ~2e-6 of the
    # result, not to the f32 pipe's error (until round 2 this case silently ran whatever kernel family the last launch of ANOTHER
    # context had selected -- gn_debug_gemm now selects its own context's)
    assert eh2 < 2e-6 and (astd < 0.1 or eh2 < 2 * e32 + 1e-7), (eh2, e32)
    assert torch.equal(y, y2)                                  # bitwise repeatable


def test_gemm_layout_is_not_transposed(eng256, dev):
    A = torch.eye(128, device=dev)
    W = torch.arange(128 * 128, dtype=torch.float32, device=dev).reshape(128, 128)   # asymmetric
    assert torch.equal(eng256.debug_gemm(A, W, None), W.T.contiguous())


@pytest.mark.parametrize("prec", ["f32", "bf16_attn"])
@pytest.mark.parametrize("cross", [False, True])
def test_attention_against_fp64_with_ragged_keys(eng256, eng256_bf16, dev, prec, cross):
    eng = eng256 if prec == "f32" else eng256_bf16
    n, BS = 256, 4
    g = torch.Generator(device="cpu").manual_seed(3)
    q, k, v = (torch.randn(BS, n, 256, generator=g).to(dev) for _ in range(3))
    k[1, 7] *= 6.0                                     # one spiked key forces the online-softmax rescale path
    nkv = torch.tensor([256, 219, 5, 130], dtype=torch.int32, device=dev)
    out = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
    for bs in range(BS):
        kvs = bs ^ 1 if cross else bs
        m = int(nkv[kvs])
        qq = q[bs].double().cpu().reshape(n, 4, 64).transpose(0, 1) * 0.125
        kk = k[kvs, :m].double().cpu().reshape(m, 4, 64).transpose(0, 1)
        vv = v[kvs, :m].double().cpu().reshape(m, 4, 64).transpose(0, 1)
        o = (torch.softmax(qq @ kk.transpose(1, 2), -1) @ vv).transpose(0, 1).reshape(n, 256).numpy()
        assert _rel(out[bs], o) < (3e-6 if prec == "f32" else 2e-2), (bs, prec, cross)


@pytest.mark.gpu
@pytest.mark.parametrize("boost", [1.0, 40.0, 400.0])
def test_attention_optimistic_reference_falls_back_exactly(eng256_bf16, dev, boost):
    """k_attn_bf16_v5 searches the softmax reference in the first two key tiles only; a workgroup whose denominators leave the safe
    range repeats its tiles with the exact running maximum.  Keys beyond the searched tiles are boosted so that their scores exceed
    the reference by tens (still in range) or by thousands (overflow -> fallback): the result must match fp64 either way, and must
    equal the always-exact developer variant (knob 1 = 56) to bf16 rounding."""
    n, BS = 256, 2
    g = torch.Generator(device="cpu").manual_seed(11)
    q, k, v = (torch.randn(BS, n, 256, generator=g).to(dev) for _ in range(3))
    k[:, 160:] *= boost                                  # scores of the late keys: ~ +-8 * boost * 0.125
    nkv = torch.tensor([256, 231], dtype=torch.int32, device=dev)
    out = eng256_bf16.debug_attention(q, k, v, nkv, False, 0.125).cpu().numpy()
    eng256_bf16.lib.gn_debug_set_variant(eng256_bf16.ctx, 1, 56)
    try:
        exact = eng256_bf16.debug_attention(q, k, v, nkv, False, 0.125).cpu().numpy()
    finally:
        eng256_bf16.lib.gn_debug_set_variant(eng256_bf16.ctx, 1, 4)
    assert np.isfinite(out).all()
    for bs in range(BS):
        m = int(nkv[bs])
        # the reference sees the operands as the kernel does (bf16 q * scale, k, v): with logits this large the softmax is nearly
        # one-hot and the rounding of the INPUTS would otherwise decide which key wins
        qq = (q[bs] * 0.125).bfloat16().double().cpu().reshape(n, 4, 64).transpose(0, 1)
        kk = k[bs, :m].bfloat16().double().cpu().reshape(m, 4, 64).transpose(0, 1)
        vv = v[bs, :m].bfloat16().double().cpu().reshape(m, 4, 64).transpose(0, 1)
        o = (torch.softmax(qq @ kk.transpose(1, 2), -1) @ vv).transpose(0, 1).reshape(n, 256).numpy()
        assert _rel(out[bs], o) < 2e-2, (bs, boost)
        assert _rel(exact[bs], o) < 2e-2, (bs, boost)
        assert _rel(out[bs], exact[bs]) < 1e-2, (bs, boost)


@pytest.mark.gpu
@pytest.mark.parametrize("cross", [False, True])
def test_attention_key_splits_equal_the_single_workgroup_result(eng256_bf16, dev, cross):
    """Opt-in (developer knob 23 = largest split; off by default because it makes results depend on the grid): small grids split the keys
    of every (slot, head, query block) over up to four workgroups that merge through a ticket.  Ragged key counts, incl. splits that receive no key at all: the merged rows equal the unsplit kernel's
    to bf16 rounding noise of the probabilities, and both match fp64 on the bf16-rounded operands."""
    n, BS = 256, 4
    g = torch.Generator(device="cpu").manual_seed(5)
    q, k, v = (torch.randn(BS, n, 256, generator=g).to(dev) for _ in range(3))
    nkv = torch.tensor([256, 70, 5, 129], dtype=torch.int32, device=dev)
    outs = {}
    try:
        for split in (1, 2, 4):
            eng256_bf16.lib.gn_debug_set_variant(eng256_bf16.ctx, 23, split)
            outs[split] = eng256_bf16.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
    finally:
        eng256_bf16.lib.gn_debug_set_variant(eng256_bf16.ctx, 23, 1)
    for bs in range(BS):
        kvs = bs ^ 1 if cross else bs
        m = int(nkv[kvs])
        qq = (q[bs] * 0.125).bfloat16().double().cpu().reshape(n, 4, 64).transpose(0, 1)
        kk = k[kvs, :m].bfloat16().double().cpu().reshape(m, 4, 64).transpose(0, 1)
        vv = v[kvs, :m].bfloat16().double().cpu().reshape(m, 4, 64).transpose(0, 1)
        o = (torch.softmax(qq @ kk.transpose(1, 2), -1) @ vv).transpose(0, 1).reshape(n, 256).numpy()
        for split in (1, 2, 4):
            assert _rel(outs[split][bs], o) < 1e-2, (bs, split, cross)
        # (each split rounds its probabilities to bf16 relative to its OWN reference: the merged rows differ from the unsplit ones by bf16 noise)
        assert _rel(outs[2][bs], outs[1][bs]) < 6e-3 and _rel(outs[4][bs], outs[1][bs]) < 6e-3, (bs, cross)


# ------------------------------------------------------------------ matcher vs oracle, stage by stage
def test_matcher_matches_oracle_per_layer_and_bit_exact_indices(eng256, state_dict_t):
    pairs = [make_pair(40 + i, n_q=256 - 13 * i, n_r=256 - 5 * i) for i in range(3)]
    inp = eng256.stage_inputs(pairs)
    taps = []
    for p in pairs:
        t = {}
        t["res"] = oracle_match(state_dict_t, p, taps=t)
        taps.append(t)
    T, npad = 4 * 2 * 256, 256
    for nl in (1, 3, 9):
        eng256.set_num_layers(nl)
        idx, score, n_match = eng256.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        torch.cuda.synchronize()
        x = eng256.debug_read("x", T * 256).reshape(4, 2, npad, 256)
        for b, p in enumerate(pairs):
            nq, nr = len(p.kp_q), len(p.kp_r)
            assert _rel(x[b, 0, :nq], taps[b][f"layer{nl - 1}_0"][0].numpy()) < 2e-5
            assert _rel(x[b, 1, :nr], taps[b][f"layer{nl - 1}_1"][0].numpy()) < 2e-5
    desc = eng256.debug_read("desc", T * 128).reshape(4, 2, npad, 128)
    cos = eng256.debug_read("cos", T * 32).reshape(4, 2, npad, 32)
    # the fused match head never writes the similarity matrix: the unfused developer path (knob 16 = 0: sim GEMM + five passes) does,
    # and both heads must return the same matches
    fused = (idx.clone(), score.clone(), n_match.clone())
    stats_f = {k: eng256.debug_read(k, 4 * npad) for k in ("rowmax", "rowlog", "colmax", "collog")}
    eng256.lib.gn_debug_set_variant(eng256.ctx, 16, 0)
    idx, score, n_match = eng256.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    eng256.lib.gn_debug_set_variant(eng256.ctx, 16, 1)
    sim = eng256.debug_read("sim", 4 * npad * npad).reshape(4, npad, npad)
    assert torch.equal(fused[2], n_match)
    for b, p in enumerate(pairs):
        k = int(n_match[b]); nq, nr = len(p.kp_q), len(p.kp_r)
        assert torch.equal(fused[0][b, :k], idx[b, :k])
        assert (fused[1][b, :k] - score[b, :k]).abs().max().item() < 1e-5
        for name, n in (("rowmax", nq), ("rowlog", nq), ("colmax", nr), ("collog", nr)):
            u = eng256.debug_read(name, 4 * npad).reshape(4, npad)[b, :n]
            assert np.abs(u - stats_f[name].reshape(4, npad)[b, :n]).max() < 1e-4, name   # different summation orders of the 256 products
    from oracle import lightglue_sift as lg
    for b, p in enumerate(pairs):
        nq, nr = len(p.kp_q), len(p.kp_r)
        mq, mr, sc, oidx = taps[b]["res"]
        assert _rel(desc[b, 0, :nq], lg.rootsift(torch.from_numpy(p.desc_q)).numpy()) < 1e-6
        assert np.abs(cos[b, 1, :nr] - taps[b]["enc1"][0, 0, 0, :, ::2].numpy()).max() < 2e-5
        assert _rel(sim[b, :nq, :nr], taps[b]["sim"][0].numpy()) < 2e-5
        k = int(n_match[b])
        assert k == len(oidx) >= 15
        assert np.array_equal(idx[b, :k].cpu().numpy(), oidx.numpy())          # bit-exact correspondences
        assert np.abs(score[b, :k].cpu().numpy() - sc.numpy()[:, 0]).max() < 1e-5
        assert idx.dtype == torch.int64


@pytest.mark.parametrize("prec", ["f32", "bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn"])
@pytest.mark.parametrize("name", ["lightglue_seed0_q96_r80", "lightglue_seed0_q200_r256"])
def test_golden_fixtures_through_c_abi(eng256, eng256_bf16, eng256_x3, eng256_h2, dev, prec, name):
    eng = {"f32": eng256, "bf16_attn": eng256_bf16, "f32x3_bf16_attn": eng256_x3, "f16x2_bf16_attn": eng256_h2}[prec]
    eng.set_num_layers(9)
    g = np.load(os.path.join(GOLD, name + ".npz"))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kq = np.column_stack([g["kp_q"], g["size_q"], g["angle_q"]]).astype(np.float32)[None]
    kr = np.column_stack([g["kp_r"], g["size_r"], g["angle_r"]]).astype(np.float32)[None]
    inp = dict(desc_q=f(g["desc_q"][None]), kpt_q=f(kq), n_q=f(np.array([len(g["kp_q"])], np.int32)),
               desc_r=f(g["desc_r"][None]), kpt_r=f(kr), n_r=f(np.array([len(g["kp_r"])], np.int32)),
               dem=f(g["dem"][None]), kpt_format=1)
    idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    k = int(n_match[0])
    assert np.array_equal(idx[0, :k].cpu().numpy(), g["idx"])
    assert np.abs(score[0, :k].cpu().numpy() - g["scores"][:, 0]).max() < (1e-5 if prec == "f32" else 5e-3)
    out = eng.estimate(inp, g["K"])
    assert int(out["ok"][0]) == 1 and int(out["n_match"][0]) == len(g["idx"])
    R, t = out["R"][0].cpu().numpy(), out["t"][0].cpu().numpy()
    assert np.linalg.norm(R - g["R"]) < 1e-8 and np.linalg.norm(t - g["t"]) / np.linalg.norm(g["t"]) < 1e-8
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, n_match, inp["dem"])
    assert np.array_equal(mkp[0, :k].cpu().numpy(), g["mkp_q"])
    x, y = np.floor(g["mkp_r"]).astype(int).T
    assert np.array_equal(obj[0, :k].cpu().numpy(), np.hstack((g["mkp_r"], g["dem"][y, x].reshape(-1, 1))).astype(np.float32))


def test_identity_weights_recover_known_permutation(dev):
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.weights import synthetic_state_dict
    eng = PoseEngine(0, max_batch=1, max_kpts=128, state_dict=synthetic_state_dict(3, identity_blocks=True))
    rng = np.random.default_rng(5)
    n = 96
    p = make_pair(11, n_q=n, n_r=n)
    perm = rng.permutation(n)
    p.desc_q = np.clip(np.rint(p.desc_r[perm] + rng.normal(0, 2.0, (n, 128))), 0, 255).astype(np.float32)
    inp = eng.stage_inputs([p])
    idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    assert int(n_match[0]) == n
    assert idx[0, :n, 0].cpu().tolist() == list(range(n)) and idx[0, :n, 1].cpu().tolist() == perm.tolist()


@pytest.mark.parametrize("prec", ["f32", "f16x2_bf16_attn"])
def test_edge_cases_empty_ragged_and_tiny_inputs(eng256, eng256_h2, state_dict_t, dev, prec):
    eng = eng256 if prec == "f32" else eng256_h2
    eng.set_num_layers(9)
    pairs = [make_pair(60, n_q=256, n_r=256), make_pair(61, n_q=1, n_r=200), make_pair(62, n_q=40, n_r=2), make_pair(63, n_q=129, n_r=128)]
    inp = eng.stage_inputs(pairs)
    inp["n_q"][1] = 0                                   # an empty query cloud
    idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    nm = n_match.cpu().numpy()
    assert nm[1] == 0 and nm[0] > 15 and nm[3] > 15    # < 2 descriptors on a side -> no match (kornia _no_match)
    assert 0 <= nm[2] <= 2
    out = eng.estimate(inp, K_MATRIX)
    ok = out["ok"].cpu().numpy()
    assert ok[0] == 1 and ok[1] == 0 and ok[2] == 0 and ok[3] == 1          # MIN_MATCHES = 15 gate
    assert torch.isfinite(out["R"]).all() and torch.isfinite(out["t"]).all()
    # the other pairs in the batch are unaffected by their neighbours
    solo = eng.stage_inputs([pairs[3]])
    i2, s2, n2 = eng.match(solo["desc_q"], solo["kpt_q"], solo["n_q"], solo["desc_r"], solo["kpt_r"], solo["n_r"])
    assert int(n2[0]) == nm[3] and torch.equal(i2[0, : nm[3]], idx[3, : nm[3]])
    # and the ragged pairs agree with the oracle index for index
    for b in (0, 3):
        _, _, _, oidx = oracle_match(state_dict_t, pairs[b])
        assert nm[b] == len(oidx) and np.array_equal(idx[b, : nm[b]].cpu().numpy(), oidx.numpy())


def test_c_abi_rejects_bad_arguments(eng256, dev):
    from gisnav_amd import _lib
    from gisnav_amd.engine import PoseEngine
    pairs = [make_pair(70 + i, n_q=64, n_r=64) for i in range(5)]
    inp = eng256.stage_inputs(pairs)                     # B = 5 > max_batch = 4
    with pytest.raises(_lib.GnError):
        eng256.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    big = eng256.stage_inputs([make_pair(71, n_q=300, n_r=64)])   # stride 300 > max_kpts 256
    with pytest.raises(_lib.GnError):
        eng256.match(big["desc_q"], big["kpt_q"], big["n_q"], big["desc_r"], big["kpt_r"], big["n_r"])
    e = PoseEngine(0, max_batch=1, max_kpts=128)         # no weights loaded
    one = e.stage_inputs([make_pair(72, n_q=64, n_r=64)])
    with pytest.raises(_lib.GnError):
        e.match(one["desc_q"], one["kpt_q"], one["n_q"], one["desc_r"], one["kpt_r"], one["n_r"])
    with pytest.raises(_lib.GnError):
        e.load_state_dict({"input_proj.weight": np.zeros((256, 64), np.float32)})


def test_retired_developer_knob_values_are_refused(eng256_h2, state_dict_t, dev):
    """Knob values of retired timing ablations and rejected experiments return an error instead of timing the default kernel under
    their label; the context still matches the oracle afterwards."""
    from gisnav_amd.loftr import LoFTR
    from oracle import loftr as olf
    for which, value in ((1, 41), (1, 48), (1, 1000), (0, 51), (8, 2), (12, 1), (18, 1),
                         (24, 0), (24, 1), (24, 2), (36, 0), (36, 1), (34, 1)):      # SuperPoint's superseded convolution and simple_nms forms
        assert eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, which, value) != 0, (which, value)
    # knob 42 belongs to LoFTR contexts (gn_loftr_debug_set_variant): bits 0-7 are retired, bits 8 and up -- the overhead term of the cost model of
    # LoFTR's convolutions -- live on; a matcher context, which it never reached, refuses it altogether
    m = LoFTR(state_dict=olf.synthetic_state_dict(0)).to("cuda:0").eval()
    m._ensure(32, 32)                                    # (the smallest image LoFTR's tests use; the knob belongs to this context alone)
    for value in (1, 2, 4, 8, 16, 15):
        assert m.lib.gn_loftr_debug_set_variant(m._ctx, 42, value) != 0, (42, value)
    assert m.lib.gn_loftr_debug_set_variant(m._ctx, 42, 50 << 8) == 0
    assert eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 42, 50 << 8) != 0
    del m
    try:     # knob 34 keeps the round-2 kernels on f32 activations (0, also the path of frames beyond 8 Mpixel) and the shipped form (2)
        assert eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 34, 0) == 0
        assert eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 34, 2) == 0
    finally:
        eng256_h2.lib.gn_debug_set_variant(eng256_h2.ctx, 34, 2)
    p = make_pair(63, n_q=129, n_r=128)
    inp = eng256_h2.stage_inputs([p])
    idx, score, n_match = eng256_h2.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    _, _, _, oidx = oracle_match(state_dict_t, p)
    k = int(n_match[0])
    assert k == len(oidx) and np.array_equal(idx[0, :k].cpu().numpy(), oidx.numpy())


# ------------------------------------------------------------------ the three seams
def test_seam_b1_lightglue_matcher_drop_in(state_dict_np, state_dict_t, dev):
    from gisnav_amd.matcher import LightGlueMatcher
    from oracle import lightglue_sift as lg
    m = LightGlueMatcher("sift", params={"n_layers": 9, "filter_threshold": 0.5, "depth_confidence": -1, "width_confidence": -1},
                         state_dict=state_dict_np, max_kpts=256).to(dev).eval()
    p = make_pair(80, n_q=230, n_r=256)
    tq = torch.from_numpy
    with torch.inference_mode():   # the calls of pose_node.py:246-287
        laf_q = lg.laf_from_center_scale_ori(tq(p.kp_q)[None], tq(p.size_q)[None, :, None, None], tq(p.angle_q)[None, :, None])
        laf_r = lg.laf_from_center_scale_ori(tq(p.kp_r)[None], tq(p.size_r)[None, :, None, None], tq(p.angle_r)[None, :, None])
        dq, dr = lg.rootsift(tq(p.desc_q)), lg.rootsift(tq(p.desc_r))
        dists, idx = m(dq.to(dev), dr.to(dev), laf_q.to(dev), laf_r.to(dev))
        osc, oidx = lg.lightglue_matcher_forward(state_dict_t, dq, dr, laf_q, laf_r)
    assert dists.shape == (len(oidx), 1) and idx.shape == (len(oidx), 2) and idx.dtype == torch.int64 and idx.device.type == "cuda"
    assert torch.equal(idx.cpu(), oidx) and (dists.cpu() - osc).abs().max() < 1e-5
    kp = tq(p.kp_q).to(dev)
    assert kp[idx[:, 0]].shape == (len(oidx), 2)          # usable as an index, pose_node.py:296
    e_d, e_i = m(dq[:1].to(dev), dr.to(dev), laf_q[:, :1].to(dev), laf_r.to(dev))
    assert e_d.shape == (0, 1) and e_i.shape == (0, 2)


@pytest.mark.parametrize("name", ["pnp_outliers_dem", "pnp_outliers_flat"])
def test_seam_b2_compute_pose_on_golden_fixture(name, dev):
    from gisnav_amd.pose import compute_pose
    from gisnav_amd.wire import CameraInfo
    g = np.load(os.path.join(GOLD, name + ".npz"))
    out = compute_pose(CameraInfo(k=g["K"].reshape(-1)), g["img"], g["mkp_r"], g["dem"])
    assert out is not None
    R, t = out
    assert R.shape == (3, 3) and t.shape == (3, 1) and R.dtype == np.float64 and t.dtype == np.float64
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.linalg.norm(R - g["R_gt"]) < 3e-3 and np.linalg.norm(t - g["t_gt"]) / np.linalg.norm(g["t_gt"]) < 3e-3
    assert np.linalg.norm(R - g["R"]) < 1e-8 and np.linalg.norm(t - g["tvec"]) / np.linalg.norm(g["tvec"]) < 1e-8
    assert compute_pose(CameraInfo(k=g["K"].reshape(-1)), g["img"][:3], g["mkp_r"][:3], g["dem"]) is None


def test_epnp_minimal_solver_per_hypothesis(dev, eng256):
    import ctypes as C
    from oracle import pnp_ransac as pr
    p = make_pair(20)
    q = np.nonzero(p.gt_q2r >= 0)[0]
    mq, mr = p.kp_q[q], p.kp_r[p.gt_q2r[q]]
    x, y = np.floor(mr).astype(int).T
    obj = np.hstack((mr, p.dem[y, x].reshape(-1, 1))).astype(np.float32).astype(np.float64)
    und = np.column_stack([(mq[:, 0].astype(np.float64) - K_MATRIX[0, 2]) / K_MATRIX[0, 0],
                           (mq[:, 1].astype(np.float64) - K_MATRIX[1, 2]) / K_MATRIX[1, 1]])
    rng = pr.CvRNG()
    subsets = [pr.get_subset(rng, len(obj), 5) for _ in range(10)]      # the subsets solvePnPRansac would draw
    pws = np.stack([obj[s] for s in subsets]); us = np.stack([und[s] for s in subsets])
    tp, tu = torch.from_numpy(pws).to(dev), torch.from_numpy(us).to(dev)
    out = torch.zeros((10, 64), dtype=torch.float64, device=dev)
    rc = eng256.lib.gn_debug_epnp(eng256.ctx, 10, C.c_void_p(tp.data_ptr()), C.c_void_p(tu.data_ptr()),
                                  C.c_void_p(out.data_ptr()), eng256._stream())
    assert rc == 0
    o = out.cpu().numpy()
    for k in range(10):
        R, t = pr.epnp(pws[k], us[k])
        assert np.linalg.norm(o[k, :9].reshape(3, 3) - R) < 1e-8 and np.linalg.norm(o[k, 9:12] - t) < 1e-8, k
        assert abs(o[k, 27]) < 1e-12 and abs(o[k, 28]) < 1e-12 and o[k, 29] > 1e-4   # exactly 2-D null space of M^T M


def test_pnp_inlier_count_and_pose_against_oracle(dev, eng256):
    from oracle import pnp_ransac as pr
    for seed in range(90, 102):
        flat = seed % 4 == 0
        p = make_pair(seed, n_q=256, n_r=256, flat_dem=flat)
        q = np.nonzero(p.gt_q2r >= 0)[0]
        mq, mr = p.kp_q[q].copy(), p.kp_r[p.gt_q2r[q]]
        rs = np.random.default_rng(seed)
        no = len(q) // 6
        mq[:no] = np.column_stack([rs.uniform(0, 640, no), rs.uniform(0, 480, no)]).astype(np.float32)   # gross outliers
        x, y = np.floor(mr).astype(int).T
        obj = np.hstack((mr, p.dem[y, x].reshape(-1, 1))).astype(np.float32)
        ok, r, t, inl = pr.solve_pnp_ransac(obj, mq, K_MATRIX, 10)
        R, tg, ninl, okg = eng256.pnp_ransac(torch.from_numpy(obj[None]).to(dev), torch.from_numpy(mq[None]).to(dev),
                                             torch.tensor([len(obj)], dtype=torch.int32, device=dev), K_MATRIX)
        assert ok and int(okg[0]) == 1
        dR = np.linalg.norm(R[0].cpu().numpy() - pr.rodrigues_vec2mat(r))
        dt = np.linalg.norm(tg[0].cpu().numpy() - t) / np.linalg.norm(t)
        assert np.linalg.norm(R[0].cpu().numpy() - p.R_gt) < 5e-3
        assert int(ninl[0]) == len(inl), (seed, flat, int(ninl[0]), len(inl))
        assert dR < 1e-8 and dt < 1e-8, (seed, flat, dR, dt)


def test_seam_b3_pose_node_shim_from_wire_bytes(state_dict_np, state_dict_t, dev):
    from gisnav_amd import wire
    from gisnav_amd.pose_node import PoseNode
    from oracle import pnp_ransac as pr
    p = make_pair(85, n_q=256, n_r=256)
    calls = []

    def extractor(ref_u8):   # stands in for cv2.SIFT_create().detectAndCompute(ref, None) (pose_node.py:230)
        calls.append(ref_u8.shape)
        return p.kp_r, p.desc_r, p.size_r, p.angle_r

    node = PoseNode(state_dict_np, extractor, max_kpts=256)
    assert node.pose() is None                                       # narrow_types: inputs not yet received
    node.camera_info = wire.CameraInfo(k=K_MATRIX.reshape(-1), height=480, width=640)
    msg = wire.OrthoStereoImage(query_sift=wire.pack_keypoints(p.kp_q, p.size_q, p.angle_q, p.desc_q),
                                reference=wire.ImageMsg(p.ref, wire.Stamp(12, 5)), dem=wire.ImageMsg(p.dem, wire.Stamp(12, 5)))
    node.pose_image = msg
    r1 = node.pose()
    r2 = node.pose()                                                  # same tile stamp -> cached reference features
    assert len(calls) == 1 and r1 is not None
    mq, mr, sc, oidx = oracle_match(state_dict_t, p)
    assert node.last_num_matches == len(oidx)
    Ro, to = pr.compute_pose(K_MATRIX.reshape(-1), mq.numpy(), mr.numpy(), p.dem)
    assert np.linalg.norm(r1[0] - Ro) < 1e-8 and np.linalg.norm(r1[1] - to) / np.linalg.norm(to) < 1e-8
    assert np.array_equal(r1[0], r2[0])
    node.pose_image = wire.OrthoStereoImage(query_sift=wire.pack_keypoints(p.kp_q[:10], p.size_q[:10], p.angle_q[:10], p.desc_q[:10]),
                                            reference=wire.ImageMsg(p.ref, wire.Stamp(13, 0)), dem=wire.ImageMsg(p.dem, wire.Stamp(13, 0)))
    assert node.pose() is None and len(calls) == 2                   # < MIN_MATCHES -> None; new stamp -> re-extract


# ------------------------------------------------------------------ BASELINE.json full size: properties
@pytest.fixture(scope="module")
def full_size(state_dict_np, dev):
    from gisnav_amd.engine import PoseEngine
    pairs = [make_pair(i) for i in range(32)]
    res = {}
    T = 32 * 2 * 1024
    for prec in ("f32", "bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn", "f16x2_f16_attn"):
        eng = PoseEngine(0, max_batch=32, max_kpts=1024, precision=prec, state_dict=state_dict_np)
        inp = eng.stage_inputs(pairs)
        idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        torch.cuda.synchronize()
        x_first = eng.debug_read("x", T * 256).copy()            # very first (cold) run of this context
        out = eng.estimate(inp, K_MATRIX)
        torch.cuda.synchronize()
        x_again = eng.debug_read("x", T * 256).copy()
        res[prec] = (idx.cpu().numpy(), score.cpu().numpy(), n_match.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()})
        res[prec + ":x"] = (x_first, x_again)
        if prec == "f32":   # permutation equivariance: shuffle the query keypoints of every pair
            rng = np.random.default_rng(0)
            perms = [rng.permutation(1024) for _ in pairs]
            shuffled = []
            for p, pm in zip(pairs, perms):
                q = make_pair(0)
                q.__dict__.update(p.__dict__)
                q.kp_q, q.desc_q, q.size_q, q.angle_q = p.kp_q[pm], p.desc_q[pm], p.size_q[pm], p.angle_q[pm]
                shuffled.append(q)
            inp2 = eng.stage_inputs(shuffled)
            i2, s2, n2 = eng.match(inp2["desc_q"], inp2["kpt_q"], inp2["n_q"], inp2["desc_r"], inp2["kpt_r"], inp2["n_r"])
            res["perm"] = (perms, i2.cpu().numpy(), n2.cpu().numpy())
        del eng
    return pairs, res


def test_full_size_matches_are_mutual_sorted_and_correct(full_size):
    pairs, res = full_size
    idx, score, nm, out = res["f32"]
    for b, p in enumerate(pairs):
        k = nm[b]
        ii = idx[b, :k]
        assert k >= 300
        assert (np.diff(ii[:, 0]) > 0).all()                          # ascending query index
        assert len(np.unique(ii[:, 1])) == k                          # one-to-one (mutual nearest neighbours)
        assert (score[b, :k] > 0.5).all() and (score[b, :k] <= 1.0 + 1e-6).all()
        gt = p.gt_q2r[ii[:, 0]]
        assert (gt == ii[:, 1]).mean() > 0.99                         # they are the true correspondences
        assert k >= 0.97 * (p.gt_q2r >= 0).sum()


def test_full_size_pose_close_to_ground_truth(full_size):
    pairs, res = full_size
    for prec in ("f32", "bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn", "f16x2_f16_attn"):
        out = res[prec][3]
        assert out["ok"].all()
        for b, p in enumerate(pairs):
            assert np.linalg.norm(out["R"][b] - p.R_gt) < 5e-3
            assert np.linalg.norm(out["t"][b] - p.t_gt) / np.linalg.norm(p.t_gt) < 5e-3
            assert abs(np.linalg.det(out["R"][b]) - 1) < 1e-12
            assert out["n_inliers"][b] >= 0.9 * out["n_match"][b]


@pytest.mark.parametrize("prec", ["bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn", "f16x2_f16_attn"])
def test_full_size_reduced_modes_give_the_same_correspondences(full_size, prec):
    _, res = full_size
    i0, s0, n0, _ = res["f32"]
    i1, s1, n1, _ = res[prec]
    assert np.array_equal(n0, n1)
    for b in range(len(n0)):
        assert np.array_equal(i0[b, : n0[b]], i1[b, : n1[b]])
        assert np.abs(s0[b, : n0[b]] - s1[b, : n0[b]]).max() < 5e-3


@pytest.mark.parametrize("prec", ["f32", "bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn", "f16x2_f16_attn"])
def test_full_size_bitwise_repeatable_including_first_run(full_size, prec):
    """Regression guard for a timing-dependent miscompile (SLP-packed v_pk_*_f32 in a GEMM epilogue): the residual
    stream after 9 layers must be bit-identical between the cold first run of a context and a later run."""
    _, res = full_size
    x_first, x_again = res[prec + ":x"]
    assert np.array_equal(x_first.view(np.int32), x_again.view(np.int32))


@pytest.mark.parametrize("prec", ["bf16_attn", "f16x2_bf16_attn", "f16x2_f16_attn"])
def test_full_size_bitwise_repeatable_over_many_runs(state_dict_np, dev, prec):
    """Sixty bench-sized forwards of one context: the residual stream after 9 layers and the matches are bit-identical every time.
    Two runs are not enough: the ring race this guards against (an LDS-DMA refill overtaking a fragment read that was issued just in
    front of the workgroup barrier; k_attn_bf16_v5 now waits lgkmcnt(0) there) changed one pair in ~5 % of the calls."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=32, max_kpts=1024, precision=prec, state_dict=state_dict_np)
    inp = eng.stage_inputs([make_pair(i, n_q=1024 - (i % 5) * 17, n_r=1024 - (i % 3) * 29) for i in range(32)])
    args = (inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    T = 32 * 2 * 1024
    ref = None
    for run in range(60):
        idx, score, n = eng.match(*args)
        torch.cuda.synchronize()
        nn = n.cpu().numpy().copy()
        valid = np.arange(1024)[None, :] < nn[:, None]                    # the lists are filled up to n_match only
        cur = (eng.debug_read("x", T * 256).view(np.uint32).copy(), np.where(valid[:, :, None], idx.cpu().numpy(), 0),
               np.where(valid, score.cpu().numpy().view(np.uint32), 0), nn)
        if ref is None:
            ref = cur
            continue
        for a_, b_ in zip(ref, cur):
            assert np.array_equal(a_, b_), (prec, run, int((a_ != b_).sum()))


def test_full_size_permutation_equivariance(full_size):
    _, res = full_size
    idx, _, nm, _ = res["f32"]
    perms, i2, n2 = res["perm"]
    for b, pm in enumerate(perms):
        assert n2[b] == nm[b]
        a = {(int(q), int(r)) for q, r in idx[b, : nm[b]]}
        c = {(int(pm[q]), int(r)) for q, r in i2[b, : n2[b]]}        # shuffled index q holds original keypoint pm[q]
        assert a == c


def test_full_size_oracle_spot_check(full_size, state_dict_t):
    from oracle import pnp_ransac as pr
    pairs, res = full_size
    idx, score, nm, out = res["f32"]
    for b in (0, 12, 17, 25):
        mq, mr, sc, oidx = oracle_match(state_dict_t, pairs[b])
        assert np.array_equal(idx[b, : nm[b]], oidx.numpy())
        assert np.abs(score[b, : nm[b]] - sc.numpy()[:, 0]).max() < 1e-5
        Ro, to = pr.compute_pose(K_MATRIX.reshape(-1), mq.numpy(), mr.numpy(), pairs[b].dem)
        for prec in ("f32", "bf16_attn", "f32x3_bf16_attn", "f16x2_bf16_attn"):      # identical correspondences -> identical pose problem
            o = res[prec][3]
            assert np.linalg.norm(o["R"][b] - Ro) < 1e-8 and np.linalg.norm(o["t"][b] - to) / np.linalg.norm(to) < 1e-8


@pytest.mark.gpu
def test_overlapped_pose_stage_gives_identical_results(state_dict_np, dev):
    """gn_set_overlap: PnP of call n on the internal stream beside the matcher of call n+1 -- back-to-back calls on
    DIFFERENT batches must return exactly what the in-order path returns (double-buffered PnP inputs)."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=4, max_kpts=256, precision="f16x2_bf16_attn", state_dict=state_dict_np)
    batches = [eng.stage_inputs([make_pair(40 + 4 * s + i, n_q=256, n_r=256) for i in range(4)]) for s in range(5)]
    serial = []
    for inp in batches:
        o = eng.estimate(inp, K_MATRIX)
        torch.cuda.synchronize()
        serial.append({k: v.cpu().numpy().copy() for k, v in o.items()})
    eng.set_overlap(True)
    outs = [eng.alloc_outputs(4) for _ in batches]
    for inp, o in zip(batches, outs):                   # no host sync in between
        eng.estimate(inp, K_MATRIX, out=o)
    eng.flush()
    torch.cuda.current_stream().synchronize()           # the caller's stream alone must now see every result
    for s, o in zip(serial, outs):
        for k in s:
            assert np.array_equal(s[k], o[k].cpu().numpy()), k
    eng.set_overlap(False)
    o = eng.estimate(batches[0], K_MATRIX)
    torch.cuda.synchronize()
    assert all(np.array_equal(serial[0][k], o[k].cpu().numpy()) for k in serial[0])


@pytest.mark.gpu
def test_substreams_give_identical_results(state_dict_np, dev):
    """gn_set_substreams: the pairs of a call run as out-of-phase groups on internal streams over views of the
    workspaces -- every output must equal the single-stream result, also for uneven group sizes."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=5, max_kpts=256, precision="f16x2_bf16_attn", state_dict=state_dict_np)
    inp = eng.stage_inputs([make_pair(80 + i, n_q=256 - 7 * i, n_r=256 - 3 * i) for i in range(5)])
    ref = {k: v.cpu().numpy().copy() for k, v in eng.estimate(inp, K_MATRIX).items()}
    for n in (2, 3, 5):
        eng.set_substreams(n)
        outs = [eng.estimate(inp, K_MATRIX, out=eng.alloc_outputs(5)) for _ in range(3)]    # back-to-back, joined once
        eng.flush()
        torch.cuda.current_stream().synchronize()
        for o in outs:
            assert all(np.array_equal(ref[k], o[k].cpu().numpy()) for k in ref), n
    eng.set_substreams(1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x2_bf16_attn"])
def test_active_kpts_padding_does_not_change_results(state_dict_np, dev, prec):
    """gn_set_active_kpts: running a batch at a smaller padded size (640 -> 256 slots per image; attention cost / 6) gives
    exactly the outputs of the full-size run -- padding is masked out exactly -- also with sub-batch streams."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=4, max_kpts=640, precision=prec, state_dict=state_dict_np)
    inp = eng.stage_inputs([make_pair(90 + i, n_q=250 - 9 * i, n_r=256 - 5 * i) for i in range(4)])
    ref = {k: v.cpu().numpy().copy() for k, v in eng.estimate(inp, K_MATRIX).items()}
    ridx, rscore, rn = (v.cpu().numpy().copy() for v in eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"]))
    assert (ref["n_match"] > 30).all() and ref["ok"].all()
    assert eng.set_active_kpts(250) == 256 and eng.kmax == 640
    out = {k: v.cpu().numpy() for k, v in eng.estimate(inp, K_MATRIX).items()}
    assert all(np.array_equal(ref[k], out[k]) for k in ref)
    idx, score, n = (v.cpu().numpy() for v in eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"]))
    assert np.array_equal(n, rn)
    for b in range(4):
        assert np.array_equal(idx[b, : n[b]], ridx[b, : n[b]]) and np.array_equal(score[b, : n[b]].view(np.int32), rscore[b, : n[b]].view(np.int32))
    eng.set_substreams(2)
    o2 = eng.estimate(inp, K_MATRIX, out=eng.alloc_outputs(4))
    eng.flush()
    torch.cuda.current_stream().synchronize()
    assert all(np.array_equal(ref[k], o2[k].cpu().numpy()) for k in ref)
    eng.set_substreams(1)
    # keypoints beyond the active size are ignored: the same as handing in truncated lists
    assert eng.set_active_kpts(128) == 128
    cut = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    cut = [v.cpu().numpy().copy() for v in cut]
    n128 = torch.full_like(inp["n_q"], 128)
    tr = [v.cpu().numpy() for v in eng.match(inp["desc_q"], inp["kpt_q"], n128, inp["desc_r"], inp["kpt_r"], n128)]
    assert np.array_equal(cut[2], tr[2]) and (cut[2] > 10).all()
    for b in range(4):
        assert np.array_equal(cut[0][b, : cut[2][b]], tr[0][b, : tr[2][b]]) and cut[0][b, : cut[2][b]].max() < 128
    assert eng.set_active_kpts(10_000) == 640                              # clamped to the context's padded maximum
    out = {k: v.cpu().numpy() for k, v in eng.estimate(inp, K_MATRIX).items()}
    assert all(np.array_equal(ref[k], out[k]) for k in ref)


@pytest.mark.gpu
def test_fused_ffn_launch_matches_the_two_launch_form(state_dict_np, state_dict_t, dev):
    """k_gemm_p2ln (ffn.0 + LayerNorm + GELU in one launch, picked for >= 256 row tiles) against ffn.0 followed by k_ln_gelu:
    same correspondences and scores, and the final features of the fused form as close to the oracle as those of the two-launch
    form (the two differ from each other by LayerNorm-statistics rounding amplified through nine layers)."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=4, max_kpts=512, precision="f16x2_bf16_attn", state_dict=state_dict_np)
    pairs = [make_pair(120 + i, n_q=512 - 11 * i, n_r=500 - 7 * i) for i in range(4)]
    inp = eng.stage_inputs(pairs)
    args = (inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    T = 4 * 2 * 512
    res = {}
    for mode in (0, 2, 3):                                # developer knob 10: 0 = three launches, 2 = ffn.0 + LN + GELU fused, 3 = the whole tail (k_ffn_fused)
        eng.lib.gn_debug_set_variant(eng.ctx, 10, mode)
        idx, score, n = (v.cpu().numpy().copy() for v in eng.match(*args))
        res[mode] = (idx, score, n, eng.debug_read("x", T * 256).copy())
    eng.lib.gn_debug_set_variant(eng.ctx, 13, 0)          # knob 13: the same kernel with out_proj as a separate GEMM launch (message rows from memory)
    idx, score, n = (v.cpu().numpy().copy() for v in eng.match(*args))
    i4, s4, n4, x4 = idx, score, n, eng.debug_read("x", T * 256).copy()
    eng.lib.gn_debug_set_variant(eng.ctx, 13, 1)
    (i0, s0, n0, x0), (i2, s2, n2, x2), (i3, s3, n3, x3) = res[0], res[2], res[3]
    assert np.array_equal(n0, n4) and _rel(x4, x0) < 3e-5 and all(np.array_equal(i0[b, : n0[b]], i4[b, : n4[b]]) for b in range(4))
    assert np.array_equal(n0, n2) and np.array_equal(n0, n3) and (n0 > 100).all()
    for b in range(4):
        assert np.array_equal(i0[b, : n0[b]], i2[b, : n2[b]]) and np.array_equal(i0[b, : n0[b]], i3[b, : n3[b]])
        assert np.abs(s0[b, : n0[b]] - s2[b, : n0[b]]).max() < 1e-5 and np.abs(s0[b, : n0[b]] - s3[b, : n0[b]]).max() < 1e-5
    assert _rel(x2, x0) < 3e-5 and _rel(x3, x0) < 3e-5
    taps = {}
    oracle_match(state_dict_t, pairs[0], taps=taps)
    nq, nr = len(pairs[0].kp_q), len(pairs[0].kp_r)
    err = []
    for x in (x0, x2, x3):
        xb = x.reshape(4, 2, 512, 256)
        err.append(max(_rel(xb[0, 0, :nq], taps["layer8_0"][0].numpy()), _rel(xb[0, 1, :nr], taps["layer8_1"][0].numpy())))
    # bf16 attention puts this precision mode ~4e-5 from the f32 oracle after nine layers; the fused form must not be further away
    assert err[0] < 1e-4 and err[1] < 1.25 * err[0] + 5e-6 and err[2] < 1.25 * err[0] + 5e-6, err

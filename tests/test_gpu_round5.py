"""Round-5 parity tests (-m gpu): the HEADLINE KERNEL FAMILY under the oracle where it is weakest.

The low- / mid-margin mismatch table of rounds 2-4 ran on 4 pairs x 512 keypoints = 32 tiles of 128 tokens: below every bulk-grid threshold, i.e. on
`k_gemm_p2` + `k_attn16_v5` + `k_ffn_fused`, not on the kernels the bench line times.  Here:

  * the same table on `k_qkv<., ., 2>` (two-product projections) + `k_attn_pw` + the composed `k_ffn128`: (a) FORCED on the table's own 4 x 512 pairs
    (knobs 14 = 128, 1 = 70, 19 = 2) and (b) SELECTED by the grid itself at 16 pairs x 1024 keypoints; the kernel names of the run are asserted from
    the library's per-launch table, so the test cannot silently measure other kernels again;
  * a RAGGED bulk batch (16 pairs, N, M ~ U(400, 2500), one call padded to 2560, work lists on: knob 31 = 1, 2 and 3) directly against the oracle:
    indices identical in f32, counted (and bounded) in the headline mode on the headline kernels;
  * contexts of more than 512 pairs per call (k_tile_lists no longer has fixed-size prefix arrays); estimate_bucketed with the
    overlapped pose stage / deferred joins.

Everything counted is written to gpurun_out/parity_r05.json, stamped with gisnav_amd.build.source_digest(): profiles/r05_parity_report.json is a copy, and
bench.py prints its counts only next to the digest of the library it runs (reference semantics: pose_node.py:285-297 bit-exact `match_indices`,
:122 unbounded SIFT).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import oracle_match
from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW_MARGIN = dict(ffn_out_std=4.8e-3, final_scale=4.0, matchability_bias=0.0, matchability_std=0.05)
MID_MARGIN = dict(ffn_out_std=1.2e-3, final_scale=12.0, matchability_bias=2.0, matchability_std=0.05)
HEADLINE = "f16x2_f16_attn"


def _report(key, value):
    from gisnav_amd.build import source_digest
    path = os.path.join(ROOT, "gpurun_out", "parity_r05.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    if data.get("source_digest") != source_digest():      # a report of another build: start over
        data = {"source_digest": source_digest()}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _threads():
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))


def _mismatches(idx_gpu, k_gpu, oidx):
    a = {(int(q), int(r)) for q, r in idx_gpu[:k_gpu]}
    b = {(int(q), int(r)) for q, r in oidx}
    return len(a ^ b), len(b)


def _family(names):
    """Which block-tail / attention / projection kernels a run's launch table shows."""
    return {"k_ffn128": any(n.startswith("k_ffn128") for n in names), "k_ffn_fused": any(n.startswith("k_ffn_fused") for n in names),
            "k_attn_pw": any(n.startswith("k_attn_pw") for n in names), "k_attn16_v5": any(n.startswith("k_attn16_v5") for n in names),
            "k_qkv_2": any(n.startswith("k_qkv<") and n.rstrip(">").endswith(" 2") for n in names),
            "k_qkv_3": any(n.startswith("k_qkv<") and n.rstrip(">").endswith(" 3") for n in names)}


def _assert_headline_family(fam, products=2):
    assert fam["k_ffn128"] and fam["k_attn_pw"] and fam["k_qkv_%d" % products], fam
    assert not fam["k_ffn_fused"] and not fam["k_attn16_v5"] and not fam["k_qkv_%d" % (5 - products)], fam


class _Knobs:
    """gn_debug_set_variant settings for the duration of a block (the knobs belong to `eng` alone; restored on leaving the block)."""

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, {int(k[1:]): v for k, v in kv.items()}
        self.default = {14: 0, 1: 4, 19: 1, 27: 2, 31: 1, 32: 1}

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.eng.lib.gn_debug_set_variant(self.eng.ctx, k, v) == 0
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            self.eng.lib.gn_debug_set_variant(self.eng.ctx, k, self.default[k])


def _match_counted(eng, pairs, ref):
    inp = eng.stage_inputs(pairs)
    eng.set_kernel_timing(400)
    idx, score, n_match = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table()]
    eng.set_kernel_timing(0)
    mism = total = 0
    idx_h, n_h = idx.cpu().numpy(), n_match.cpu().numpy()
    for b, r in enumerate(ref):
        d, t = _mismatches(idx_h[b], int(n_h[b]), r[3].numpy())
        mism += d; total += t
    return mism, total, _family(names), (idx_h, n_h)


@pytest.mark.parametrize("name,kw,th", [("low_margin", LOW_MARGIN, 0.0), ("mid_margin", MID_MARGIN, 0.01)])
def test_headline_kernels_forced_on_the_low_margin_table(name, kw, th):
    """The 4 x 512 pairs of test_gpu_parity2's table, with the bulk kernels FORCED (knob 14 = 128: k_ffn128 with the composed first GEMM; 1 = 70:
    k_attn_pw; 19 = 2: k_qkv at any grid size; 27 = 2 / 3: two / three partial products).  f32 must be 0; the headline family is counted, bounded at
    1 % of the oracle's matches, and must not be worse than the small-grid kernels' count + 2."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    sd = synthetic_state_dict(0, **kw)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    pairs = [make_pair(400 + i, n_q=512 - 31 * i, n_r=512 - 17 * i) for i in range(4)]
    ref = [oracle_match(tsd, p, filter_threshold=th) for p in pairs]
    table = {}
    eng = PoseEngine(0, max_batch=4, max_kpts=512, precision="f32", state_dict=sd, filter_threshold=th)
    m, t, _, _ = _match_counted(eng, pairs, ref)
    table["f32"] = {"index_mismatches": m, "cpu_matches": t}
    del eng
    eng = PoseEngine(0, max_batch=4, max_kpts=512, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    m, t, fam, _ = _match_counted(eng, pairs, ref)
    assert fam["k_ffn_fused"] and fam["k_attn16_v5"] and not fam["k_ffn128"] and not fam["k_attn_pw"], fam      # what this grid selects by itself
    table["small_grid_kernels"] = {"index_mismatches": m, "cpu_matches": t, "kernels": "k_gemm_p2 (3 products) + k_attn16_v5 + k_ffn_fused"}
    for products in (2, 3):
        with _Knobs(eng, k14=128, k1=70, k19=2, k27=products):
            m, t, fam, _ = _match_counted(eng, pairs, ref)
        _assert_headline_family(fam, products)
        table["headline_kernels_%d_products" % products] = {"index_mismatches": m, "cpu_matches": t,
                                                            "kernels": "k_qkv<., ., %d> + k_attn_pw + k_ffn128 (composed)" % products}
    del eng
    print(name, table)
    _report("forced_4x512_" + name, table)
    assert table["f32"]["index_mismatches"] == 0, table
    head = table["headline_kernels_2_products"]
    assert head["index_mismatches"] <= 0.01 * head["cpu_matches"], table
    assert head["index_mismatches"] <= table["small_grid_kernels"]["index_mismatches"] + 2, table


@pytest.mark.parametrize("name,kw,th", [("low_margin", LOW_MARGIN, 0.0), ("mid_margin", MID_MARGIN, 0.01)])
def test_headline_kernels_selected_by_a_bulk_grid_on_low_margin_weights(name, kw, th):
    """16 pairs x 1024 keypoints: 256 tiles of 128 tokens, 512 attention items -- the grid itself selects k_qkv<., ., 2>, k_attn_pw and k_ffn128,
    with the work lists on (the default), exactly as in the bench's 32-pair step.  Counted against the oracle, bounded at 1 %."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    sd = synthetic_state_dict(0, **kw)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    pairs = [make_pair(4400 + i, n_q=1024 - 13 * (i % 5), n_r=1024 - 29 * (i % 3)) for i in range(16)]
    ref = [oracle_match(tsd, p, filter_threshold=th) for p in pairs]
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    m, t, fam, _ = _match_counted(eng, pairs, ref)
    _assert_headline_family(fam, 2)
    del eng
    row = {"index_mismatches": m, "cpu_matches": t, "kernels": "k_qkv<., ., 2> + k_attn_pw + k_ffn128 (composed), selected by the grid"}
    print(name, row)
    _report("bulk_16x1024_" + name, row)
    assert t > 500 and m <= 0.01 * t, row


def test_ragged_bulk_batch_with_work_lists_directly_against_the_oracle(state_dict_np, state_dict_t):
    """16 pairs with N, M ~ U(400, 2500) in ONE call padded to 2560 (the bench's ragged workload at half the batch), margin-built weights.
    f32: correspondence indices identical to the oracle's for every pair (the lists do not exist in that mode: it is the reference point).
    Headline mode on the headline kernels (asserted from the launch table) with the work lists in each form -- knob 31 = 1 (automatic), 2 (the
    block tail always walks), 3 (never walks) and 0 (no lists) -- : identical to each other bit for bit, and compared with the ORACLE: counted,
    bounded at 0.1 % of its matches (measured: 0)."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    rs = np.random.default_rng(77)
    nq = rs.integers(400, 2501, 16); nr = rs.integers(400, 2501, 16)
    pairs = [make_pair(500 + i, n_q=int(nq[i]), n_r=int(nr[i])) for i in range(16)]
    npad = ((max(max(len(p.kp_q), len(p.kp_r)) for p in pairs) + 127) // 128) * 128
    ref = [oracle_match(state_dict_t, p) for p in pairs]
    eng = PoseEngine(0, max_batch=16, max_kpts=npad, precision="f32", state_dict=state_dict_np)
    m, t, _, _ = _match_counted(eng, pairs, ref)
    del eng
    assert m == 0 and t > 3000, (m, t)
    eng = PoseEngine(0, max_batch=16, max_kpts=npad, precision=HEADLINE, state_dict=state_dict_np)
    rows, first = {}, None
    for lists in (1, 2, 3, 0):
        with _Knobs(eng, k31=lists):
            for _ in range(2):      # the second call of the automatic form has seen the first one's padding
                m, t, fam, (idx_h, n_h) = _match_counted(eng, pairs, ref)
        _assert_headline_family(fam, 2)
        rows["lists_%d" % lists] = {"index_mismatches": m, "cpu_matches": t}
        if first is None:
            first = (idx_h, n_h)
        else:
            assert np.array_equal(n_h, first[1]) and all(np.array_equal(idx_h[b, : n_h[b]], first[0][b, : n_h[b]]) for b in range(16)), lists
    del eng
    real = int(sum(len(p.kp_q) + len(p.kp_r) for p in pairs))
    rows["padded_to"] = int(npad); rows["padding_waste"] = round(1.0 - real / (32.0 * npad), 4)
    print("ragged 16 x U(400, 2500):", rows)
    _report("ragged_16_pairs_u400_2500", rows)
    assert rows["lists_1"]["index_mismatches"] <= 0.001 * t, rows


def test_more_than_512_pairs_per_call_with_work_lists(state_dict_np, state_dict_t):
    """k_tile_lists kept per-slot prefix sums in two 1025-entry LDS arrays -- a call of more than 512 pairs overran them.
    600 pairs x <= 128 keypoints in one call, headline mode, bulk kernels forced (so the lists are read): every 37th pair against the oracle, and
    the whole batch against the same call without lists."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    B = 600
    base = [make_pair(7000 + i, n_q=128 - (i * 7) % 90, n_r=128 - (i * 11) % 70) for i in range(24)]
    pairs = [base[i % 24] for i in range(B)]
    eng = PoseEngine(0, max_batch=B, max_kpts=128, precision=HEADLINE, state_dict=state_dict_np)
    inp = eng.stage_inputs(pairs)
    res = {}
    for lists in (1, 0):
        with _Knobs(eng, k14=128, k19=2, k31=lists):
            idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
            torch.cuda.synchronize()
            res[lists] = (idx.cpu().numpy(), n.cpu().numpy())
    assert np.array_equal(res[1][1], res[0][1]) and res[1][1].max() > 40
    assert all(np.array_equal(res[1][0][b, : res[1][1][b]], res[0][0][b, : res[0][1][b]]) for b in range(B))
    for b in list(range(0, B, 37)) + [511, 512, 513, B - 1]:
        oidx = oracle_match(state_dict_t, pairs[b])[3].numpy()
        assert int(res[1][1][b]) == len(oidx) and np.array_equal(res[1][0][b, : len(oidx)], oidx), b
    del eng


def test_estimate_bucketed_with_overlapped_pose_stage_and_deferred_joins(state_dict_np):
    """estimate_bucketed read its scratch outputs while the overlapped PnP stage / unjoined sub-batch groups could still be
    running.  With the flush in place the bucketed result equals the plain call's in every mode."""
    from gisnav_amd.engine import PoseEngine
    rs = np.random.default_rng(5)
    nq = rs.integers(200, 1000, 12); nr = rs.integers(200, 1000, 12)
    pairs = [make_pair(900 + i, n_q=int(nq[i]), n_r=int(nr[i])) for i in range(12)]
    eng = PoseEngine(0, max_batch=12, max_kpts=1024, precision=HEADLINE, state_dict=state_dict_np)
    inp = eng.stage_inputs(pairs)
    n_q = np.array([len(p.kp_q) for p in pairs]); n_r = np.array([len(p.kp_r) for p in pairs])
    want = {k: v.clone() for k, v in eng.estimate(inp, K_MATRIX).items()}
    torch.cuda.synchronize()
    assert int(want["ok"].sum()) >= 10
    for mode in ("overlap", "deferred"):
        if mode == "overlap":
            eng.set_overlap(True)
        else:
            eng.set_overlap(False); eng.set_substreams(2, deferred_join=True)
        for _ in range(3):
            got, _ = eng.estimate_bucketed(inp, K_MATRIX, n_q, n_r, bucket_pairs=4)
            # read on the caller's stream, in stream order, with NO flush by the caller
            assert torch.equal(got["ok"], want["ok"]) and torch.equal(got["n_match"], want["n_match"]), mode
            assert float((got["R"] - want["R"]).abs().max()) < 1e-9 and float((got["t"] - want["t"]).abs().max()) < 1e-6, mode
    eng.set_substreams(1)
    eng.flush()
    del eng


@pytest.mark.parametrize("products", [3, 2])
def test_projection_fused_into_the_block_tail_gives_the_bits_of_the_separate_launches(state_dict_np, state_dict_t, products):
    """Round 5: on bulk grids k_ffn128 computes the NEXT block's attention input projection from the rows its epilogue has just produced
    (k_ffn128<0, true, ., 1 / 2>; knob 32).  Same partial products in the same order and the same epilogue expressions as k_qkv<., true, 2>:
    everything downstream -- match descriptors, scores, correspondence indices, poses -- is BITWISE what the separate launches give; the launch
    table shows 17 fused tails + 1 plain one and ONE k_qkv launch (the first block's) instead of 18.  Checked on a full batch (16 x 1024), on a
    ragged one (work lists; the walking and the one-tile form of the tail), and the full batch against the oracle.  On both block-tail levels
    (gn_set_ffn_products 3 and 2: k_ffn128<., ., ., 1 / 2, PROD>)."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    rs = np.random.default_rng(3)
    full = [make_pair(8800 + i, n_q=1024, n_r=1024 - 7 * (i % 4)) for i in range(16)]
    rag = [make_pair(8900 + i, n_q=int(rs.integers(60, 1025)), n_r=int(rs.integers(60, 1025))) for i in range(16)]
    eng = PoseEngine(0, max_batch=16, max_kpts=1024, precision=HEADLINE, state_dict=state_dict_np)
    eng.set_ffn_products(products)
    for label, pairs, forms in (("full", full, (1,)), ("ragged", rag, (2, 3))):
        inp = eng.stage_inputs(pairs)
        for lists in forms:
            got = {}
            for fused in (1, 0):
                with _Knobs(eng, k31=lists):
                    eng.lib.gn_debug_set_variant(eng.ctx, 32, fused)
                    eng.set_kernel_timing(400)
                    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
                    torch.cuda.synchronize()
                    tab = {r["name"]: int(r["launches"]) for r in eng.kernel_table()}
                    eng.set_kernel_timing(0)
                    md = eng.debug_read("md", 2 * 16 * 1024 * 256).copy()
                    out = eng.estimate(inp, K_MATRIX)
                    torch.cuda.synchronize()
                    got[fused] = (idx.cpu().numpy().copy(), score.cpu().numpy().copy(), n.cpu().numpy().copy(), md, out["R"].cpu().numpy().copy(), tab)
            eng.lib.gn_debug_set_variant(eng.ctx, 32, 1)
            a, b = got[1], got[0]
            fused_tail = lambda k: k.startswith("k_ffn128") and k.rstrip(">").split(", ")[3] in ("1", "2")      # noqa: E731  (k_ffn128<ABL, COMP, LOOP, QKV, PROD>)
            nf = sum(v for k, v in a[5].items() if fused_tail(k))
            assert nf == 17 and sum(v for k, v in a[5].items() if k.startswith("k_qkv")) == 1, a[5]
            assert all(k.rstrip(">").split(", ")[4] == str(products) for k in list(a[5]) + list(b[5]) if k.startswith("k_ffn128")), (a[5], b[5])
            assert sum(v for k, v in b[5].items() if k.startswith("k_qkv")) == 18 and not any(fused_tail(k) for k in b[5]), b[5]
            assert np.array_equal(a[2], b[2]) and a[2].max() > 300, (label, lists)
            for p in range(16):
                k = int(a[2][p])
                assert np.array_equal(a[0][p, :k], b[0][p, :k]) and np.array_equal(a[1][p, :k].view(np.uint32), b[1][p, :k].view(np.uint32)), (label, lists, p)
                nq, nr = len(pairs[p].kp_q), len(pairs[p].kp_r)
                for side, nv in ((0, nq), (1, nr)):        # the match descriptors of the VALID tokens, bit for bit
                    lo = (2 * p + side) * 1024 * 256
                    assert np.array_equal(a[3][lo: lo + nv * 256].view(np.uint32), b[3][lo: lo + nv * 256].view(np.uint32)), (label, lists, p, side)
            assert np.array_equal(a[4], b[4]), (label, lists)
        if label == "full":
            ref = [oracle_match(state_dict_t, p) for p in pairs]
            m, t, fam, _ = _match_counted(eng, pairs, ref)
            assert fam["k_ffn128"] and fam["k_attn_pw"] and m == 0 and t > 8000, (m, t, fam)
            _report(f"fused_tail_projection_16x1024_margin_built{'' if products == 3 else '_two_products'}", {"index_mismatches": m, "cpu_matches": t})
    del eng


def _attn_ref64(q, k, v, nkv, cross, cast):
    BS, n, _ = q.shape
    outs = []
    for bs in range(BS):
        kvs = bs ^ 1 if cross else bs
        m = int(nkv[kvs])
        qq = cast(q[bs] * 0.125).double().cpu().reshape(n, 4, 64).transpose(0, 1)
        kk = cast(k[kvs, :m]).double().cpu().reshape(m, 4, 64).transpose(0, 1)
        vv = cast(v[kvs, :m]).double().cpu().reshape(m, 4, 64).transpose(0, 1)
        outs.append((torch.softmax(qq @ kk.transpose(1, 2), -1) @ vv).transpose(0, 1).reshape(n, 256).numpy())
    return outs


@pytest.mark.parametrize("cross", [False, True])
def test_key_split_attention_of_one_pair_against_fp64(state_dict_np, cross):
    """k_attn_ks (round 5; the reference's operating point is ONE pair per message, pose_node.py:178-184): the four waves of a workgroup share
    32 queries and split the key tiles, partial results merged through LDS.  One pair x 1024 tokens per side with ragged key counts (a side
    with 5 keys: three waves of every workgroup have no tile; 833: a masked last tile), against fp64 on the fp16-rounded operands (only the
    rounding of the probabilities is left: same bound as k_attn16_v5's test) and against k_attn16_v5 itself; selected by the grid on its own."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=1, max_kpts=1024, precision=HEADLINE, state_dict=state_dict_np)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(17)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())      # noqa: E731
    worst = 0.0
    for nk in ((1024, 833), (5, 1000), (64, 65)):
        q, k, v = (torch.randn(2, 1024, 256, generator=g).to(dev) for _ in range(3))
        k[1, 7] *= 6.0
        nkv = torch.tensor(nk, dtype=torch.int32, device=dev)
        eng.set_kernel_timing(8)
        out = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
        names = [r["name"] for r in eng.kernel_table()]
        eng.set_kernel_timing(0)
        eng.lib.gn_debug_set_variant(eng.ctx, 1, 5)
        try:
            v5 = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
        finally:
            eng.lib.gn_debug_set_variant(eng.ctx, 1, 4)
        ref = _attn_ref64(q, k, v, nkv, cross, lambda t: t.half())
        assert np.isfinite(out).all()
        for bs in range(2):
            worst = max(worst, rel(out[bs], ref[bs]))
            assert rel(out[bs], ref[bs]) < 1.5e-3 and rel(out[bs], v5[bs]) < 1.5e-3, (nk, bs, rel(out[bs], ref[bs]), rel(out[bs], v5[bs]))
    _report("attn_ks_rel_err_vs_fp64_cross%d" % int(cross), worst)
    del eng


def test_one_pair_runs_the_small_grid_kernels_and_matches_the_oracle(state_dict_np, state_dict_t):
    """Batch 1 (the reference's operating point): the launch table shows k_attn_ks, and the correspondences of full-size pairs are the oracle's."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    eng = PoseEngine(0, max_batch=1, max_kpts=1024, precision=HEADLINE, state_dict=state_dict_np)
    m_all = t_all = 0
    for seed, nq, nr in ((9100, 1024, 1024), (9101, 1000, 777), (9102, 333, 1024)):
        p = make_pair(seed, n_q=nq, n_r=nr)
        ref = [oracle_match(state_dict_t, p)]
        inp = eng.stage_inputs([p])
        eng.set_kernel_timing(200)
        idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        torch.cuda.synchronize()
        names = [r["name"] for r in eng.kernel_table()]
        eng.set_kernel_timing(0)
        assert any(nm.startswith("k_attn_ks") for nm in names), names
        d, t = _mismatches(idx.cpu().numpy()[0], int(n.cpu().numpy()[0]), ref[0][3].numpy())
        m_all += d; t_all += t
    assert m_all == 0 and t_all > 600, (m_all, t_all)
    _report("one_pair_small_grid_kernels_margin_built", {"index_mismatches": m_all, "cpu_matches": t_all})
    del eng


def test_small_grid_projections_give_the_bits_of_the_bulk_kernel_and_the_small_grid_tail_its_features(state_dict_np):
    """gn_skinny.hip (one pair per call): k_skinny_qkv forms k_qkv's partial products in k_qkv's order with k_qkv's epilogue expressions, so with
    the block tail held fixed (knob 33 = 9: projections only) EVERYTHING downstream of the 18 projections is bitwise what the bulk kernel (forced by
    knob 19 = 2) gives; the two-launch tail (knob 33 = 5: tail only) uses k_ln_gelu's row arithmetic and one accumulator per output like k_ffn_fused,
    but another k order inside the composed ffn.0 (natural instead of register-fed), so the final residual stream agrees to f32 rounding and the
    correspondences are identical."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=1, max_kpts=1024, precision=HEADLINE, state_dict=state_dict_np)
    eng.lib.gn_debug_set_variant(eng.ctx, 19, 2)          # the bulk k_qkv also on this small grid
    p = make_pair(9200, n_q=1024, n_r=901)
    inp = eng.stage_inputs([p])
    got = {}
    for knob in (0, 9, 5, 1):
        eng.lib.gn_debug_set_variant(eng.ctx, 33, knob)
        eng.set_kernel_timing(400)
        idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
        torch.cuda.synchronize()
        names = {r["name"].split("<")[0] for r in eng.kernel_table()}
        eng.set_kernel_timing(0)
        got[knob] = (idx.cpu().numpy()[0].copy(), score.cpu().numpy()[0].copy(), int(n.cpu().numpy()[0]), eng.debug_read("x", 2 * 1024 * 256).copy(), names)   # the residual stream behind the last block
    eng.lib.gn_debug_set_variant(eng.ctx, 33, 1); eng.lib.gn_debug_set_variant(eng.ctx, 19, 1)
    assert "k_qkv" in got[0][4] and "k_skinny_qkv" not in got[0][4] and "k_skinny_h" not in got[0][4], got[0][4]
    assert "k_skinny_qkv" in got[9][4] and "k_qkv" not in got[9][4] and "k_skinny_h" not in got[9][4], got[9][4]
    assert "k_skinny_h" in got[5][4] and "k_skinny_out" in got[5][4] and "k_skinny_qkv" not in got[5][4], got[5][4]
    assert {"k_skinny_qkv", "k_skinny_h", "k_skinny_out"} <= got[1][4], got[1][4]
    a, b = got[0], got[9]
    assert a[2] == b[2] and a[2] > 200
    assert np.array_equal(a[0][:a[2]], b[0][:a[2]]) and np.array_equal(a[1][:a[2]].view(np.uint32), b[1][:a[2]].view(np.uint32))
    for side, nv in ((0, 1024), (1, 901)):
        lo = side * 1024 * 256
        assert np.array_equal(a[3][lo: lo + nv * 256].view(np.uint32), b[3][lo: lo + nv * 256].view(np.uint32)), side
    worst = 0.0
    for knob in (5, 1):
        c = got[knob]
        assert c[2] == a[2] and np.array_equal(c[0][:a[2]], a[0][:a[2]]), knob
        for side, nv in ((0, 1024), (1, 901)):
            lo = side * 1024 * 256
            d = float(np.abs(c[3][lo: lo + nv * 256] - a[3][lo: lo + nv * 256]).max() / np.abs(a[3][lo: lo + nv * 256]).max())
            worst = max(worst, d)
            assert d < 2e-5, (knob, side, d)
    assert np.abs(a[3]).max() > 0.1
    _report("small_grid_tail_vs_k_ffn_fused_final_features_rel", worst)
    del eng


@pytest.mark.parametrize("cross", [False, True])
def test_exact_f32_key_split_attention_of_one_pair_against_fp64(state_dict_np, cross):
    """k_attn_f32_ks (round 5): BASELINE configs[1] as SURVEY.md reads it -- one pair per call in the guaranteed f32 arithmetic.  The four waves of a
    workgroup share 32 queries and split the 32-key tiles (wave-private LDS, the next tile prefetched into registers), merged through LDS.  Ragged
    key counts as in the fp16 twin's test (5 keys: three waves without a tile; 833: a masked last tile; 0 keys: an empty side gives zeros),
    against fp64 at f32 accuracy and against k_attn_f32 (knob 43 = 1), selected by the number of pairs on its own."""
    from gisnav_amd.engine import PoseEngine
    eng = PoseEngine(0, max_batch=1, max_kpts=1024, precision="f32", state_dict=state_dict_np)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(23)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())      # noqa: E731
    worst = 0.0
    try:
        for nk in ((1024, 833), (5, 1000), (64, 65), (33, 0)):
            q, k, v = (torch.randn(2, 1024, 256, generator=g).to(dev) for _ in range(3))
            k[1, 7] *= 6.0
            nkv = torch.tensor(nk, dtype=torch.int32, device=dev)
            out = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()      # (two slots: the key-split kernel; the launch table of the next test names it)
            eng.lib.gn_debug_set_variant(eng.ctx, 43, 4)                             # its eight-wave form (two waves per SIMD; measured, not shipped)
            out4 = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
            eng.lib.gn_debug_set_variant(eng.ctx, 43, 1)
            old = eng.debug_attention(q, k, v, nkv, cross, 0.125).cpu().numpy()
            eng.lib.gn_debug_set_variant(eng.ctx, 43, 0)
            ref = _attn_ref64(q, k, v, nkv, cross, lambda t: t)
            assert np.isfinite(out).all()
            for bs in range(2):
                kvs = bs ^ 1 if cross else bs
                if nk[kvs] == 0:
                    assert not out[bs].any() and not old[bs].any() and not out4[bs].any()
                    continue
                assert rel(out4[bs], ref[bs]) < 5e-6, (nk, bs, rel(out4[bs], ref[bs]))
                worst = max(worst, rel(out[bs], ref[bs]))
                assert rel(out[bs], ref[bs]) < 5e-6 and rel(out[bs], old[bs]) < 2e-5, (nk, bs, rel(out[bs], ref[bs]), rel(out[bs], old[bs]))
    finally:
        eng.lib.gn_debug_set_variant(eng.ctx, 43, 0)
    _report("attn_f32_ks_rel_err_vs_fp64_cross%d" % int(cross), worst)
    del eng


def test_one_pair_in_the_exact_f32_mode_small_grid_kernels_against_the_oracle_and_the_bulk_kernels(state_dict_np, state_dict_t):
    """One pair per call in GN_PREC_F32 (BASELINE configs[1] as SURVEY.md reads it): the launch table shows k_attn_f32_ks and the 64-row GEMM
    (k_gemm_f32_m64 / its four-slot-ring form k_gemm_f32_r64, also behind the rotary / column-scale / residual epilogues); correspondence indices are the oracle's; with the 64-row
    GEMM switched off (knob 41 = 0) every output is BITWISE the same (it sums the same products in the same order as k_gemm_f32_v3); with the
    key-split attention switched off as well (knob 43 = 1) the indices stay identical and the scores agree to f32 rounding."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    eng = PoseEngine(0, max_batch=1, max_kpts=1024, precision="f32", state_dict=state_dict_np)
    m_all = t_all = 0
    try:
        for seed, nq, nr in ((9200, 1024, 1024), (9201, 1000, 777), (9202, 333, 1024)):
            p = make_pair(seed, n_q=nq, n_r=nr)
            ref = oracle_match(state_dict_t, p)
            inp = eng.stage_inputs([p])
            args = (inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
            eng.set_kernel_timing(200)
            idx, score, n = (t.clone() for t in eng.match(*args))
            torch.cuda.synchronize()
            names = [r["name"] for r in eng.kernel_table()]
            eng.set_kernel_timing(0)
            assert any(nm.startswith("k_attn_f32_ks") for nm in names) and any(nm.startswith(("k_gemm_f32_m64", "k_gemm_f32_r64")) for nm in names), names
            assert not any(nm.startswith("k_gemm_f32_v3") for nm in names), names        # every GEMM of the call is on 64-row tiles at one pair
            d, t = _mismatches(idx.cpu().numpy()[0], int(n.cpu().numpy()[0]), ref[3].numpy())
            m_all += d; t_all += t
            eng.lib.gn_debug_set_variant(eng.ctx, 41, 0)
            idx2, score2, n2 = (t.clone() for t in eng.match(*args))
            k = int(n.item())                   # (entries behind the match count are not written)
            assert torch.equal(n, n2) and torch.equal(idx[0, :k], idx2[0, :k]) and torch.equal(score[0, :k], score2[0, :k])
            eng.lib.gn_debug_set_variant(eng.ctx, 43, 1)
            idx3, score3, n3 = (t.clone() for t in eng.match(*args))
            assert torch.equal(n, n3) and torch.equal(idx[0, :k], idx3[0, :k]) and float((score[0, :k] - score3[0, :k]).abs().max()) < 1e-5
            eng.lib.gn_debug_set_variant(eng.ctx, 41, 320)
            eng.lib.gn_debug_set_variant(eng.ctx, 43, 0)
    finally:
        eng.lib.gn_debug_set_variant(eng.ctx, 41, 320)
        eng.lib.gn_debug_set_variant(eng.ctx, 43, 0)
    assert m_all == 0 and t_all > 600, (m_all, t_all)
    _report("one_pair_exact_f32_small_grid_kernels", {"index_mismatches": m_all, "cpu_matches": t_all})
    del eng

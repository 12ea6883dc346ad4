"""GPU tests (-m gpu) of the split-fp16 attention (k_attn_f16x2), the precision mode built on it (GN_PREC_F16X2_F16X2_ATTN = 5, "f16x2_f16x2_attn")
and the certificate's re-run ladder (gn_set_certify_ladder: flagged pairs re-run in mode-5 arithmetic before exact f32).

What is measured goes to test_reports/parity_ladder.json (git-ignored), stamped with the digest of the loaded library.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import oracle_match
from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import default_init_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW_MARGIN = dict(ffn_out_std=4.8e-3, final_scale=4.0, matchability_bias=0.0, matchability_std=0.05)
MID_MARGIN = dict(ffn_out_std=1.2e-3, final_scale=12.0, matchability_bias=2.0, matchability_std=0.05)
HEADLINE = "f16x2_f16_attn"
MODE5 = "f16x2_f16x2_attn"
SAFETY = 4.0
FAMILIES = {"low_margin": (lambda: synthetic_state_dict(0, **LOW_MARGIN), 0.0), "mid_margin": (lambda: synthetic_state_dict(0, **MID_MARGIN), 0.01),
            "margin_built": (lambda: synthetic_state_dict(0), 0.5), "default_init": (lambda: default_init_state_dict(0), 0.0)}
_REF_CACHE = {}


def _report(key, value):
    from gisnav_amd import _lib
    path = os.path.join(ROOT, "test_reports", "parity_ladder.json")
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


def _family(name):
    make, th = FAMILIES[name]
    sd = make()
    return sd, {k: torch.from_numpy(v) for k, v in sd.items()}, th


def _pairs(shape):
    if shape == "4x512":
        return [make_pair(400 + i, n_q=512 - 31 * i, n_r=512 - 17 * i) for i in range(4)], [make_pair(460 + i, n_q=500, n_r=490) for i in range(4)], 4, 512
    if shape == "8x1024":
        return [make_pair(6400 + i, n_q=1024 - 11 * (i % 3), n_r=1024 - 19 * (i % 4)) for i in range(8)], [make_pair(6460 + i, n_q=1024, n_r=1000) for i in range(8)], 8, 1024
    return [make_pair(4400 + i, n_q=1024 - 13 * (i % 5), n_r=1024 - 29 * (i % 3)) for i in range(16)], [make_pair(4460 + i, n_q=1024, n_r=1000) for i in range(16)], 16, 1024


def _refs(name, shape):
    key = (name, shape)
    if key not in _REF_CACHE:
        _threads()
        _, tsd, th = _family(name)
        _REF_CACHE[key] = [oracle_match(tsd, p, filter_threshold=th)[3].numpy() for p in _pairs(shape)[0]]
    return _REF_CACHE[key]


def _sets(idx_h, n_h):
    return [{(int(q), int(c)) for q, c in idx_h[b, : int(n_h[b])]} for b in range(len(n_h))]


def _diff(idx_h, n_h, refs):
    got = _sets(idx_h, n_h)
    per = [len(got[b] ^ {(int(q), int(c)) for q, c in r}) for b, r in enumerate(refs)]
    return sum(per), per


def _match(eng, inp):
    idx, score, n = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    torch.cuda.synchronize()
    return idx.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("npad,BS", [(128, 2), (1024, 2), (4096, 2), (512, 34)])
@pytest.mark.parametrize("cross", [False, True])
def test_split_attention_is_f32_accurate(npad, BS, cross):
    """k_attn_f16x2 through gn_debug_attention on a mode-5 context (BS <= 16: the key-split form, else the bulk form) against a float64 reference:
    self and cross attention, ragged key counts, one spiked key (the running maximum jumps mid-sequence), and the operands scaled by 2^-8, 1 and 2^8
    (the power-of-two operand scales).  Error <= 4e-6 of max |ref| and <= 2x k_attn_f32's on the same inputs (floor 2^-21: see below); two runs
    bitwise equal."""
    from gisnav_amd.engine import PoseEngine
    _threads()
    e5 = PoseEngine(0, max_batch=max(1, BS // 2), max_kpts=npad, precision=MODE5)
    e32 = PoseEngine(0, max_batch=max(1, BS // 2), max_kpts=npad, precision="f32")
    dev = e5.device
    g = torch.Generator(device="cpu").manual_seed(npad + BS + int(cross))
    base = [torch.randn(BS, npad, 256, generator=g) for _ in range(3)]
    base[1][1, min(37, npad - 1)] *= 6.0                         # spiked key
    nkv = torch.tensor([npad - (37 * b) % (npad // 2) for b in range(BS)], dtype=torch.int32)
    nkv[BS - 1] = 5
    rows = {}
    for sc in (2.0 ** -8, 1.0, 2.0 ** 8):
        # q and v scaled by sc, k by 1 / sc: every operand's magnitude moves by 2^8 either way while the scores -- and with them the conditioning of
        # the softmax -- stay those of the unscaled inputs (scaling q and k alike would move the scores by 2^16, where f32 itself loses 1e-3)
        q, k, v = base[0] * sc, base[1] / sc, base[2] * sc
        qd, kd, vd = (x.to(dev) for x in (q, k, v))
        out = e5.debug_attention(qd, kd, vd, nkv.to(dev), cross, 0.125).cpu().numpy()
        again = e5.debug_attention(qd, kd, vd, nkv.to(dev), cross, 0.125).cpu().numpy()
        o32 = e32.debug_attention(qd, kd, vd, nkv.to(dev), cross, 0.125).cpu().numpy()
        assert np.array_equal(out, again), sc
        err5 = err32 = 0.0
        for bs in range(BS):
            kvs = bs ^ 1 if cross else bs
            m = int(nkv[kvs])
            qq = q[bs].double().reshape(npad, 4, 64).transpose(0, 1) * 0.125
            kk = k[kvs, :m].double().reshape(m, 4, 64).transpose(0, 1)
            vv = v[kvs, :m].double().reshape(m, 4, 64).transpose(0, 1)
            ref = (torch.softmax(qq @ kk.transpose(1, 2), -1) @ vv).transpose(0, 1).reshape(npad, 256).numpy()
            err5, err32 = max(err5, _rel(out[bs], ref)), max(err32, _rel(o32[bs], ref))
        rows[str(sc)] = {"k_attn_f16x2": err5, "k_attn_f32": err32}
        assert np.isfinite(out).all()
        assert err5 <= 4e-6, (sc, err5, err32)      # (k_attn_f32 itself measures 3.5e-6 on the 4096-key inputs with the spiked key)
        # no worse than twice k_attn_f32's error -- or than 2^-21 where that is smaller: on rows whose softmax is one-hot (scaled by 2^8 the scores
        # reach ~1e5) k_attn_f32 returns the winning v row exactly, while two fp16 terms hold v to 22 significant bits
        assert err5 <= max(2.0 * err32, 2.0 ** -21), (sc, err5, err32)
    _report(f"attention_npad{npad}_bs{BS}_{'cross' if cross else 'self'}", rows)


# ---------------------------------------------------------------------------------------------------------------- 2. mode 5 end to end
@pytest.mark.parametrize("shape", ["4x512", "16x1024"])
def test_mode5_indices_equal_the_oracle_on_margin_built_weights(shape):
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family("margin_built")
    pairs, _, B, K = _pairs(shape)
    refs = _refs("margin_built", shape)
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=MODE5, state_dict=sd, filter_threshold=th)
    eng.set_kernel_timing(400)
    idx_h, n_h, _ = _match(eng, eng.stage_inputs(pairs))
    names = [r["name"] for r in eng.kernel_table()]
    eng.set_kernel_timing(0)
    assert any(n.startswith("k_attn_f16x2") for n in names), names
    assert not any(n.startswith(("k_attn_pw", "k_attn16", "k_attn_bf16", "k_qkv", "k_attn_f32")) for n in names), names
    m, per = _diff(idx_h, n_h, refs)
    _report(f"mode5_{shape}_margin_built", {"index_mismatches": m, "oracle_matches": sum(len(r) for r in refs)})
    assert m == 0, per


def test_mode5_refused_for_superpoint_contexts():
    from gisnav_amd import _lib
    from gisnav_amd.engine import PoseEngine
    with pytest.raises(_lib.GnError):
        PoseEngine(0, max_batch=1, max_kpts=256, precision=MODE5, feature="superpoint")


# ---------------------------------------------------------------------------------------------------------------- 3. the eps it buys
@pytest.mark.parametrize("name", ["low_margin", "mid_margin", "default_init"])
def test_mode5_error_is_a_fraction_of_the_headline_modes(name):
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family(name)
    _, cal_pairs, B, K = _pairs("8x1024")
    got = {}
    for prec in (HEADLINE, MODE5):
        eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=prec, state_dict=sd, filter_threshold=th)
        got[prec] = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)["measured"]
        del eng
    _report(f"eps_measured_{name}", {"headline_max_dP": got[HEADLINE], "mode5_max_dP": got[MODE5]})
    # measured: low margin 9.95e-3 -> 5.1e-5, mid margin 3.76e-4 -> 3.6e-5 (a quarter or less); default-init 3.5e-5 -> 1.9e-5 only -- there the
    # headline mode's error is already at the level of the other stages', which the split attention does not change
    assert got[MODE5] <= (0.25 if name != "default_init" else 0.75) * got[HEADLINE], got


# ---------------------------------------------------------------------------------------------------------------- 4. certified with the ladder
def _f32_indices(sd, th, pairs, B, K):
    from gisnav_amd.engine import PoseEngine
    e32 = PoseEngine(0, max_batch=B, max_kpts=K, precision="f32", state_dict=sd, filter_threshold=th)
    idx, n, _ = _match(e32, e32.stage_inputs(pairs))
    del e32
    return _sets(idx, n)


@pytest.mark.parametrize("name,shape", [("low_margin", "8x1024"), ("mid_margin", "8x1024"), ("default_init", "8x1024"),
                                        ("low_margin", "16x1024"), ("mid_margin", "16x1024"), ("default_init", "16x1024")])
def test_ladder_certified_indices_equal_the_oracle(name, shape):
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family(name)
    pairs, cal_pairs, B, K = _pairs(shape)
    refs = _refs(name, shape)
    want32 = _f32_indices(sd, th, pairs, B, K)
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_certify_ladder(True)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    assert cal["eps_mid"] is not None and cal["eps_mid"] > 0.0, cal
    inp = eng.stage_inputs(pairs)
    eng.set_certify("flag")
    _match(eng, inp)
    flags = eng.uncertain(B)
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    idx_c, n_c, _ = _match(eng, inp)
    st, ls = eng.certify_stats(), eng.certify_ladder_stats()
    m, per = _diff(idx_c, n_c, refs)
    got = _sets(idx_c, n_c)
    row = {"eps": cal["eps"], "eps_mid": cal["eps_mid"], "pairs": B, "flagged_margin": st["flagged_margin"], "flagged_range": st["flagged_fp16_range"],
           "mid_rerun": ls["mid_rerun"], "mid_certified": ls["mid_certified"], "passed_to_f32": ls["passed_to_f32"], "f32_rerun": st["rerun_pairs"],
           "certified_index_mismatches": m}
    _report(f"ladder_{shape}_{name}", row)
    del eng
    assert m == 0, (row, per)
    assert st["flagged_margin"] == ls["mid_rerun"] == ls["mid_certified"] + ls["passed_to_f32"], row
    assert st["rerun_pairs"] == ls["passed_to_f32"] + st["flagged_fp16_range"], row
    for b in range(B):
        if flags[b]:
            assert got[b] == want32[b], b       # a re-run pair -- certified on the middle level or exact f32 -- has the f32 context's indices
    if name == "mid_margin":
        assert ls["passed_to_f32"] < st["flagged_margin"], row


# ---------------------------------------------------------------------------------------------------------------- 5. off is unchanged
def test_ladder_off_is_bitwise_the_plain_certificate():
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family("mid_margin")
    pairs, cal_pairs, B, K = _pairs("4x512")
    res = []
    for variant in ("never", "on_then_off"):
        eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
        if variant == "on_then_off":
            eng.set_certify_ladder(True)
            eng.set_certify_ladder(False)
        cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
        eng.set_certify("rerun")
        eng.certify_stats(reset=True)
        idx, n, score = _match(eng, eng.stage_inputs(pairs))
        res.append((cal["eps"], idx, n, score, eng.certify_stats(), eng.certify_ladder_stats()))
        del eng
    a, b = res
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    assert a[4] == b[4], (a[4], b[4])
    assert a[5]["mid_rerun"] == b[5]["mid_rerun"] == 0


# ---------------------------------------------------------------------------------------------------------------- 6. deferred, streams, range
def test_ladder_deferred_sub_batch_streams_and_a_tripped_group():
    from gisnav_amd.engine import PoseEngine
    _threads()
    sd, _, th = _family("mid_margin")
    pairs = [make_pair(7400 + i, n_q=512 - 9 * i, n_r=500) for i in range(8)]
    cal = [make_pair(7460 + i, n_q=500, n_r=490) for i in range(8)]
    eng = PoseEngine(0, max_batch=8, max_kpts=512, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_certify_ladder(True)
    eng.calibrate_certify(eng.stage_inputs(cal), safety=SAFETY)
    inp = eng.stage_inputs(pairs)
    eng.set_substreams(2)
    eng.set_certify("rerun")
    want = {k: v.clone() for k, v in eng.estimate(inp, K_MATRIX).items()}
    torch.cuda.synchronize()
    # deferred (mode 3): call n is resolved when call n + 1 is queued; two output sets, then flush
    eng.set_certify("deferred")
    outs = [eng.estimate(inp, K_MATRIX), None]
    outs[1] = eng.estimate(inp, K_MATRIX)
    eng.flush()
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o["n_match"], want["n_match"]) and torch.equal(o["ok"], want["ok"])
        assert torch.equal(o["R"], want["R"]) and torch.equal(o["t"], want["t"])
    eng.set_certify("rerun")
    # group 1's guard word raised: its pairs are flagged 2 and go straight to exact f32, never through the middle level
    assert eng.lib.gn_debug_set_variant(eng.ctx, 25, 2) == 0
    eng.certify_stats(reset=True)
    got = eng.estimate(inp, K_MATRIX)
    torch.cuda.synchronize()
    st, ls = eng.certify_stats(), eng.certify_ladder_stats()
    eng.lib.gn_debug_set_variant(eng.ctx, 25, 0)
    eng.set_substreams(1)
    assert st["flagged_fp16_range"] == 4, st
    assert ls["mid_rerun"] == st["flagged_margin"] <= 4, (st, ls)
    assert st["rerun_pairs"] == ls["passed_to_f32"] + 4, (st, ls)
    assert torch.equal(got["n_match"], want["n_match"]) and torch.equal(got["ok"], want["ok"])
    del eng


# ---------------------------------------------------------------------------------------------------------------- 7. weight reload
def test_ladder_weight_reload_sends_flagged_pairs_straight_to_f32():
    from gisnav_amd.engine import PoseEngine
    sd, _, th = _family("mid_margin")
    pairs, cal_pairs, B, K = _pairs("4x512")
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=sd, filter_threshold=th)
    eng.set_certify_ladder(True)
    cal = eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    assert cal["eps_mid"] is not None
    eng.load_state_dict(sd)
    assert eng.certify_ladder_stats()["eps_mid"] is None
    eng.set_certify("rerun", eps=cal["eps"])
    eng.certify_stats(reset=True)
    inp = eng.stage_inputs(pairs)
    _match(eng, inp)
    st, ls = eng.certify_stats(), eng.certify_ladder_stats()
    assert st["flagged_margin"] > 0, st
    assert ls["mid_rerun"] == 0 and st["rerun_pairs"] == st["flagged_margin"] + st["flagged_fp16_range"], (st, ls)
    eng.calibrate_certify(eng.stage_inputs(cal_pairs), safety=SAFETY)
    eng.certify_stats(reset=True)
    _match(eng, inp)
    assert eng.certify_ladder_stats()["mid_rerun"] == eng.certify_stats()["flagged_margin"]
    del eng

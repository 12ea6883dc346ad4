"""PnP beside the next call's matcher (sub-stream mode) and the fused head of the call.

In sub-stream mode every group hands its PnP to the context's PnP stream and goes on with the next call; under the deferred certificate the flags of a
call are recorded behind the match head, not behind PnP, and a re-run waits for the pending PnP of its call before it writes.  None of that may change
a bit of any output:

  * headline configuration (32 x 1024, two sub-batch streams, set_certify("deferred"), automatic block-tail level, two alternating output sets): six
    consecutive estimate() calls over three distinct staged batches, then flush().  R, t, n_match, n_inliers and ok of EVERY call -- read one call
    later, when the contract says they are final, and after the flush for the last one -- are bitwise what the same engine returns for the same
    batches on one stream under set_certify("rerun").  Margin-built weights (nothing flagged) and the mid-margin family of test_gpu_round6.py (some
    pairs flagged and re-run in exact f32: a re-run that raced the pending PnP of its call would leave that PnP's pose in the outputs);
  * a call of ONE pair takes the single-stream path on the caller's stream, in the whole workspaces.  Right behind a deferred grouped call,
    without a flush (PoseEngine.estimate_bucketed's remainder bucket), it must order itself behind that call's groups and PnP: both calls bitwise
    equal to their synchronous results, three times over;
  * k_prep's own hm16 descriptor rows and rot4 table equal, bit for bit, what k_split_hm16 and k_rot_table make of its f32 outputs (developer knob 48:
    0 = the two-launch form), at 1024 keypoints and at a ragged size.
"""
import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu
HEADLINE = "f16x2_f16_attn"
MID_MARGIN = dict(ffn_out_std=1.2e-3, final_scale=12.0, matchability_bias=2.0, matchability_std=0.05)      # tests/test_gpu_round6.py
FAMILIES = {"margin_built": (lambda: synthetic_state_dict(0), 0.5), "mid_margin": (lambda: synthetic_state_dict(0, **MID_MARGIN), 0.01)}
KEYS = ("R", "t", "n_match", "n_inliers", "ok")


@pytest.mark.parametrize("name", ["margin_built", "mid_margin"])
def test_six_pipelined_calls_equal_the_one_stream_synchronous_results_bitwise(name):
    from gisnav_amd.engine import PoseEngine
    make, th = FAMILIES[name]
    B, K = 32, 1024
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=make(), filter_threshold=th)
    eng.set_ffn_products("auto")
    eng.calibrate_certify(eng.stage_inputs([make_pair(9460 + i, n_q=1024, n_r=1000) for i in range(16)]), safety=4.0)
    inps = [eng.stage_inputs([make_pair(9000 + B * j + i, n_q=1024 - 7 * (i % 5), n_r=1024 - 11 * (i % 3)) for i in range(B)]) for j in range(3)]
    eng.set_substreams(1)
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    want = [{k: v.clone() for k, v in eng.estimate(inps[j], K_MATRIX).items()} for j in range(3)]
    torch.cuda.synchronize()
    sync_stats = eng.certify_stats(reset=True)
    eng.set_substreams(2)
    eng.set_certify("deferred")
    outs = [eng.alloc_outputs(B), eng.alloc_outputs(B)]
    got = []
    for i in range(6):
        eng.estimate(inps[i % 3], K_MATRIX, out=outs[i % 2])
        if i > 0:       # call i - 1 is final now, in stream order: copy it before call i + 1 writes that set again
            got.append({k: v.clone() for k, v in outs[(i - 1) % 2].items()})
    eng.flush()
    got.append({k: v.clone() for k, v in outs[5 % 2].items()})
    torch.cuda.synchronize()
    st = eng.certify_stats()
    eng.set_certify("off")
    eng.set_substreams(1)
    del eng
    bad = [(i, k) for i in range(6) for k in KEYS if not torch.equal(got[i][k], want[i % 3][k])]
    print(name, "rerun pairs", st["rerun_pairs"], "of", st["pairs"], "| synchronous", sync_stats["rerun_pairs"], "of", sync_stats["pairs"], "| differing (call, output):", bad)
    assert not bad, bad
    assert st["calls"] == 6 and st["pairs"] == 6 * B, st
    assert int(sum(int(w["ok"].sum()) for w in want)) > 0
    if name == "margin_built":
        assert st["rerun_pairs"] == 0 and sync_stats["rerun_pairs"] == 0, (st, sync_stats)
    else:
        assert st["rerun_pairs"] > 0 and sync_stats["rerun_pairs"] > 0, (st, sync_stats)


def test_a_one_pair_call_right_behind_a_deferred_grouped_call_is_ordered_behind_it():
    from gisnav_amd.engine import PoseEngine
    B, K = 32, 1024
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=synthetic_state_dict(0), filter_threshold=0.5)
    eng.set_ffn_products("auto")
    eng.calibrate_certify(eng.stage_inputs([make_pair(9460 + i, n_q=1024, n_r=1000) for i in range(16)]), safety=4.0)
    big = [eng.stage_inputs([make_pair(9300 + B * j + i, n_q=1024 - 7 * (i % 5), n_r=1024 - 11 * (i % 3)) for i in range(B)]) for j in range(3)]
    one = [eng.stage_inputs([make_pair(9400 + j, n_q=1024 - 5 * j, n_r=1017)]) for j in range(3)]
    eng.set_substreams(1)
    eng.set_certify("rerun")
    eng.certify_stats(reset=True)
    want_big = [{k: v.clone() for k, v in eng.estimate(x, K_MATRIX).items()} for x in big]
    want_one = [{k: v.clone() for k, v in eng.estimate(x, K_MATRIX).items()} for x in one]
    torch.cuda.synchronize()
    sync_stats = eng.certify_stats(reset=True)
    eng.set_substreams(2)
    eng.set_certify("deferred")
    out_big = [eng.alloc_outputs(B) for _ in range(3)]
    out_one = [eng.alloc_outputs(1) for _ in range(3)]
    for j in range(3):                  # grouped call, one-pair call, no flush in between (nor before the next grouped call)
        eng.estimate(big[j], K_MATRIX, out=out_big[j])
        eng.estimate(one[j], K_MATRIX, out=out_one[j])
    eng.flush()
    torch.cuda.synchronize()
    eng.set_certify("off")
    eng.set_substreams(1)
    del eng
    bad = [("big", j, k) for j in range(3) for k in KEYS if not torch.equal(out_big[j][k], want_big[j][k])]
    bad += [("one", j, k) for j in range(3) for k in KEYS if not torch.equal(out_one[j][k], want_one[j][k])]
    print("synchronous rerun pairs", sync_stats["rerun_pairs"], "of", sync_stats["pairs"], "| differing (call, index, output):", bad)
    assert sync_stats["rerun_pairs"] == 0, sync_stats       # (nothing flagged: the one-pair path of the deferred mode has no re-run of its own)
    assert not bad, bad
    assert sum(int(w["n_match"].sum()) for w in want_one) > 0 and sum(int(w["ok"].sum()) for w in want_big) > 0


@pytest.mark.parametrize("shape", ["1024", "ragged"])
def test_prep_writes_the_hm16_rows_and_the_rotary_table_of_the_two_launch_form(shape):
    from gisnav_amd.engine import PoseEngine
    B, K = 4, 1024
    eng = PoseEngine(0, max_batch=B, max_kpts=K, precision=HEADLINE, state_dict=synthetic_state_dict(0))
    if shape == "1024":
        pairs = [make_pair(9700 + i, n_q=1024, n_r=1024) for i in range(B)]
    else:
        pairs = [make_pair(9700 + i, n_q=1024 - 131 * i - 3, n_r=701 - 97 * i) for i in range(B)]
    inp = eng.stage_inputs(pairs)
    other = eng.stage_inputs([make_pair(9800 + i, n_q=900, n_r=1024) for i in range(B)])
    T = B * 2 * K

    def run(fused, x):
        assert eng.lib.gn_debug_set_variant(eng.ctx, 48, 1 if fused else 0) == 0
        eng.match(x["desc_q"], x["kpt_q"], x["n_q"], x["desc_r"], x["kpt_r"], x["n_r"])
        torch.cuda.synchronize()
        return eng.debug_read("desc_p", T * 128, np.uint32).copy(), eng.debug_read("rot4", T * 64, np.uint32).copy()

    run(True, other)                   # (every buffer holds another batch's values before each form runs)
    desc_two, rot_two = run(False, inp)
    run(False, other)
    desc_one, rot_one = run(True, inp)
    del eng
    assert desc_two.size == T * 128 and rot_two.size == T * 64
    assert desc_two.any() and rot_two.any()
    nd, nr = int((desc_one != desc_two).sum()), int((rot_one != rot_two).sum())
    print(shape, "differing words: desc_p", nd, "rot4", nr)
    assert nd == 0 and nr == 0, (nd, nr)

"""GPU tests (-m gpu): a developer knob belongs to the context it is set on (include/gisnav_amd.h, conventions: nothing the launch paths consult
is process-wide).

Each case builds two contexts of one kind in one process, runs B on its defaults, sets a knob on A ONLY, runs A, and runs B again: A's launch table
shows the forced kernel, B's second run shows the kernels of its first and returns its bits.  No knob is restored at the end -- both contexts die with
the test, and no other context ever saw the knob.

Shapes: the smallest at which each choice exists.  One pair of 256 keypoints: the exact-f32 GEMMs run on 64-row tiles (grids of at most 8
workgroups of 128 x 128, against the threshold of 320), the exact-f32 attention on k_attn_f32_ks (2 slots), and the f16x2 block tail on the
small-grid kernels unless a workgroup shape is forced.  LoFTR: 136 x 200, the image of test_loftr_conv_tilings_are_bitwise_equal.
"""
import numpy as np
import pytest
import torch

from gisnav_amd.synthetic import make_pair

pytestmark = pytest.mark.gpu
GEMM64 = ("k_gemm_f32_m64", "k_gemm_f32_r64")


def _engines(precision, sd):
    from gisnav_amd.engine import PoseEngine
    return [PoseEngine(0, max_batch=1, max_kpts=256, precision=precision, state_dict=sd) for _ in range(2)]


def _run(eng, args):
    """(launch-table kernel names, (idx, score, n) on the host) of one matcher call"""
    eng.set_kernel_timing(200)
    out = tuple(t.cpu().numpy().copy() for t in eng.match(*args))
    torch.cuda.synchronize()
    names = [r["name"] for r in eng.kernel_table()]
    eng.set_kernel_timing(0)
    return names, out


def _args(eng):
    inp = eng.stage_inputs([make_pair(9300, n_q=256, n_r=256)])
    return inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"]


def _same_bits(a, b):
    k = int(a[2][0])                   # (entries behind the match count are not written)
    return np.array_equal(a[2], b[2]) and np.array_equal(a[0][0, :k], b[0][0, :k]) and np.array_equal(a[1][0, :k].view(np.uint32), b[1][0, :k].view(np.uint32))


def _has(names, *prefixes):
    return any(nm.startswith(prefixes) for nm in names)


def _plain_attn_f32(names):
    return any(nm.startswith("k_attn_f32") and not nm.startswith("k_attn_f32_ks") for nm in names)


def test_exact_f32_gemm_and_attention_knobs_stay_on_their_context(state_dict_np):
    a, b = _engines("f32", state_dict_np)
    args_a, args_b = _args(a), _args(b)
    names0, out0 = _run(b, args_b)
    assert _has(names0, *GEMM64) and not _has(names0, "k_gemm_f32_v3") and _has(names0, "k_attn_f32_ks") and not _plain_attn_f32(names0), names0
    assert int(out0[2][0]) > 10

    assert a.lib.gn_debug_set_variant(a.ctx, 41, 0) == 0             # A: never the 64-row tiles
    names_a, _ = _run(a, args_a)
    names_b, out_b = _run(b, args_b)
    assert _has(names_a, "k_gemm_f32_v3") and not _has(names_a, *GEMM64), names_a
    assert not _has(names_b, "k_gemm_f32_v3") and names_b == names0, names_b
    assert _same_bits(out_b, out0)

    assert a.lib.gn_debug_set_variant(a.ctx, 43, 1) == 0             # A: never the key-split attention
    names_a, _ = _run(a, args_a)
    names_b, out_b = _run(b, args_b)
    assert _plain_attn_f32(names_a) and not _has(names_a, "k_attn_f32_ks"), names_a
    assert _has(names_b, "k_attn_f32_ks") and not _plain_attn_f32(names_b) and names_b == names0, names_b
    assert _same_bits(out_b, out0)


def test_block_tail_shape_knob_stays_on_its_context(state_dict_np):
    """Knob 14 = 64 (a shape test_gpu_round4 forces): the 64-token workgroups of k_ffn_fused<., ., ., 2> instead of the automatic choice at one pair."""
    a, b = _engines("f16x2_f16_attn", state_dict_np)
    args_a, args_b = _args(a), _args(b)
    tail = lambda names: [nm for nm in names if nm.startswith(("k_ffn", "k_skinny_h", "k_skinny_out"))]      # noqa: E731
    forced = lambda names: [nm for nm in names if nm.startswith("k_ffn_fused<") and nm.rstrip(">").endswith(" 2")]      # noqa: E731
    names0, out0 = _run(b, args_b)
    assert tail(names0) and not forced(names0), names0
    assert int(out0[2][0]) > 10

    assert a.lib.gn_debug_set_variant(a.ctx, 14, 64) == 0
    names_a, _ = _run(a, args_a)
    names_b, out_b = _run(b, args_b)
    assert forced(names_a) and forced(names_a) == tail(names_a), names_a
    assert not forced(names_b) and names_b == names0, names_b
    assert _same_bits(out_b, out0)


def test_loftr_conv_knob_needs_no_matcher_context_and_stays_on_its_own(state_dict_np):
    """Knob 42 (bits 8 and up: the overhead term of lf_conv's cost model, here large enough for the tallest tiles everywhere) on LoFTR matcher A only:
    A and B both return the default's bits (the tile height never changes one), B's before and after; a matcher context refuses the knob."""
    from gisnav_amd.engine import PoseEngine
    from gisnav_amd.loftr import LoFTR
    from oracle import loftr as lf
    sd = lf.synthetic_state_dict(0)
    h, w = 136, 200
    i0, i1 = lf.synthetic_pair(2, h, w)
    data = {"image0": i0[None, None].cuda(), "image1": i1[None, None].cuda()}
    a, b = (LoFTR(state_dict=sd).to("cuda:0").eval() for _ in range(2))
    run = lambda m: {k: v.cpu() for k, v in m(data, with_ids=True).items()}      # noqa: E731
    out0 = run(b)
    assert out0["keypoints0"].shape[0] > 100
    a.debug_variant(42, 100000 << 8)
    out_a, out_b = run(a), run(b)
    for k in out0:
        assert torch.equal(out0[k], out_a[k]) and torch.equal(out0[k], out_b[k]), k
    eng = PoseEngine(0, max_batch=1, max_kpts=256, precision="f32", state_dict=state_dict_np)
    assert eng.lib.gn_debug_set_variant(eng.ctx, 42, 100000 << 8) != 0
    assert a.lib.gn_loftr_debug_set_variant(a._ctx, 43, 1) != 0              # (a matcher knob: nothing of LoFTR's reads it)

"""The pairs of the padded-size tests (tests/test_padded_sizes_host.py checks them on the CPU, tests/test_gpu_fp64_padded_sizes.py runs them on
the GPU) and their float64 reference, oracle.lightglue_sift.pose_node_match(..., dtype=torch.float64), cached per pair for the process.

The deployed callers never run the matcher at a fixed 512 or 1024 slots a side: PoseNode, estimate_bucketed and estimate_images all call
set_active_kpts(max(n_q, n_r)), any multiple of 128 up to the context's max_kpts.  The sizes here are the ones at which gn_api.hip's dispatch
pairs kernels that no other test pairs:

  * one pair (the node's own call: k_skinny_qkv / k_skinny_h / k_skinny_out and the key-split k_attn_ks on a grid of P / 32, the fused head's
    partial buffers of P / 32 rows) at P = 128 .. 4096, a last tile nearly full on one side and holding a single keypoint on the other;
  * 8 pairs at P = 1152 (144 tiles of 128 tokens: k_qkv, but P % 256 != 0, so k_attn16_v5 reads its packed q | k and V^T buffers);
  * 26 pairs at P = 640 (260 tiles: k_qkv fused into k_ffn128, again feeding k_attn16_v5; k_tile_lists without its item lists);
  * 8 pairs at P = 1024 on a 2048-slot context (128 tiles: k_qkv and k_attn_pw with the small-grid block tail);
  * a one-pair and an eight-pair batch that fit 256 / 512 slots, run at several padded sizes.

Weights are margin-built (synthetic_state_dict(0)), threshold 0.5, as in tests/test_gpu_fp64_parity.py."""
import os

import numpy as np
import torch

from gisnav_amd.synthetic import make_pair
from gisnav_amd.weights import synthetic_state_dict

THRESHOLD = 0.5
LAYERS = (1, 5, 9)
MIN_MATCHES = 15      # gisnav_amd.engine.MIN_MATCHES: what a pose needs

# ---------------------------------------------------------------------------------------------------------------- 1. one pair
SINGLE_SIZES = (128, 384, 640, 1152, 2176, 4096)
# n_q = P - 3 (last tile nearly full), n_r = P - 127 (last tile holds one keypoint); 128: the reference side needs two keypoints to match at all;
# 384: the query side fills the padding exactly; 4096: a short reference side keeps the fp64 run cheap
SINGLE_SIDES = {P: (P - 3, P - 127) for P in SINGLE_SIZES}
SINGLE_SIDES.update({128: (125, 2), 384: (384, 257), 4096: (4093, 200)})


def single_pair(P):
    nq, nr = SINGLE_SIDES[P]
    return make_pair(23000 + P, n_q=nq, n_r=nr)


# ---------------------------------------------------------------------------------------------------------------- 2. groups
def _ragged(seed, count, lo, hi):
    rs = np.random.default_rng(seed)
    return [(int(rs.integers(lo, hi + 1)), int(rs.integers(lo, hi + 1))) for _ in range(count)]


def _pairs(first, sizes):
    return [make_pair(first + i, n_q=q, n_r=r) for i, (q, r) in enumerate(sizes)]


def group_sizes(name):
    if name == "8x1152":
        return [(1149, 1025), (600, 1152)] + _ragged(31, 6, 130, 400)
    if name == "26x640":      # two pairs near 640, a side of 129 and a side of 127, the rest 130 .. 300
        return [(640, 633), (611, 640), (129, 300), (280, 127)] + _ragged(32, 22, 130, 300)
    if name == "8x1024of2048":
        return [(1024, 1000), (897, 1024)] + _ragged(33, 6, 300, 900)
    if name == "pad_1":
        return [(250, 240)]
    if name == "pad_8":       # eight pairs of <= 500 keypoints
        return [(500, 471), (433, 500)] + _ragged(34, 6, 260, 480)
    raise KeyError(name)


# name -> (first pair index, max_batch, max_kpts of the context, the active sizes it runs at)
GROUPS = {"8x1152": (24000, 8, 1152, (1152,)), "26x640": (24100, 26, 640, (640,)), "8x1024of2048": (24200, 8, 2048, (1024,)),
          "pad_1": (24300, 1, 4096, (256, 4096)), "pad_8": (24400, 8, 2048, (512, 1024, 2048))}
_PAIRS = {}


def group(name):
    """(pairs, max_batch, max_kpts, active sizes); the pairs are built once per process."""
    first, B, K, active = GROUPS[name]
    if name not in _PAIRS:
        _PAIRS[name] = _pairs(first, group_sizes(name))
    return _PAIRS[name], B, K, active


def tiles(n_pairs, P):
    """128-token tiles of a call: what gn_api.hip's thresholds (k_qkv from 128, k_ffn128 from 256) count."""
    return 2 * n_pairs * P // 128


# ---------------------------------------------------------------------------------------------------------------- the fp64 reference
_REF = {}
_SD = {}


def state_dict():
    if not _SD:
        _SD.update(synthetic_state_dict(0))
    return _SD


def ref64(p):
    """fp64 run of one pair, cached: the residual stream of both sides after the layers of LAYERS, best / runner-up score of every row, match list."""
    k = (len(p.kp_q), len(p.kp_r), hash(p.kp_q.tobytes()), hash(p.desc_r.tobytes()))
    if k not in _REF:
        from oracle import lightglue_sift as lg
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
        tsd = {n: torch.from_numpy(v) for n, v in state_dict().items()}
        tq = torch.from_numpy
        taps = {}
        _, _, _, idx = lg.pose_node_match(tsd, tq(p.kp_q), tq(p.desc_q), tq(p.size_q), tq(p.angle_q), tq(p.kp_r), tq(p.desc_r), tq(p.size_r),
                                          tq(p.angle_r), taps=taps, filter_threshold=THRESHOLD, dtype=torch.float64)
        nq, nr = len(p.kp_q), len(p.kp_r)
        P = taps["scores"][0, :nq, :nr].numpy()
        top2 = -np.partition(-P, 1, axis=1)[:, :2]
        _REF[k] = {"layers": {l: (taps[f"layer{l - 1}_0"][0].numpy(), taps[f"layer{l - 1}_1"][0].numpy()) for l in LAYERS},
                   "best": top2[:, 0].copy(), "second": top2[:, 1].copy(), "idx": idx.numpy()}
    return _REF[k]

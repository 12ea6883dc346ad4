"""CPU restatement of LightGlue's point pruning (width_confidence > 0, early exit off), composed from the oracle's blocks.

Restated from the public kornia 0.7.2 / cvg LightGlue `_forward`; kornia is not importable in this project's environment, so parity with it is
UNPINNED, like the rest of the oracle.  Both sides start with ind = arange(n), prune = ones(n).  After the cross block of layer i < n_layers - 1
each side whose CURRENT count is > min_kpts keeps the rows with sigmoid(matchability_i(x)) > 1 - width_confidence (ascending order, torch.where)
and prune[ind] += 1.  After the head the matches go back through ind: matches over the original query keypoints, a pruned query has none.

This project's own rule, mirrored here: a side left with NO keypoint makes the pair report no match (kornia would raise in a max over an empty
dimension).  A side left with one keypoint runs on, as in kornia, whose fewer-than-two rule (LightGlueMatcher._no_match) looks at the input counts.

Used by tests/test_width_pruning_host.py and tests/test_gpu_width_pruning.py.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import lightglue_sift as lg

Tensor = torch.Tensor
DEFAULT_MIN_KPTS = 1536      # recalled from kornia's pruning_keypoint_thresholds (CUDA with flash; 1024 without), not verifiable here


def tau(width_confidence: float) -> float:
    """The threshold on z: sigmoid(z) > 1 - wc  <=>  z > logit(1 - wc)."""
    return math.log((1.0 - width_confidence) / width_confidence)


def sift_inputs(p, dtype=torch.float32):
    """The tensors lightglue_forward takes for a synthetic.Pair, prepared as pose_node_match + lightglue_matcher_forward prepare them."""
    tq = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    kp_q, desc_q, size_q, angle_q, kp_r, desc_r, size_r, angle_r = (tq(a) for a in (p.kp_q, p.desc_q, p.size_q, p.angle_q, p.kp_r, p.desc_r, p.size_r, p.angle_r))
    laf_q = lg.laf_from_center_scale_ori(kp_q.unsqueeze(0), size_q[None, :, None, None], angle_q[None, :, None])
    laf_r = lg.laf_from_center_scale_ori(kp_r.unsqueeze(0), size_r[None, :, None, None], angle_r[None, :, None])
    dq, dr = lg.rootsift(desc_q).unsqueeze(0), lg.rootsift(desc_r).unsqueeze(0)
    kp1, kp2 = lg.get_laf_center(laf_q), lg.get_laf_center(laf_r)
    size1, size2 = kp1.max(dim=1)[0].reshape(-1, 2), kp2.max(dim=1)[0].reshape(-1, 2)

    def ori(laf):
        o = lg.get_laf_orientation(laf).reshape(1, -1) * math.pi / 180.0
        return torch.where(o < 0, o + 2.0 * math.pi, o)
    return dict(kpts0=kp1, kpts1=kp2, desc0=dq, desc1=dr, scales0=lg.get_laf_scale(laf_q).reshape(1, -1), scales1=lg.get_laf_scale(laf_r).reshape(1, -1),
                oris0=ori(laf_q), oris1=ori(laf_r), size0=size1, size1=size2)


def sp_inputs(p, dtype=torch.float32):
    """The tensors oracle.lightglue_superpoint.lightglue_forward takes for a 256-d pair (image size = keypoint extent)."""
    tq = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    k0, k1 = tq(p.kp_q)[None], tq(p.kp_r)[None]
    return dict(kpts0=k0, kpts1=k1, desc0=tq(p.desc_q)[None], desc1=tq(p.desc_r)[None],
                size0=k0.max(dim=1)[0].reshape(-1, 2), size1=k1.max(dim=1)[0].reshape(-1, 2))


def _tsd(sd, dtype) -> Dict[str, Tensor]:
    return {k: torch.as_tensor(v).to(dtype) for k, v in lg.canonical_state_dict(sd).items()}


def _matchability(sd, i, x):
    p = f"log_assignment.{i}"
    return F.linear(x, sd[p + ".matchability.weight"], sd[p + ".matchability.bias"])[0, :, 0]


def forward(sd, inp: dict, feature: str = "sift", n_layers: int = lg.N_LAYERS, filter_threshold: float = lg.FILTER_THRESHOLD,
            width_confidence: float = -1.0, min_kpts: int = DEFAULT_MIN_KPTS, dtype=torch.float32, forced_keep: Optional[dict] = None,
            stop_before_layer: Optional[int] = None) -> dict:
    """One pair.  inp: sift_inputs / sp_inputs (converted to dtype here).  forced_keep: {(layer, side): array of ORIGINAL indices to keep}
    -- replays someone else's decisions instead of deciding (a side / layer that is not in it is decided here).
    Returns matches0 (n0,) int64 over the original query keypoints (-1 = none), scores0 (n0,), idx (K, 2), score (K,), prune0 / prune1 (int32),
    z = {(layer, side): z of the rows present at that layer (only where the side was up for pruning)}, present = {(layer, side): their original
    indices}, xmax = {(layer, side): max |x| over those rows}, kept = {(layer, side): original indices after the layer}, counts = [(n0, n1) after every layer], x = the residual rows (d0, d1) when
    stop_before_layer cuts the run in front of that layer's self block (then nothing else but z / present / kept is returned)."""
    sd = _tsd(sd, dtype)
    inp = {k: v.to(dtype) for k, v in inp.items()}
    with torch.inference_mode():
        k0 = lg.normalize_keypoints(inp["kpts0"], inp["size0"]).clone()
        k1 = lg.normalize_keypoints(inp["kpts1"], inp["size1"]).clone()
        if feature == "sift":
            k0 = torch.cat([k0, inp["scales0"].unsqueeze(-1), inp["oris0"].unsqueeze(-1)], -1)
            k1 = torch.cat([k1, inp["scales1"].unsqueeze(-1), inp["oris1"].unsqueeze(-1)], -1)
            d0 = F.linear(inp["desc0"].contiguous(), sd["input_proj.weight"], sd["input_proj.bias"])
            d1 = F.linear(inp["desc1"].contiguous(), sd["input_proj.weight"], sd["input_proj.bias"])
        else:
            d0, d1 = inp["desc0"].contiguous(), inp["desc1"].contiguous()
        e0, e1 = lg.posenc(sd["posenc.Wr.weight"], k0), lg.posenc(sd["posenc.Wr.weight"], k1)
        n0, n1 = d0.shape[1], d1.shape[1]
        ind = [torch.arange(n0), torch.arange(n1)]
        prune = [torch.ones(n0, dtype=torch.int32), torch.ones(n1, dtype=torch.int32)]
        on = width_confidence > 0
        if not on:
            prune = [torch.full((n0,), n_layers, dtype=torch.int32), torch.full((n1,), n_layers, dtype=torch.int32)]
        thr = torch.tensor(1.0 - width_confidence, dtype=dtype) if on else None
        z_out, present, kept, counts, xmax = {}, {}, {}, [], {}
        d, e = [d0, d1], [e0, e1]
        for i in range(n_layers):
            if stop_before_layer is not None and i == stop_before_layer:
                return dict(x=(d[0], d[1]), ind=ind, z=z_out, present=present, kept=kept, counts=counts, xmax=xmax)
            d[0] = lg.self_block(sd, i, d[0], e[0])
            d[1] = lg.self_block(sd, i, d[1], e[1])
            d[0], d[1] = lg.cross_block(sd, i, d[0], d[1])
            if on and i < n_layers - 1:
                for s in (0, 1):
                    if d[s].shape[1] <= min_kpts:
                        continue
                    z = _matchability(sd, i, d[s])
                    z_out[(i, s)], present[(i, s)] = z.clone(), ind[s].clone()
                    xmax[(i, s)] = float(d[s].abs().max())
                    if forced_keep is not None and (i, s) in forced_keep:
                        keep = torch.isin(ind[s], torch.as_tensor(np.asarray(forced_keep[(i, s)], np.int64)))
                    else:
                        keep = torch.sigmoid(z) > thr
                    w = torch.where(keep)[0]
                    d[s], e[s], ind[s] = d[s].index_select(1, w), e[s].index_select(-2, w), ind[s][w]
                    prune[s][ind[s]] += 1
                    kept[(i, s)] = ind[s].clone()
            counts.append((d[0].shape[1], d[1].shape[1]))
            if min(counts[-1]) == 0:      # this project's rule: the pair reports no match (the oracle's blocks cannot run on an empty side)
                counts += [counts[-1]] * (n_layers - 1 - i)
                break
        m0_full = torch.full((n0,), -1, dtype=torch.int64)
        s0_full = torch.zeros(n0, dtype=dtype)
        if min(n0, n1) >= 2 and d[0].shape[1] >= 1 and d[1].shape[1] >= 1:      # _no_match on the INPUT counts; an emptied side: this project's rule
            scores, _ = lg.match_assignment(sd, n_layers - 1, d[0], d[1])
            m0, _, ms0, _ = lg.filter_matches(scores, filter_threshold)
            m0, ms0 = m0[0], ms0[0]
            valid = m0 > -1
            m0_full[ind[0][valid]] = ind[1][m0[valid]]
            s0_full[ind[0]] = ms0
        v = m0_full > -1
        q = torch.where(v)[0]
        return dict(matches0=m0_full, scores0=s0_full, idx=torch.stack([q, m0_full[v]], -1).numpy(), score=s0_full[v].numpy(),
                    prune0=prune[0].numpy(), prune1=prune[1].numpy(), z=z_out, present=present, kept=kept, counts=counts, xmax=xmax)


def kept_from_prune(prune: np.ndarray, n: int, counts_before: List[int], min_kpts: int, n_layers: int) -> dict:
    """{layer: original indices kept after that layer} of ONE side from its final prune vector: the side was up for pruning at layer i exactly
    when its count in front of it exceeded min_kpts, and a keypoint that survived j such layers has prune = 1 + j."""
    out, fired = {}, 0
    for i in range(n_layers - 1):
        if counts_before[i] > min_kpts:
            fired += 1
            out[i] = np.where(prune[:n] >= 1 + fired)[0]
    return out


def build_pruning_weights(pairs_inputs: List[dict], feature: str = "sift", seed: int = 0, prune_layers=(1, 4, 6), width_confidence: float = 0.9,
                          min_kpts: int = 100, weight_scale: float = 1.0, keep_range=(0.4, 0.9), n_layers: int = lg.N_LAYERS, base: Optional[dict] = None):
    """synthetic_state_dict(seed) (margin-built) with matchability biases set for a pruning test: +30 (nothing pruned) on every layer but
    `prune_layers`; on those, layer by layer in fp64 over the given pairs, the bias puts the threshold into the WIDEST gap of the pooled z of the
    rows present at that layer whose cut keeps between keep_range (a pair, or {layer: pair}) of them.  weight_scale multiplies those layers' matchability.weight (the gaps
    grow with it; the relative margin of the 16-bit modes does not).  Returns (state dict, {layer: half-gap in z})."""
    from gisnav_amd.weights import synthetic_state_dict
    sd = dict(base) if base is not None else synthetic_state_dict(seed, feature=feature)
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    for i in range(n_layers):
        sd[f"log_assignment.{i}.matchability.bias"] = np.array([30.0], np.float32)
    t = tau(width_confidence)
    half_gaps = {}
    for li in prune_layers:
        wk = f"log_assignment.{li}.matchability.weight"
        sd[wk] = (sd[wk].astype(np.float64) * weight_scale).astype(np.float32)
        us = []
        for inp in pairs_inputs:      # layer li's bias is still +30 here: the run records its z (every row kept) and stops behind it
            r = forward(sd, inp, feature, n_layers, width_confidence=width_confidence, min_kpts=min_kpts, dtype=torch.float64, stop_before_layer=li + 1)
            us += [r["z"][(li, s)].numpy() - 30.0 for s in (0, 1) if (li, s) in r["z"]]
        if not us:      # no side is still above min_kpts at this layer: nothing to place (the bias stays +30)
            half_gaps[li] = None
            continue
        u = np.sort(np.concatenate(us))
        n = len(u)
        kr = keep_range[li] if isinstance(keep_range, dict) else keep_range
        gaps = u[1:] - u[:-1]                        # a cut in gap j keeps the n - 1 - j values above it
        keep_frac = (n - 1 - np.arange(n - 1)) / n
        ok = (keep_frac >= kr[0]) & (keep_frac <= kr[1])
        j = int(np.argmax(np.where(ok, gaps, -1.0)))
        mid = 0.5 * (u[j] + u[j + 1])
        sd[f"log_assignment.{li}.matchability.bias"] = np.array([t - mid], np.float32)
        half_gaps[li] = 0.5 * float(gaps[j])
    return sd, half_gaps


def settled(sd, inp, feature, width_confidence, min_kpts, margin_of, n_layers: int = lg.N_LAYERS, filter_threshold: float = lg.FILTER_THRESHOLD):
    """The 'decisions are settled' precondition of one pair: the fp64 and the f32 run agree on every decision, and every |z - tau| of BOTH runs
    exceeds margin_of(layer, side, r64) -- a callable, so that a mode's margin can depend on the layer's weights and the fp64 rows.
    Returns (r64, r32, smallest |z - tau| / margin over all decisions)."""
    r64 = forward(sd, inp, feature, n_layers, filter_threshold, width_confidence, min_kpts, torch.float64)
    r32 = forward(sd, inp, feature, n_layers, filter_threshold, width_confidence, min_kpts, torch.float32)
    assert r64["kept"].keys() == r32["kept"].keys(), (sorted(r64["kept"]), sorted(r32["kept"]))
    t, worst = tau(width_confidence), math.inf
    for key in r64["kept"]:
        assert np.array_equal(r64["kept"][key].numpy(), r32["kept"][key].numpy()), key
        m = margin_of(key[0], key[1], r64)
        for r in (r64, r32):
            worst = min(worst, float((r["z"][key].double() - t).abs().min()) / m)
    assert np.array_equal(r64["prune0"], r32["prune0"]) and np.array_equal(r64["prune1"], r32["prune1"])
    return r64, r32, worst

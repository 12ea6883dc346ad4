"""Cost of the pose covariance: gn_estimate_cov against gn_estimate of the same build, interleaved in one process and timed
by HIP events, at B = 32 (one stream, and two sub-batch streams as the bench runs) and B = 1, 1024 keypoints per side, headline precision; and
the PnP stage alone (k_pnp_hyp + k_pnp_refine [+ k_pnp_cov]) on the same batch's correspondences.  Medians over 24 alternating repetitions.

    python tools/cov_cost.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gisnav_amd.engine import PoseEngine
from gisnav_amd.synthetic import K_MATRIX, make_pair
from gisnav_amd.weights import synthetic_state_dict

sd = synthetic_state_dict(0)
res = {}
for B, sub in ((32, 1), (32, 2), (1, 1)):
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=sd)
    inp = eng.stage_inputs([make_pair(100 + i, n_q=1024, n_r=1024) for i in range(B)])
    eng.set_substreams(sub)
    outs = {False: eng.alloc_outputs(B), True: eng.alloc_outputs(B, covariance=True)}
    inner = 10 if B == 32 else 50
    for cov in (False, True, False, True):
        for _ in range(5):
            eng.estimate(inp, K_MATRIX, out=outs[cov], covariance=cov)
    eng.flush(); torch.cuda.synchronize()
    ms = {False: [], True: []}
    for rep in range(24):
        for cov in ((False, True) if rep % 2 == 0 else (True, False)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                eng.estimate(inp, K_MATRIX, out=outs[cov], covariance=cov)
            eng.flush()
            e1.record(); e1.synchronize()
            ms[cov].append(e0.elapsed_time(e1) / inner)
    # the PnP stage alone (k_pnp_hyp + k_pnp_refine [+ k_pnp_cov]) on the staged points of this batch
    idx, _, nm = eng.match(inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    mkp, obj = eng.gather_points(inp["kpt_q"], inp["kpt_r"], idx, nm, inp["dem"])
    pnp = {False: [], True: []}
    for rep in range(24):
        for cov in ((False, True) if rep % 2 == 0 else (True, False)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                eng.pnp_ransac(obj, mkp, nm, K_MATRIX, min_pts=15, covariance=cov)
            e1.record(); e1.synchronize()
            pnp[cov].append(e0.elapsed_time(e1) / 20)
    eng.set_substreams(1)
    key = f"B{B}_sub{sub}"
    med = lambda v: float(np.median(v))
    res[key] = dict(estimate_ms=med(ms[False]), estimate_cov_ms=med(ms[True]), estimate_spread_ms=float(np.percentile(ms[False], 90) - np.percentile(ms[False], 10)),
                    delta_pct=100.0 * (med(ms[True]) / med(ms[False]) - 1.0), pnp_ms=med(pnp[False]), pnp_cov_ms=med(pnp[True]),
                    inliers=[int(x) for x in eng.estimate(inp, K_MATRIX)["n_inliers"].cpu()[:4]])
    print(key, json.dumps(res[key]), flush=True)
    del eng
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)

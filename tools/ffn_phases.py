"""Developer tool: per-phase shader-clock stamps of k_ffn_fused (knob 12 = 8), from the last FFN launch of one bench-sized call."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gisnav_amd.engine import PoseEngine  # noqa: E402
from gisnav_amd.synthetic import make_pair  # noqa: E402
from gisnav_amd.weights import synthetic_state_dict  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
if len(sys.argv) > 2:
    # ffn_phases.py <batch> <products>: the stamps of k_ffn128<8, true, false, ., products>, products = 3 / 2 / 1 (one-tile composed form of the headline mode; tools/ffn128_ab.py
    # prints the same table for three products next to its A/B) from the first block-tail launch of a bench-sized call
    products = int(sys.argv[2])
    eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_f16_attn", state_dict=synthetic_state_dict(0))
    eng.set_ffn_products(products)
    eng.lib.gn_debug_set_variant(eng.ctx, 31, 3)      # one workgroup per tile
    inp = eng.stage_inputs([make_pair(i) for i in range(B)])
    args = (inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
    eng.match(*args)
    assert eng.lib.gn_debug_set_variant(eng.ctx, 12, 8) == 0
    eng.lib.gn_debug_set_variant(eng.ctx, 4, 5)       # stop after the first FFN launch
    eng.set_kernel_timing(400)
    eng.match(*args)
    torch.cuda.synchronize()
    ran = [r["name"] for r in eng.kernel_table() if r["name"].startswith("k_ffn128")]
    eng.set_kernel_timing(0)
    nb = B * 2 * 1024 // 128
    order = [0, 1, 2, 3, 10, 4, 5, 6, 7, 8, 9]      # stamp 10 sits between the two halves of GEMM 1
    ts = eng.debug_read("sim", nb * 4 * 12 * 2, np.uint32).view(np.int64).reshape(nb, 4, 12)[:, :, order]
    d = np.diff(ts, axis=2).astype(np.float64)
    print(f"k_ffn128<8, true, false, ., {products}> ({', '.join(ran)}), batch {B}: phase cycles (s_memtime), median over workgroups of wave 0 / of the max over waves:")
    for k, nm in enumerate(["prologue", "gemm0", "publish msg", "gemm1 msg", "gemm1 x", "ln stats", "gelu q0", "gemm2+gelu", "yt store", "epilogue"]):
        print(f"  {nm:12s} {np.median(d[:, 0, k]):9.0f}   {np.median(d[:, :, k].max(axis=1)):9.0f}")
    print("  workgroup total, median", np.median(ts[:, 0, -1] - ts[:, 0, 0]))
    sys.exit(0)
eng = PoseEngine(0, max_batch=B, max_kpts=1024, precision="f16x2_bf16_attn", state_dict=synthetic_state_dict(0))
inp = eng.stage_inputs([make_pair(i) for i in range(B)])
args = (inp["desc_q"], inp["kpt_q"], inp["n_q"], inp["desc_r"], inp["kpt_r"], inp["n_r"])
eng.match(*args)
eng.lib.gn_debug_set_variant(eng.ctx, 12, 8)
eng.lib.gn_debug_set_variant(eng.ctx, 4, 5)       # stop after the first FFN launch: the stamps in `sim` are not overwritten by the head
eng.match(*args)
torch.cuda.synchronize()
TOK = 64 if B * 2 * 1024 // 64 >= 256 else 32          # the launcher's shape rule (gn_ffn.hip)
nb = B * 2 * 1024 // TOK
ts = eng.debug_read("sim", nb * 8 * 8 * 2, np.uint32).view(np.int64).reshape(nb, 8, 8)
d = np.diff(ts, axis=2).astype(np.float64)
names = ["prologue", "gemm1", "ln+gelu", "publish", "gemm2", "barrier", "epilogue"]
print("phase cycles, median over blocks (wave 0) / max over waves:")
for k, n in enumerate(names):
    print(f"  {n:9s} {np.median(d[:, 0, k]):9.0f}   {np.median(d[:, :, k].max(axis=1)):9.0f}")
tot = ts[:, 0, 7] - ts[:, 0, 0]
print("block total median", np.median(tot), " kernel span (max end - min start)", ts[:, :, 7].max() - ts[:, :, 0].min())
starts = np.sort(ts[:, 0, 0] - ts[:, :, 0].min())
print("block start times (cycles) quartiles:", starts[[0, nb // 4, nb // 2, 3 * nb // 4, -1]])

import os, sys, time, torch
sys.path.insert(0, "/root/repo")
from gisnav_amd import loftr_synthetic as olf
from gisnav_amd.loftr import LoFTR
dev = torch.device("cuda", 0)
m = LoFTR(state_dict=olf.synthetic_state_dict(0), fine=True, graph=True, arithmetic="exact_f32").to(dev).eval()
i0, i1 = olf.synthetic_pair(1, 480, 640)
data = {"image0": i0.to(dev), "image1": i1.to(dev)}
for thr in (0, 170, 320, 0, 170, 320):
    m2 = LoFTR(state_dict=olf.synthetic_state_dict(0), fine=True, graph=True, arithmetic="exact_f32").to(dev).eval()
    m2.debug_variant(41, thr)        # (the knob of this LoFTR context alone)
    for _ in range(3): out = m2(data)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): out = m2(data)
    torch.cuda.synchronize()
    print(f"m64 threshold {thr}: {(time.perf_counter() - t0) / 10 * 1e3:.3f} ms per pair, matches {int(out['keypoints0'].shape[0])}", flush=True)
    del m2

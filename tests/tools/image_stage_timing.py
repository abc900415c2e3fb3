"""Developer tool: what the image stage (trained exposure + alpha mask + random background) costs the train step.
   python3 tests/tools/image_stage_timing.py [cfg] [steps]
Times train_iteration at a BASELINE size (default c3) in three forms, each on a fresh trainer in the deferred depth-limited
mode bench.py runs:
  plain  - no exposure, no mask, fixed background
  stage  - exposure + alpha masks + random background on the fast step (gs_image_stage_*, ExposureAdam)
  torch  - exposure with torch's optimizer: the form every exposure run took before the stage (torch matmul in the render,
           no manual backward, no deferred depth limits)
and prints one line per form and one JSON line with the three ms / step."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from gsplat_amd.io import camera_alpha_mask  # noqa: E402
from gsplat_amd.trainer import TrainOptions  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
dev = torch.device("cuda", 0)


def run(form):
    tr, scene, cams, gts = bench.build_workload(cfg, dev, 0, 1)
    tr.depth_limit = "deferred"
    opt = TrainOptions(random_background=(form == "stage"), seed=0)
    if form in ("stage", "torch"):
        tr.model.enable_exposure(len(cams))
        if form == "torch":
            tr.model.exposure_optimizer = torch.optim.Adam([tr.model.exposure])
    if form == "stage":
        g = torch.Generator().manual_seed(1)
        H, W = gts[0].shape[-2:]
        tr.alpha_masks = []
        for k in range(len(cams)):
            rgba = torch.ones((4, H, W))
            rgba[3] = (torch.rand((H, W), generator=g) > 0.05).float()
            tr.alpha_masks.append(camera_alpha_mask(rgba, True, k % 8 == 0, False).to(dev))
    it = 1
    for _ in range(len(cams) + 10):   # every camera visited (limits exist), then some
        tr.train_iteration(it, opt)
        it += 1
    tr.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_iteration(it, opt)
        it += 1
    tr.sync()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    path = tr.last["path"]
    del tr
    torch.cuda.empty_cache()
    print("%-6s %s: %.4f ms / iteration (last step form: %s)" % (form, cfg, ms, path), flush=True)
    return ms


out = {form: round(run(form), 4) for form in ("plain", "stage", "torch")}
print(json.dumps(dict(cfg=cfg, steps=steps, ms_per_iteration=out)))

"""Developer tool: of the Gaussians a depth-limited, region-binned C3 view accepts (tiles_touched > 0), how many does the
BACKWARD blend reach - own a list entry in front of their tile's deepest last contributor (GeomView.reached, written by the
forward blend)?  The others have all-zero gradient rows: the share the reached split (GsStepState.reached_split) takes off
the backward's tail.  Gaussian counts and counts of 256-row blocks (the model's row order) that hold at least one.
   python tests/tools/reached_probe.py [c3]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from gsplat_amd import hip_backend, synthetic  # noqa: E402
from test_gpu_raster_parity import forward_state  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
dev = torch.device("cuda", 0)
tr, scene, cams, gts = bench.build_workload(cfg, dev, 0, 1)
if tr.model.spatial_order:   # (the rows as the train step holds them)
    scene = synthetic.spatially_ordered(scene)
be = hip_backend()
be.tile_cull, be.binning, be.depth_limit_on = True, "region", True
be._cam_cache.clear()
P = scene["means3D"].shape[0]
NB = (P + 255) // 256


def blocks(mask):
    pad = torch.zeros((NB * 256,), dtype=torch.bool)
    pad[:P] = mask
    return int(pad.view(NB, 256).any(dim=1).sum())


tot = dict(accepted=0, listed=0, reached=0)
print("%s: P %d, %d blocks of 256 rows, rows in %s order" % (cfg, P, NB, "spatial" if tr.model.spatial_order else "generated"))
for ci in (0, 5, 11, 17):
    cam = cams[ci]
    forward_state(be, scene, cam, dev, torch.zeros(3), False)               # first visit: measures the stop depths
    buf = {}
    cut = forward_state(be, scene, cam, dev, torch.zeros(3), False, buffers=buf)   # second visit: depth-limited lists
    accepted = cut["tiles_touched"] > 0
    listed = torch.zeros((P,), dtype=torch.bool)
    listed[cut["point_list"].long()] = True
    reached = be.export_reached(P, buf["geom"]).cpu().bool()
    assert bool((listed | ~reached).all()) and bool((accepted | ~listed).all())
    n = {k: int(v.sum()) for k, v in (("accepted", accepted), ("listed", listed), ("reached", reached))}
    print("camera %2d: R %d | accepted %d (%d blocks) | with list entries %d (%d blocks) | reached %d (%d blocks) | "
          "accepted but unreached: %.1f %% of the accepted" % (
              ci, cut["num_rendered"], n["accepted"], blocks(accepted), n["listed"], blocks(listed), n["reached"], blocks(reached),
              100.0 * (n["accepted"] - n["reached"]) / max(n["accepted"], 1)))
    for k in tot:
        tot[k] += n[k]
print("all: accepted %d, with list entries %d, reached %d -> unreached %.1f %% of the accepted (%.1f %% of them never listed)" % (
    tot["accepted"], tot["listed"], tot["reached"], 100.0 * (tot["accepted"] - tot["reached"]) / tot["accepted"],
    100.0 * (tot["accepted"] - tot["listed"]) / tot["accepted"]))

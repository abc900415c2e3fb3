"""Developer tool: one plain FSGS iteration (one training camera, one optimizer step) in two forms, same process, same GPU:
    unfused   TrainerFSGS with FUSED_STEP off: activation kernel, gs_forward_render_fsgs, FsgsCriterion's node,
              gs_backward_fsgs (six gradient tensors written, scaled by the confidence of ones as the reference does),
              gs_activations_bwd, gs_densify_stats, gs_adam_step
    fused     the same trainer class with the fused step: raw rows into gs_forward_render_fsgs, the same criterion node,
              gs_backward_step_fsgs (backward, activation backward, statistics and Adam in the per-Gaussian kernel)
Both forms are the SAME commit and the SAME call (TrainerFSGS.step); pseudo-view and densifying iterations take the un-fused
form in either and are not timed.
Sizes: trained_like(60 000) at 504 x 378 - 504 x 378 is the `images_8` size of the LLFF scenes FSGS trains on; the Gaussian
count is an ASSUMPTION, not taken from a trained model - and the benchmark's trained_like(1 000 000) at 1920 x 1080.
The two forms alternate after warm-up; device-synchronised wall time over STEPS steps each (host work included: that is what
a training loop pays), cameras in rotation; the whole comparison REPS times to show the spread.  Nothing is asserted.
Writes to stdout and to profiles/fsgs_step_timing.txt (or the path given)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (("trained_like(60 000), 504 x 378 (LLFF images_8; the Gaussian count is an assumption)", 60_000, 504, 378),
         ("trained_like(1 000 000), 1920 x 1080 (the benchmark's size)", 1_000_000, 1920, 1080))
STEPS, WARMUP, REPS, CAMERAS = 120, 12, 3, 4


def trainers(torch, P, W, H):
    """-> (unfused, fused): two TrainerFSGS over copies of one scene"""
    import fsgs_loss
    from gsplat_amd import hip_backend, synthetic
    from gsplat_amd.trainer import GaussianModelLite, TrainerFSGS, camera_to
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    sc = synthetic.trained_like(P, seed=0, knn=lambda x: distCUDA2(x.to(dev)).cpu(), sh_degree=3)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:CAMERAS]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g).to(dev) for _ in cams]
    midas = [(1000.0 - 100.0 * (2.0 + 6.0 * torch.rand((H, W), generator=g))).to(dev) for _ in cams]
    out = []
    for fused in (False, True):
        model = GaussianModelLite(sc, dev, api=hip_backend().api)
        tr = TrainerFSGS(model, cams, gts, midas, fsgs_loss.criterion(), torch.zeros(3, device=dev))
        tr.FUSED_STEP = fused
        out.append(tr)
    return out


def per_step_ms(torch, tr, first, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(first, first + steps):
        tr.step(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main(path):
    import torch
    assert torch.cuda.is_available(), "fsgs_step_timing needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("one FSGS iteration (TrainerFSGS.step) per step, ms: device-synchronised wall time over %d steps of each form, %d cameras "
        "in rotation, forms alternating after %d warm-up steps; %d repetitions of the whole comparison" % (STEPS, CAMERAS, WARMUP, REPS))
    say("unfused = gs_backward_fsgs + gs_activations_bwd + gs_densify_stats + gs_adam_step; fused = gs_backward_step_fsgs on raw rows")
    for what, P, W, H in SIZES:
        say(what)
        unfused, fused = trainers(torch, P, W, H)
        for tr in (unfused, fused):
            per_step_ms(torch, tr, 0, WARMUP)
        k = WARMUP
        reps = []
        for _ in range(REPS):
            u = per_step_ms(torch, unfused, k, STEPS)
            f = per_step_ms(torch, fused, k, STEPS)
            k += STEPS
            reps.append((u, f))
        assert unfused.last["path"] == "unfused" and fused.last["path"] == "fused"
        us, fs = [r[0] for r in reps], [r[1] for r in reps]
        say("  unfused %s   fused %s   unfused / fused: %s"
            % (" ".join("%.3f" % x for x in us), " ".join("%.3f" % x for x in fs), " ".join("%.2f" % (a / b) for a, b in reps)))
        say("  spread (max - min) unfused %.3f, fused %.3f; smallest gap between the forms %.3f"
            % (max(us) - min(us), max(fs) - min(fs), min(us) - max(fs)))
        del unfused, fused
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fsgs_step_timing.txt"))

"""Developer tool: one DNGaussian iteration (TrainerDNG.train_iteration) with all three legs active - hard depth leg, soft depth
leg, photometric leg - and the depth legs in two forms, same process, same GPU, same trainer:
    unfused   depth_pass -> depth regulariser -> autograd backward (gs_depth_backward writes dL_dmeans3D / dL_dmeans2D or
              dL_dopacity) -> torch's sigmoid backward (soft leg) -> FlatAdam.step on one segment (gs_adam_step)
    fused     gs_depth_forward -> the same loss node, differentiated for its two image cotangents -> gs_depth_backward_step
              (blend backward, then ONE per-Gaussian kernel that steps the row it has differentiated)
The two forms give the same bits (tests/test_gpu_dng_trainer.py), so ONE trainer alternates between them: DngOptions with
fused_depth_legs on and off, in windows of WINDOW iterations, REPS repetitions, after a warm-up of both.  Device-synchronised
wall time per iteration (host work included: that is what a training loop pays).  Then each leg alone - the leg's call only,
on one camera, the two forms of a depth leg alternating window by window in the same way (the leg keeps stepping the model, so
consecutive windows drift).
Sizes: trained_like(60 000) at 504 x 378 - the `images_8` size of the LLFF scenes DNGaussian trains on; the Gaussian count is
an ASSUMPTION, not taken from a trained model - and trained_like(1 000 000) at 1920 x 1080.
No densification, prune or clean runs inside the windows.  Nothing is asserted.
Writes to stdout and to profiles/dng_step_timing.txt (or the path given)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (("trained_like(60 000), 504 x 378 (LLFF images_8; the Gaussian count is an assumption)", 60_000, 504, 378),
         ("trained_like(1 000 000), 1920 x 1080", 1_000_000, 1920, 1080))
WINDOW, WARMUP, REPS, CAMERAS = 100, 10, 3, 4


def trainer(torch, P, W, H):
    from gsplat_amd import hip_backend, synthetic
    from gsplat_amd.trainer import GaussianModelLite, TrainerDNG, camera_to
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    sc = synthetic.trained_like(P, seed=0, knn=lambda x: distCUDA2(x.to(dev)).cpu(), sh_degree=0)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:CAMERAS]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g).to(dev) for _ in cams]
    mono = [(255.0 * torch.rand((H, W), generator=g)).to(dev) for _ in cams]
    model = GaussianModelLite(sc, dev, api=hip_backend().api)
    model.active_sh_degree = 0
    return TrainerDNG(model, cams, gts, mono)


def options(fused, **kw):
    from gsplat_amd.trainer import DngOptions
    o = dict(iterations=10 ** 9, hard_depth_start=0, soft_depth_start=0, smooth_start=0, densify_until_iter=0,
             near_prune_start=10 ** 9, clean_iterations=[], fused_depth_legs=fused)
    o.update(kw)
    return DngOptions(**o)


def window_ms(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main(path):
    import torch
    assert torch.cuda.is_available(), "dng_step_timing needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("one DNGaussian iteration (TrainerDNG.train_iteration: hard leg, soft leg, photometric leg), ms per iteration: "
        "device-synchronised wall time over windows of %d iterations, %d cameras, fused and un-fused depth legs alternating in one "
        "trainer after %d warm-up iterations of each; %d repetitions" % (WINDOW, CAMERAS, WARMUP, REPS))
    for what, P, W, H in SIZES:
        say(what)
        tr = trainer(torch, P, W, H)
        assert tr.fused_legs_available()
        it = [0]

        def iteration(opt):
            it[0] += 1
            r = tr.train_iteration(it[0], opt)
            if opt.hard_depth_start == 0:
                assert r["path"]["hard"] == r["path"]["soft"] == ("fused" if opt.fused_depth_legs else "unfused")
        forms = {name: options(name == "fused") for name in ("unfused", "fused")}
        for name in forms:
            window_ms(torch, lambda: iteration(forms[name]), WARMUP)
        reps = []
        for _ in range(REPS):
            reps.append(tuple(window_ms(torch, lambda: iteration(forms[name]), WINDOW) for name in ("unfused", "fused")))
        us, fs = [r[0] for r in reps], [r[1] for r in reps]
        say("  whole iteration   unfused %s   fused %s   unfused / fused: %s"
            % (" ".join("%.3f" % x for x in us), " ".join("%.3f" % x for x in fs), " ".join("%.2f" % (a / b) for a, b in reps)))
        say("  spread (max - min) unfused %.3f, fused %.3f; fastest unfused window - slowest fused window = %.3f"
            % (max(us) - min(us), max(fs) - min(fs), min(us) - max(fs)))
        # each leg alone
        tr.draw_cameras(0)
        for leg, kind in (("hard leg", "means"), ("soft leg", "opacity")):
            fns = {name: (lambda opt=forms[name]: tr._depth_leg(it[0] % CAMERAS, kind, 11, 13, 0.1, opt, True)) for name in forms}
            for name in forms:
                window_ms(torch, fns[name], WARMUP)
            row = [tuple(window_ms(torch, fns[name], WINDOW) for name in ("unfused", "fused")) for _ in range(REPS)]
            say("  %-16s  unfused %s   fused %s   fastest unfused - slowest fused = %.3f"
                % (leg, " ".join("%.3f" % r[0] for r in row), " ".join("%.3f" % r[1] for r in row),
                   min(r[0] for r in row) - max(r[1] for r in row)))
        photo = options(True, hard_depth_start=10 ** 9, soft_depth_start=10 ** 9)
        window_ms(torch, lambda: iteration(photo), WARMUP)
        say("  photometric leg   %s" % " ".join("%.3f" % window_ms(torch, lambda: iteration(photo), WINDOW) for _ in range(REPS)))
        del tr
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dng_step_timing.txt"))

"""Developer tool: one DNGaussian DTU iteration (TrainerDNGDTU.train_iteration) with every leg active - hard, soft (the gate held
open), alpha, photometric - in three forms, same process, same GPU:
    boolean   TrainerDNGDTU's un-fused loop with torch's boolean-index statements in place of the new calls, as train_dtu.py has
              them: every iteration forms the mask with the 49-step loop, zeroes the image and fills the mono target
              (`x[mask] = x[~mask].mean()`), both depth legs fill their depth image the same way, the alpha leg is
              `(alpha[mask] ** 2).mean()` (tests/dtu_reference.py's statements on device tensors)
    unfused   TrainerDNGDTU: mask, zeroed image and filled target formed once, gs_masked_fill_* and gs_alpha_penalty_* in the legs
    fused     the same with DngDtuOptions.fused_depth_legs: all three opacity / means legs through depth_pass.depth_leg_step
Device-synchronised wall time per iteration over windows of WINDOW iterations, REPS repetitions, the forms taking turns window
by window after a warm-up of each (each form has its own trainer from the same scene; they keep stepping, so windows drift).
Host stalls per iteration: the calls torch itself reports as synchronising (torch.cuda.set_sync_debug_mode("warn")) over one
iteration of each form, and how many of them are aten::nonzero (torch.profiler): every one of them blocks the host until the
device has caught up.
Then the colour rules alone at the same Gaussian count: gs_dng_colour_rule against the boolean-index statements.
Size: trained_like(60 000) at 400 x 300, the DTU training resolution of scripts/run_dtu.sh; the Gaussian count is an ASSUMPTION,
not taken from a trained model.  No densification or clean runs inside the windows.  Nothing is asserted.
Writes to stdout and to profiles/dtu_step_timing.txt (or the path given)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

P, W, H = 60_000, 400, 300
WINDOW, WARMUP, REPS, CAMERAS = 50, 10, 3, 4
FORMS = ("boolean", "unfused", "fused")


def scene(torch):
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import camera_to
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    sc = synthetic.trained_like(P, seed=0, knn=lambda x: distCUDA2(x.to(dev)).cpu(), sh_degree=0)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:CAMERAS]]
    g = torch.Generator().manual_seed(5)
    gts = []
    for _ in cams:     # an object in front of a dark background: a bright disc, dark outside it
        gt = 0.2 + 0.8 * torch.rand((3, H, W), generator=g)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        outside = ((yy - H / 2) / (0.42 * H)) ** 2 + ((xx - W / 2) / (0.42 * W)) ** 2 > 1
        gts.append(torch.where(outside[None], gt * 0.05, gt).to(dev))
    mono = [(255.0 * torch.rand((H, W), generator=g)).to(dev) for _ in cams]
    return sc, cams, gts, mono


def options(fused):
    from gsplat_amd.trainer import DngDtuOptions
    return DngDtuOptions(iterations=10 ** 9, hard_depth_start=0, soft_depth_start=0, soft_gate=float("inf"), densify_until_iter=0,
                         clean_iterations=[], fused_depth_legs=fused)


def trainer(torch, form, inputs):
    import dtu_reference as dr
    from gsplat_amd import hip_backend
    from gsplat_amd.trainer import GaussianModelLite, TrainerDNGDTU
    sc, cams, gts, mono = inputs
    model = GaussianModelLite(sc, torch.device("cuda:0"), api=hip_backend().api)
    model.active_sh_degree = 0
    kw = {}
    if form == "boolean":
        kw = dict(background_mask=lambda gt, thr, run=50: dr.background_mask(gt.clone(), thr, run),
                  masked_fill=dr.masked_mean_fill, alpha_penalty=dr.alpha_penalty,
                  colour_rule=lambda c, s, o, black=None, white=None, value=None: dr.colour_rules(c, s, o, black, white, value))
    tr = TrainerDNGDTU(model, cams, [g.clone() for g in gts], mono, **kw)
    tr.raw_gts, tr.raw_mono = gts, [255.0 - m for m in mono]
    return tr


def window_ms(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main(path):
    import torch

    import dtu_reference as dr
    assert torch.cuda.is_available(), "dtu_step_timing needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("one DNGaussian DTU iteration (TrainerDNGDTU.train_iteration: hard, soft, alpha and photometric legs), ms per iteration: "
        "device-synchronised wall time over windows of %d iterations, %d cameras, the three forms taking turns after %d warm-up "
        "iterations of each; %d repetitions" % (WINDOW, CAMERAS, WARMUP, REPS))
    say("trained_like(%d), %d x %d (the DTU training size; the Gaussian count is an assumption)" % (P, W, H))
    inputs = scene(torch)
    trs = {f: trainer(torch, f, inputs) for f in FORMS}
    opts = {f: options(f == "fused") for f in FORMS}
    its = {f: 0 for f in FORMS}
    say("  masked pixels per camera: %s of %d" % (" ".join(str(int(m.sum())) for m in trs["unfused"].bg_masks), W * H))

    def iteration(f):
        tr, opt = trs[f], opts[f]
        its[f] += 1
        if f == "boolean":      # what train_dtu.py:84-94, :102-104 and :135-137 do every iteration
            ci = tr._stack[-1] if tr._stack else 0
            mask, _ = dr.background_mask(tr.raw_gts[ci].clone(), opt.bg_threshold, opt.bg_run)
            for _ in range(2):
                dr.masked_mean_fill(tr.raw_mono[ci].reshape(mask.shape), mask)
        r = tr.train_iteration(its[f], opt)
        want = "fused" if f == "fused" else "unfused"
        assert r["path"] == dict(hard=want, soft=want, alpha=want), r["path"]
    for f in FORMS:
        window_ms(torch, lambda: iteration(f), WARMUP)
    reps = [tuple(window_ms(torch, lambda: iteration(f), WINDOW) for f in FORMS) for _ in range(REPS)]
    for k, f in enumerate(FORMS):
        v = [r[k] for r in reps]
        say("  whole iteration  %-8s %s   spread (max - min) %.3f" % (f, " ".join("%.3f" % x for x in v), max(v) - min(v)))
    b, u, fz = ([r[k] for r in reps] for k in range(3))
    say("  fastest boolean window - slowest unfused window = %.3f; fastest unfused window - slowest fused window = %.3f"
        % (min(b) - max(u), min(u) - max(fz)))
    import warnings
    from torch.profiler import ProfilerActivity, profile
    for f in FORMS:
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            iteration(f)
        torch.cuda.synchronize()
        nz = sum(e.count for e in prof.key_averages() if e.key == "aten::nonzero")
        # torch's own count of calls that made the host wait for the device (scalar reads of CPU tensors are not among them)
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                iteration(f)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        stalls = sum(1 for w in caught if "synchroniz" in str(w.message).lower())
        say("  host stalls per iteration  %-8s %d synchronising calls (torch.cuda.set_sync_debug_mode), of them aten::nonzero %d"
            % (f, stalls, nz))
    # the colour rules alone
    from gsplat_amd import dng_dtu
    g = torch.Generator().manual_seed(9)
    colour = torch.rand((P, 3), generator=g).cuda()
    stat, opa = torch.rand((P, 1), generator=g).cuda(), torch.randn((P, 1), generator=g).cuda()
    black, white, value = (20 / 255, 10, True), (240 / 255, 2, True), dr.reset_value(0.1)
    fns = dict(kernel=lambda: dng_dtu.colour_rule(colour, stat, opa, black, white, value),
               boolean=lambda: dr.colour_rules(colour, stat, opa, black, white, value))
    for name, fn in fns.items():
        window_ms(torch, fn, WARMUP)
        say("  colour rules, P = %d  %-8s %s" % (P, name, " ".join("%.4f" % window_ms(torch, fn, WINDOW) for _ in range(REPS))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dtu_step_timing.txt"))

"""Developer tool: one DNGaussian Blender iteration of each loop - TrainerDNGBlender.train_iteration (hard, soft and photometric
legs) and TrainerDNGBlenderSH.train_iteration (hard and photometric legs) - with the depth legs running on EVERY iteration
(depth_leg_interval = 1; train_blender.py runs them on every tenth, so a real run spends a tenth of the legs' share), in three
forms, same process, same GPU:
    boolean   the un-fused loop with torch's boolean-index statements in place of the new calls, as train_blender.py has them:
              every iteration forms the mask (`gt.min(0) > 254/255`) and every leg the target (`depth_mono[bg_mask] = 0`)
              (tests/blender_reference.py's statements on device tensors)
    unfused   the trainers as they are: mask and target formed once per camera by gs_blender_target
    fused     the same with DngBlenderOptions.fused_depth_legs: the legs through depth_pass.depth_leg_step
Device-synchronised wall time per iteration over windows of WINDOW iterations, REPS repetitions, the forms taking turns window
by window after a warm-up of each (each form has its own trainer from the same scene; they keep stepping, so windows drift).
Host stalls per iteration: the calls torch itself reports as synchronising (torch.cuda.set_sync_debug_mode("warn")) over one
iteration of each form, and how many aten::nonzero it ran (torch.profiler).
Then the white rule alone at the same Gaussian count: gs_dng_white_rule and gs_dng_white_rule_sh (degree 3, packed rows) against
the boolean-index statements, the SH one with its Python eval_sh, over windows of RULE_WINDOW calls.  Every call starts from the
same opacity rows (a device copy in front of it, in all four forms - its own cost is printed), since a rule applied over and
over drives the rows it fires on to -inf.
Size: trained_like(60 000) at 400 x 400 (`-r 2` of NeRF-synthetic's 800 x 800, scripts/run_blender.sh); the Gaussian count is an
ASSUMPTION, not taken from a trained model.  No densification, clean or reset runs inside the windows.  Nothing is asserted.
Writes to stdout and to profiles/blender_step_timing.txt (or the path given)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

P, W, H = 60_000, 400, 400
WINDOW, WARMUP, REPS, CAMERAS = 200, 20, 5, 4
RULE_WINDOW = 2000   # calls per white-rule window: tens of milliseconds, not one, so that clock and launch overhead do not decide
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
    for _ in cams:     # an object in front of a white background: white outside a disc
        gt = 0.1 + 0.8 * torch.rand((3, H, W), generator=g)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        outside = ((yy - H / 2) / (0.42 * H)) ** 2 + ((xx - W / 2) / (0.42 * W)) ** 2 > 1
        gts.append(torch.where(outside[None], torch.ones_like(gt), gt).to(dev))
    mono = [(255.0 * torch.rand((H, W), generator=g)).to(dev) for _ in cams]
    return sc, cams, gts, mono


def options(fused, sh):
    from gsplat_amd.trainer import DngBlenderOptions
    return DngBlenderOptions(iterations=10 ** 9, hard_depth_start=0, soft_depth_start=0, densify_until_iter=10 ** 9,
                             densify_from_iter=10 ** 9, opacity_reset_interval=10 ** 9, sh_increase_interval=10 ** 9,
                             depth_leg_interval=1, clean_iterations=[], fused_depth_legs=fused, use_sh=sh)


def boolean_mask(gt, thr, mono=None):
    import blender_reference as br
    mask = br.background_mask(gt, thr)
    return mask if mono is None else (mask, br.depth_target(mono, mask))


def trainer(torch, form, sh, inputs):
    from gsplat_amd import hip_backend
    from gsplat_amd.trainer import GaussianModelLite, TrainerDNGBlender, TrainerDNGBlenderSH
    sc, cams, gts, mono = inputs
    model = GaussianModelLite(sc, torch.device("cuda:0"), api=hip_backend().api)
    model.active_sh_degree = 0
    kw = dict(background_mask=boolean_mask) if form == "boolean" else {}
    tr = (TrainerDNGBlenderSH if sh else TrainerDNGBlender)(model, cams, gts, mono, **kw)
    tr.raw_mono = mono
    return tr


def window_ms(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main(path):
    import warnings

    import torch
    from torch.profiler import ProfilerActivity, profile

    import blender_reference as br
    assert torch.cuda.is_available(), "blender_step_timing needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("one DNGaussian Blender iteration with the depth legs on every iteration (the script: every tenth), ms per iteration: "
        "device-synchronised wall time over windows of %d iterations, %d cameras, the three forms taking turns after %d warm-up "
        "iterations of each; %d repetitions" % (WINDOW, CAMERAS, WARMUP, REPS))
    say("trained_like(%d), %d x %d (-r 2 of 800 x 800; the Gaussian count is an assumption)" % (P, W, H))
    inputs = scene(torch)
    for sh in (False, True):
        loop = "SH loop (TrainerDNGBlenderSH: hard, photometric)" if sh else "neural loop (TrainerDNGBlender: hard, soft, photometric)"
        say(loop)
        trs = {f: trainer(torch, f, sh, inputs) for f in FORMS}
        opts = {f: options(f == "fused", sh) for f in FORMS}
        its = {f: 0 for f in FORMS}
        n_legs = 1 if sh else 2
        if not sh:
            say("  masked pixels per camera: %s of %d" % (" ".join(str(int(m.sum())) for m in trs["unfused"].bg_masks), W * H))

        def iteration(f):
            tr, opt = trs[f], opts[f]
            its[f] += 1
            if f == "boolean":      # what train_blender.py:87 does every iteration and :96-97 / :123-124 in every leg
                ci = tr._stack[-1] if tr._stack else 0
                mask = br.background_mask(tr.gts[ci], opt.bg_threshold)
                for _ in range(n_legs):
                    br.depth_target(tr.raw_mono[ci], mask)
            r = tr.train_iteration(its[f], opt)
            want = "fused" if f == "fused" else "unfused"
            assert (r["path"] == want) if sh else (r["path"] == dict(hard=want, soft=want)), r["path"]
        for f in FORMS:
            window_ms(torch, lambda: iteration(f), WARMUP)
        reps = [tuple(window_ms(torch, lambda: iteration(f), WINDOW) for f in FORMS) for _ in range(REPS)]
        for k, f in enumerate(FORMS):
            v = [r[k] for r in reps]
            say("  whole iteration  %-8s %s   spread (max - min) %.3f" % (f, " ".join("%.3f" % x for x in v), max(v) - min(v)))
        b, u, fz = ([r[k] for r in reps] for k in range(3))
        say("  fastest boolean window - slowest unfused window = %.3f; fastest unfused window - slowest fused window = %.3f"
            % (min(b) - max(u), min(u) - max(fz)))
        for f in FORMS:
            with profile(activities=[ProfilerActivity.CPU]) as prof:
                iteration(f)
            torch.cuda.synchronize()
            nz = sum(e.count for e in prof.key_averages() if e.key == "aten::nonzero")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    iteration(f)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            stalls = sum(1 for w in caught if "synchroniz" in str(w.message).lower())
            say("  host stalls per iteration  %-8s %d synchronising calls (torch.cuda.set_sync_debug_mode), aten::nonzero calls %d"
                % (f, stalls, nz))
        del trs
    # the white rule alone
    from gsplat_amd import dng_blender
    g = torch.Generator().manual_seed(9)
    colour = (0.9 + 0.1 * torch.rand((P, 3), generator=g)).cuda()
    stat, opa = torch.rand((P, 1), generator=g).cuda(), torch.randn((P, 1), generator=g).cuda()
    xyz, campos = torch.randn((P, 3), generator=g).cuda(), torch.tensor([0.3, -1.7, 2.1]).cuda()
    shs = (torch.randn((P, 16, 3), generator=g) * 0.05).cuda()
    shs[:, 0, :] = 1.7
    thr = 253 / 255
    stat0, opa0 = stat.clone(), opa.clone()

    def fresh(fn):
        def call():
            stat.copy_(stat0)
            opa.copy_(opa0)
            return fn()
        return call
    fns = (("the two copies alone   ", fresh(lambda: None)),
           ("white rule      kernel ", fresh(lambda: dng_blender.white_rule(colour, stat, opa, thr))),
           ("white rule      boolean", fresh(lambda: br.white_rule(colour, stat, opa, thr))),
           ("white rule, SH  kernel ", fresh(lambda: dng_blender.white_rule_sh(xyz, shs, 3, campos, stat, opa, thr))),
           ("white rule, SH  boolean", fresh(lambda: br.white_rule_sh(xyz, shs, 3, campos, stat, opa, thr))))
    say("the white rule alone, ms per call over windows of %d calls (each call behind two device copies that restore its rows)"
        % RULE_WINDOW)
    for name, fn in fns:
        window_ms(torch, fn, WARMUP)
        say("  P = %d  %s %s" % (P, name, " ".join("%.4f" % window_ms(torch, fn, RULE_WINDOW) for _ in range(REPS))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "blender_step_timing.txt"))

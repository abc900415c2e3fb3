"""Developer tool: what DNGaussian's near-camera prune and its densification cost on one MI355X in three forms.  Needs the GPU;
nothing is asserted.  Writes profiles/dng_prune_timing.txt (or the path given with --out) and prints the same lines.

Forms:
  reference  the restatement of the reference (tests/dng_densify_reference.py: Reference) on the device - the mask_near loop of
             train_llff.py:208-213 in torch, boolean indexing of every group's parameter and both moments, torch.optim.Adam
             state re-registered per group: what a user of the reference's model class runs today;
  host       GaussianModelLite's host path (near_camera_mask in one launch, then prune_points; densify_and_prune_dng);
  device     the same with on_device=True (gs_prune_plan / gs_prune_emit / gs_densify_plan_gated + the gather).
Workloads, at 10 000 and 1 000 000 Gaussians, rows as generated and in Morton order (spatial_order):
  prune      a near-camera prune that removes about 1 % of the rows (K = 8 centres; the range is the 1 % quantile of the
             distance to the nearest centre);
  densify    one DNGaussian densification in which every rule fires (clones, splits, rows the gate stops, pruned rows).

Method: a call re-lays the model out, so every call starts from the same state, restored on the device outside the timed span;
wall-clock time of ONE call between two device synchronisations (the calls read counts back, so the host's waits are part of
what they cost); WARMUP calls, then REPS calls per form with the forms alternating; median and spread (max - min).  First the
spread of ONE form measured twice: a difference between two forms counts when it is larger than that."""
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (10_000, 1_000_000)
WARMUP, REPS = 2, 7
K_CENTRES, SHARE = 8, 0.01
EXTENT, MAX_GRAD, MIN_OPACITY, OPA_THRESH = 4.4, 2e-4, 0.005, 0.1

OUT = [None]


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(line + "\n")


def build(torch, api, dev, P, spatial_order):
    """-> (model, restore()): trained_like(P) with moments and statistics from CPU generators; restore() puts the model back."""
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import GaussianModelLite
    from simple_knn._C import distCUDA2
    sc = synthetic.trained_like(P, seed=0, scale_mult=1.5, knn=lambda x: distCUDA2(x.to(dev)).cpu())
    m = GaussianModelLite(sc, dev, api=api, spatial_order=spatial_order)
    g = torch.Generator().manual_seed(1)
    n = m.flat.numel()
    with torch.no_grad():
        m.params["opacity"][::9] = -6.0      # faint rows: the final prune fires
        flat = m.flat.clone()
        ea = (torch.randn(n, generator=g) * 1e-3).to(dev)
        ev = (torch.rand(n, generator=g) * 1e-6).to(dev)
        accum = (torch.rand((P, 1), generator=g) * 6e-4).to(dev)
        denom = torch.randint(0, 3, (P, 1), generator=g).float().to(dev)
        radii = (torch.rand((P,), generator=g) * 50).to(dev)

    def restore():
        with torch.no_grad():
            m._allocate(P)
            m.optimizer.alloc_moments()
            m.flat.copy_(flat)
            m.optimizer.exp_avg.copy_(ea)
            m.optimizer.exp_avg_sq.copy_(ev)
            m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), denom.clone(), radii.clone()
            for p in m.params.values():
                p.grad = None
    restore()
    return m, restore


def measure(torch, forms):
    """{name: (prepare, call)} -> {name: (median, spread, result)} seconds per call; prepare() runs outside the timed span"""
    times = {name: [] for name in forms}
    result = {}
    gc.collect()
    gc.disable()
    try:
        for rep in range(WARMUP + REPS):
            for name, (prepare, call) in forms.items():
                state = prepare()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                result[name] = call(state)
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times[name].append(time.perf_counter() - t0)
    finally:
        gc.enable()
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v), result[k]) for k, v in times.items()}


def report(res, spread):
    ref = res["reference"][0]
    for name, (med, sp, out) in res.items():
        say("    %-10s %9.3f ms (%.3f)   reference / this = %5.2f x   -> %s" % (name, med * 1e3, sp * 1e3, ref / med, out))
    d, h = res["device"][0], res["host"][0]
    say("    host - device = %+.3f ms (same-form spread %.3f ms): the device form %s the host path here"
        % ((h - d) * 1e3, spread * 1e3, "beats" if h - d > spread else "does NOT beat"))


def main():
    import torch
    assert torch.cuda.is_available(), "dng_prune_timing needs the GPU"
    import dng_densify_reference as dg
    from gsplat_amd._lib import hip_api
    from gsplat_amd.dng_reg import near_camera_mask
    out = os.path.join(ROOT, "profiles", "dng_prune_timing.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    sizes = SIZES if "--sizes" not in sys.argv else tuple(int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(","))
    dev = torch.device("cuda:0")
    api = hip_api()
    open(out, "w").close()
    OUT[0] = out
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("ms per call: median (spread = max - min) of %d calls after %d warm-up calls, wall clock between device synchronisations, "
        "forms alternating; every call starts from the same restored model" % (REPS, WARMUP))
    for P in sizes:
        for spatial_order in (False, True):
            m, restore = build(torch, api, dev, P, spatial_order)
            say("P = %d, %s" % (P, "rows in Morton order (spatial_order)" if spatial_order else "rows as generated"))
            xyz = m.params["xyz"].detach()
            g = torch.Generator().manual_seed(2)
            centers = xyz[torch.randint(0, P, (K_CENTRES,), generator=g).to(dev)].clone() + 0.01
            nearest = torch.cdist(xyz, centers).min(dim=1).values
            near = float(nearest.kthvalue(max(int(SHARE * P), 1)).values)

            def model_state():
                restore()
                return m

            def reference_state():
                restore()
                return dg.Reference.of(m)

            def reference_prune(ref):
                mask_near = None
                for c in centers:
                    t = (ref.p["xyz"] - c.repeat(ref.P, 1)).norm(dim=1, keepdim=True) < near
                    mask_near = mask_near + t if mask_near is not None else t
                mask_near = mask_near.squeeze()
                ref.prune_points(mask_near)
                return "P %d" % ref.P

            def model_prune(on_device):
                def call(mm):
                    n = mm.prune_points(near_camera_mask(mm.params["xyz"].detach(), centers, near), on_device=on_device)
                    return "P %d (%d removed)" % (mm.P, n)
                return call

            def reference_densify(ref):
                r = ref.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, OPA_THRESH, None,
                                          generator=torch.Generator().manual_seed(3))
                return "P %d %s" % (ref.P, r)

            def model_densify(on_device):
                def call(mm):
                    r = mm.densify_and_prune_dng(MAX_GRAD, MIN_OPACITY, EXTENT, None, OPA_THRESH, None,
                                                 generator=torch.Generator().manual_seed(3), on_device=on_device)
                    return "P %d %s" % (mm.P, r)
                return call

            same = measure(torch, {"host": (model_state, model_prune(False)), "host again": (model_state, model_prune(False))})
            vals = [v[0] for v in same.values()]
            spread = max(max(vals) - min(vals), max(v[1] for v in same.values()))
            say("  the same form (host prune) measured twice: %.3f and %.3f ms -> same-form spread %.3f ms"
                % (vals[0] * 1e3, vals[1] * 1e3, spread * 1e3))
            say("  near-camera prune, %d centres, range %.4f (about %.1f %% of the rows)" % (K_CENTRES, near, 100 * SHARE))
            report(measure(torch, {"reference": (reference_state, reference_prune), "host": (model_state, model_prune(False)),
                                   "device": (model_state, model_prune(True))}), spread)
            say("  densification, DNGaussian's rule (n_outliers, n_clone, n_split, n_pruned); the split noise is drawn on the CPU "
                "and uploaded inside the timed span in all three forms")
            report(measure(torch, {"reference": (reference_state, reference_densify), "host": (model_state, model_densify(False)),
                                   "device": (model_state, model_densify(True))}), spread)
            del m, restore
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

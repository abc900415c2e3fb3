"""Developer tool: forward + backward of DNGaussian's two depth passes in two forms, same process, same GPU:
    general     the reference composition (tests/depth_pass_reference.py: colours = ones, detaches, constant or own opacity)
                through dgr_dng.GaussianRasterizer - what serves these passes without gsplat_amd.depth_pass
    depth_pass  gsplat_amd.depth_pass (csrc/gs_depth_pass.hip)
Modes: hard (opacity 0.95, gradient to the means) and soft (the scene's opacities, gradient to the opacities).
Sizes: trained_like(60 000) at 504 x 378 - a stand-in for DNGaussian's LLFF runs at 1/8 resolution; the Gaussian count is an
ASSUMPTION, not taken from a trained model - and the benchmark's trained_like(1 000 000) at 1920 x 1080.
The two forms alternate after warm-up; device-synchronised wall time over CALLS calls each (host work included: that is what a
training loop pays); the whole comparison REPS times to show the spread.  Nothing is asserted.
Writes to stdout and to profiles/depth_pass_timing.txt (or the path given).

Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/depth_pass_timing.py --trace
    python tests/tools/depth_pass_timing.py --kernels DIR [FILE to append to]
--trace enqueues TRACE_CALLS calls of each form and mode at the small size and nothing else."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (("trained_like(60 000), 504 x 378 (stand-in for LLFF at 1/8; the count is an assumption)", 60_000, 504, 378),
         ("trained_like(1 000 000), 1920 x 1080 (the benchmark's size)", 1_000_000, 1920, 1080))
CALLS, WARMUP, REPS = 200, 10, 3
TRACE_CALLS = 20
KERNELS = ("depth_fwd_wave_kernel", "depth_bwd_wave_kernel", "depth_point_bwd_kernel", "render_fwd_wave_kernel",
           "render_bwd_wave_kernel", "chain_kernel", "preprocess_bwd_kernel", "preprocess_fwd", "zero_rows_kernel",
           "tile_order_kernel")


def forms(torch, P, W, H):
    """-> {mode: (general, depth_pass)} of callables doing one forward + backward"""
    import depth_pass_reference as dpr
    import dgr_dng
    from gsplat_amd import synthetic
    from gsplat_amd.depth_pass import depth_pass
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    sc = synthetic.trained_like(P, seed=0, knn=lambda x: distCUDA2(x.to(dev)).cpu(), sh_degree=0)
    cam = synthetic.orbit_cameras(W, H)[5]
    means = sc["means3D"].to(dev).requires_grad_(True)
    op = sc["opacities"].to(dev).requires_grad_(True)
    scales, rot = sc["scales"].to(dev), sc["rotations"].to(dev)
    rs = dpr._settings(dgr_dng.GaussianRasterizationSettings, cam, torch.zeros(3), dev, P)
    dd, da = (t.to(dev) for t in dpr.cotangents(H, W, 1))
    rast = dgr_dng.GaussianRasterizer(rs)

    def general(hard):
        # DNGaussian/gaussian_renderer/__init__.py:128-269, line for line
        means.grad = op.grad = None
        m2 = torch.zeros_like(means, requires_grad=True) + 0
        o = torch.ones((P, 1), device=dev) * 0.95 if hard else op
        colors = torch.ones_like(means)
        _, radii, depth, alpha = rast(means3D=means if hard else means.detach(), means2D=m2, opacities=o, shs=None,
                                      colors_precomp=colors, scales=scales.detach(), rotations=rot.detach(), cov3D_precomp=None)
        ((depth * dd).sum() + (alpha * da).sum()).backward()

    def lean(hard):
        means.grad = op.grad = None
        if hard:
            m2 = torch.zeros_like(means, requires_grad=True)
            depth, alpha, radii = depth_pass(rs, means, 0.95, scales, rot, grad="means", means2D=m2)
        else:
            depth, alpha, radii = depth_pass(rs, means.detach(), op, scales, rot, grad="opacity")
        ((depth * dd).sum() + (alpha * da).sum()).backward()
    return {"hard": (lambda: general(True), lambda: lean(True)), "soft": (lambda: general(False), lambda: lean(False))}


def per_call_ms(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main(path):
    import torch
    assert torch.cuda.is_available(), "depth_pass_timing needs the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("forward + backward per call, ms: device-synchronised wall time over %d calls of each form, forms alternating after %d "
        "warm-up calls; %d repetitions of the whole comparison" % (CALLS, WARMUP, REPS))
    say("general = the reference composition through dgr_dng.GaussianRasterizer; depth_pass = gsplat_amd.depth_pass")
    for what, P, W, H in SIZES:
        say(what)
        fs = forms(torch, P, W, H)
        for mode, (general, lean) in fs.items():
            for _ in range(WARMUP):
                general()
                lean()
            reps = []
            for _ in range(REPS):
                g = per_call_ms(torch, general, CALLS)
                d = per_call_ms(torch, lean, CALLS)
                reps.append((g, d))
            gs, ds = [r[0] for r in reps], [r[1] for r in reps]
            say("  %-4s general %s   depth_pass %s   general / depth_pass: %s"
                % (mode, " ".join("%.3f" % x for x in gs), " ".join("%.3f" % x for x in ds),
                   " ".join("%.2f" % (a / b) for a, b in reps)))
            say("       spread (max - min) general %.3f, depth_pass %.3f; smallest gap between the forms %.3f"
                % (max(gs) - min(gs), max(ds) - min(ds), min(gs) - max(ds)))
        del fs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")


def trace():
    import torch
    assert torch.cuda.is_available(), "depth_pass_timing needs the GPU"
    _, P, W, H = SIZES[0]
    for mode, (general, lean) in forms(torch, P, W, H).items():
        for _ in range(TRACE_CALLS):
            general()
        for _ in range(TRACE_CALLS):
            lean()
    torch.cuda.synchronize()
    print("enqueued %d calls of each form and mode at P = %d, %d x %d" % (TRACE_CALLS, P, W, H))


def kernels(where, path=None):
    rows = []
    for p in sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True)):
        rows += list(csv.DictReader(open(p)))
    assert rows, "no kernel table under %s" % where
    out = ["kernels at %s (rocprofv3 --kernel-trace --stats, a run of its own: %d calls of each form and mode; hard and soft "
           "share a row where they share a kernel)" % (SIZES[0][0], TRACE_CALLS)]
    for row in rows:
        name = next((k for k in KERNELS if k in row["Name"]), None)
        if name is None:
            continue
        targs = row["Name"][row["Name"].find("<"):row["Name"].find(">") + 1] if "<" in row["Name"] else ""
        out.append("  %-26s %-22s %5d calls  average %8.2f us" % (name, targs[:22], int(row["Calls"]), float(row["AverageNs"]) / 1e3))
    print("\n".join(out))
    if path:
        open(path, "a").write("\n".join(out) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
    elif len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_pass_timing.txt"))

"""Developer tool: what one coloured depth frame costs, per frame at 504 x 378 and 1920 x 1080, two sides from the same depth and
alpha images in device memory:

  reference's statements   device -> host copy of the composite (depth.squeeze().cpu().numpy() after render.py:121 on the
                           device), then on the host the numpy restatement gsplat_amd.depth_vis.colour_depth_numpy states:
                           np.argsort percentiles, curve, table look-up, bytes.  Host clock around the whole, the device
                           synchronised before and after; median of HOST_REPS.  This is the baseline, never the code under test.
  colour_depth             gsplat_amd.depth_vis.colour_depth(depth, alpha, rule) on the device (csrc/gs_depth_vis.hip: ten or
                           twelve launches, no read-back).  Device events around a window of calls, after warm-up: the call count
                           is what fills WINDOW_S of device time, from a probe of PROBE calls; REPS windows; median and spread
                           (max - min) of the per-call time.  Beside it one call's host clock with a synchronise after it (what a
                           caller that needs the bytes at once waits).

Nothing is asserted and no ratio is claimed: the two sides run on different processors, and the host side depends on the
machine's load and on numpy's build.  Writes to stdout and to --out (default profiles/depth_vis_timing.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S, PROBE, WARMUP, REPS, HOST_REPS = 0.25, 50, 20, 11, 5
SIZES = ((378, 504), (1080, 1920))


def per_call_ms(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def median_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def timed(torch, fn):
    for _ in range(WARMUP):
        fn()
    iters = max(PROBE, int(WINDOW_S * 1e3 / per_call_ms(torch, fn, PROBE)) + 1)
    return median_spread([per_call_ms(torch, fn, iters) for _ in range(REPS)]) + (iters,)


def main(out_path):
    import torch
    assert torch.cuda.is_available(), "depth_vis_timing needs the GPU"
    import depth_vis_cases as dc
    from gsplat_amd import depth_vis as dv
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("coloured depth, per frame: device side median ms (spread = max - min over %d windows of at least %.2f s), device events; "
        "host side median of %d, host clock, %d torch threads" % (REPS, WINDOW_S, HOST_REPS, torch.get_num_threads()))
    for H, W in SIZES:
        depth = torch.from_numpy(dc.smooth_depth(H, W, 300)).to(dev)
        alpha = torch.from_numpy(dc.smooth_alpha(H, W, 301)).to(dev)
        for rule, with_alpha in (("dng", True), ("fsgs", False)):
            a = alpha if with_alpha else None
            t = timed(torch, lambda: dv.colour_depth(depth, a, rule=rule))
            torch.cuda.synchronize()
            one = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                out = dv.colour_depth(depth, a, rule=rule)
                torch.cuda.synchronize()
                one.append((time.perf_counter() - t0) * 1e3)

            def reference():
                x = depth
                if with_alpha:
                    x = (depth - depth.min()) / (depth.max() - depth.min()) + 1 * (1 - alpha)
                host = x.squeeze().cpu().numpy()
                return dv.colour_depth_numpy(host, None, rule)[0]
            reference()
            ref = []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rgb = reference()
                ref.append((time.perf_counter() - t0) * 1e3)
            differ = int((torch.from_numpy(rgb).to(dev) != out).any(dim=-1).sum())
            m1, mr = median_spread(one), median_spread(ref)
            say("  %4d x %4d %-4s%s  colour_depth %8.4f ms (spread %.4f, %d calls a window), one call + synchronise %7.3f ms (spread %.3f)"
                "   reference's statements (copy + numpy) %9.3f ms (spread %.3f)   pixels differing %d of %d"
                % (W, H, rule, " + composite" if with_alpha else "            ", t[0], t[1], t[2], m1[0], m1[1], mr[0], mr[1],
                   differ, H * W))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "depth_vis_timing.txt")
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        out = sys.argv[2]
    main(out)

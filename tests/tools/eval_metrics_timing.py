"""Developer tool: the per-view cost of test-set evaluation at 400 x 400 and 1080 x 1920 (C = 3), in two forms in the same
process on the same GPU:
    fused   gsplat_amd.evaluate.image_metrics(clamp=True, quantise=True) - csrc/gs_eval.hip, two launches, no read-back
    chain   what it replaces, written with torch on the device: clamp, the stated 8-bit quantisation of both images, the
            reference-form psnr (20 log10(1 / sqrt(mean squared error))), the package's own fused_ssim, and the mean |a - b|
            (no read-back either: the chain is timed as launches on the stream)
Device events around ITERS calls, after warm-up, REPS repetitions with the forms alternating; median and spread (max - min)
of the per-call time.  Beside the fused time: the bytes of one read of the two images over the CALL's time, as a fraction
of 6.3 TB/s - an end-to-end rate that includes both launches and the allocations of the call, not a kernel's share of peak.

Then a test set of 24 views (pre-rendered images: the rasterizer is not what is measured) scored in two loops:
    one read-back   Evaluator.add per view, Evaluator.result() at the end
    item per metric the chain per view with a .item() for psnr, ssim and l1, as metrics.py / training_report read them
Host clock around the loop, ending in a device synchronise, median of REPS.  Nothing is asserted.
Writes to stdout (kept as profiles/eval_metrics_timing.txt).

Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/eval_metrics_timing.py --trace
    python tests/tools/eval_metrics_timing.py --kernels DIR
--trace enqueues TRACE_CALLS fused calls at each size and nothing else of this library; --kernels reads the profiler's kernel
table and prints the two kernels of csrc/gs_eval.hip (their averages are over both sizes' calls when both were traced: trace
one size with --trace H W)."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((400, 400), (1080, 1920))
ITERS, WARMUP, REPS = 100, 10, 21
VIEWS = 24
HBM = 6.3e12
TRACE_CALLS = 20


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


def main():
    import torch
    assert torch.cuda.is_available(), "eval_metrics_timing needs the GPU"
    import eval_reference as ref
    from fused_ssim import fused_ssim
    from gsplat_amd import evaluate
    dev = torch.device("cuda:0")

    def quantise(x):
        return x.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).to(torch.float32).div(255)

    def chain(r, g):
        a, b = quantise(r)[None], quantise(g)[None]
        mse = ((a - b) ** 2).view(1, -1).mean(1, keepdim=True)
        return 20 * torch.log10(1.0 / torch.sqrt(mse)), fused_ssim(a, b, train=False), torch.abs(a - b).mean()

    print("per view: median ms (spread = max - min over %d repetitions of %d calls), C = 3" % (REPS, ITERS))
    for H, W in SIZES:
        render, gt = (t.to(dev) for t in ref.seeded_pair(3, H, W, seed=H, spread=0.1))
        fs = (("fused", lambda: evaluate.image_metrics(render, gt, clamp=True, quantise=True)), ("chain", lambda: chain(render, gt)))
        with torch.no_grad():
            got, want = evaluate.image_metrics(render, gt, clamp=True, quantise=True), chain(render, gt)
            print("  %d x %d: fused psnr %.6f ssim %.7f l1 %.7f | chain psnr %.6f ssim %.7f l1 %.7f"
                  % (H, W, float(got["psnr"]), float(got["ssim"]), float(got["l1"]), float(want[0]), float(want[1]), float(want[2])))
            for _, fn in fs:
                for _ in range(WARMUP):
                    fn()
            times = {n: [] for n, _ in fs}
            for _ in range(REPS):
                for n, fn in fs:
                    times[n].append(per_call_ms(torch, fn, ITERS))
        f, c = median_spread(times["fused"]), median_spread(times["chain"])
        nbytes = 2 * 3 * H * W * 4
        print("  %d x %d: fused %8.4f ms (spread %.4f)   chain %8.4f ms (spread %.4f)   chain / fused = %.2f"
              % (H, W, f[0], f[1], c[0], c[1], c[0] / f[0]))
        print("  %s one read of the two images is %.2f MB: %.1f %% of 6.3 TB/s over the fused call's time"
              % (" " * len("%d x %d:" % (H, W)), nbytes / 1e6, 100.0 * nbytes / (f[0] * 1e-3) / HBM))

        views = [tuple(t.to(dev) for t in ref.seeded_pair(3, H, W, seed=1000 + i, spread=0.1)) for i in range(VIEWS)]

        def one_read_back():
            ev = evaluate.Evaluator(VIEWS, 3, H, W, dev)
            for i, (r, g) in enumerate(views):
                ev.add(i, r, g, clamp=True, quantise=True)
            return ev.result()

        def item_per_metric():
            out = []
            for r, g in views:
                p, s, l1 = chain(r, g)
                out.append((p.item(), s.item(), l1.item()))
            return out

        loops = (("one read-back", one_read_back), ("item per metric", item_per_metric))
        wall = {n: [] for n, _ in loops}
        with torch.no_grad():
            for _, fn in loops:
                fn()
            for _ in range(REPS):
                for n, fn in loops:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall[n].append((time.perf_counter() - t0) * 1e3)
        a, b = median_spread(wall["one read-back"]), median_spread(wall["item per metric"])
        print("  %d x %d, %d views (host clock, ms per loop): one read-back %8.3f (spread %.3f)   item per metric %8.3f (spread %.3f)"
              "   ratio %.2f" % (H, W, VIEWS, a[0], a[1], b[0], b[1], b[0] / a[0]))


def trace(sizes):
    import torch
    assert torch.cuda.is_available(), "eval_metrics_timing needs the GPU"
    import eval_reference as ref
    from gsplat_amd import evaluate
    for H, W in sizes:
        render, gt = (t.to("cuda:0") for t in ref.seeded_pair(3, H, W, seed=H, spread=0.1))
        for _ in range(TRACE_CALLS):
            evaluate.image_metrics(render, gt, clamp=True, quantise=True)
        torch.cuda.synchronize()
        print("enqueued %d fused calls at %d x %d" % (TRACE_CALLS, H, W))


def kernels(where):
    rows = []
    for path in sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True)):
        rows += list(csv.DictReader(open(path)))
    assert rows, "no kernel table under %s" % where
    print("kernels of csrc/gs_eval.hip (rocprofv3 --kernel-trace --stats, a run of its own)")
    for row in rows:
        for k in ("eval_tile_kernel", "eval_finish_kernel"):
            if k in row["Name"]:
                print("  %-20s %4d calls  average %8.2f us" % (k, int(row["Calls"]), float(row["AverageNs"]) / 1e3))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace(((int(sys.argv[2]), int(sys.argv[3])),) if len(sys.argv) > 3 else SIZES)
    elif len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        main()

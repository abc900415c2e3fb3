"""Developer tool: what the evaluation from files costs per view on the device (csrc/gs_eval_files.hip), two figures:

  DTU view   uint8 render, ground truth [1200,1600,3] and mask [1200,1600,1] already in device memory -> the view's metrics
             row: three gs_resize_bicubic_u8 calls to 400 x 300 (bytes and the fp32 planar image) and Evaluator.add with the
             mask, without and with ssim_sk.  Reading and decoding the PNG files is host work and is not in the figure.
  ssim_sk    gs_eval_ssim_sk alone (its two launches, scratch preallocated) at 400 x 300 and at 1080 x 1920, C = 3.

Device events around a window of calls, after warm-up: the call count of a case is what fills WINDOW_S (0.25 s) of device
time, from a probe of PROBE calls; REPS such windows; median and spread (max - min) of the per-call time.
Beside them, where Pillow imports, the host's cost of the same DTU view: three Image.resize calls, and torch on the CPU for
to_tensor, the blend and the reference-form PSNR / SSIM (tests/eval_reference.py's float64 restatement - not the reference's
float32 CUDA run, which needs the reference's own stack).  Host clock, median of HOST_REPS.  Nothing is asserted and no ratio
is claimed: the two sides run on different processors and the host side depends on the machine's load.
Writes to stdout and to --out (default profiles/eval_files_timing.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S, PROBE, WARMUP, REPS, HOST_REPS = 0.25, 50, 20, 11, 5   # a repetition is a window of at least WINDOW_S of device time
FULL, QUARTER = (1200, 1600), (300, 400)
SK_SIZES = ((300, 400), (1080, 1920))


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
    """-> (median ms per call, spread, calls per window)"""
    for _ in range(WARMUP):
        fn()
    iters = max(PROBE, int(WINDOW_S * 1e3 / per_call_ms(torch, fn, PROBE)) + 1)
    return median_spread([per_call_ms(torch, fn, iters) for _ in range(REPS)]) + (iters,)


def main(out_path):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "eval_files_timing needs the GPU"
    import eval_files_reference as fref
    import eval_reference as ref
    from gsplat_amd import evaluate, imageio
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    H, W = FULL
    H2, W2 = QUARTER
    render8, gt8 = fref.seeded_u8(H, W, 3, 1), fref.seeded_u8(H, W, 3, 2)
    mask8 = fref.content_u8("masklike", H, W, 1)
    r, g, m = (torch.from_numpy(a).to(dev) for a in (render8, gt8, mask8))
    ev = {sk: evaluate.Evaluator(1, 3, H2, W2, dev, ssim_sk=sk) for sk in (False, True)}

    def view(sk):
        mp = imageio.resize_u8(m, (W2, H2), return_planar=True)[1][0]
        rp = imageio.resize_u8(r, (W2, H2), return_planar=True)[1]
        gp = imageio.resize_u8(g, (W2, H2), return_planar=True)[1]
        ev[sk].add(0, rp, gp, mask=mp)

    say("evaluation from files, per view: median ms (spread = max - min over %d windows of at least %.2f s), device events" % (REPS, WINDOW_S))
    for sk in (False, True):
        t = timed(torch, lambda: view(sk))
        row = ev[sk].result()
        say("  DTU view %d x %d -> %d x %d, bytes on the device -> metrics row%s: %8.4f ms (spread %.4f, %d calls a window)   PSNR %.4f SSIM %.6f%s"
            % (W, H, W2, H2, " + ssim_sk" if sk else "           ", t[0], t[1], t[2], row["PSNR"], row["SSIM"],
               " SSIM_sk %.6f" % row["SSIM_sk"] if sk else ""))
    for h, w in SK_SIZES:
        a, b = (x.to(dev) for x in ref.seeded_pair(3, h, w, seed=h, spread=0.1))
        tmp = evaluate._sk_tmp(dev, 3, h, w)
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        fn = lambda: evaluate._launch_sk(a, b, None, 3, h, w, evaluate.CLAMP | evaluate.QUANTISE, tmp, out)  # noqa: E731
        t = timed(torch, fn)
        say("  ssim_sk %4d x %4d, C = 3 (two launches, clamp + quantise): %8.4f ms (spread %.4f, %d calls a window)   value %.7f"
            % (h, w, t[0], t[1], t[2], float(out)))
    try:
        from PIL import Image
    except ImportError:
        say("  host: Pillow does not import here - not measured")
    else:
        def host_resize():
            size = (W // 4, H // 4)
            return (Image.fromarray(mask8[:, :, 0]).resize(size), Image.fromarray(render8).resize(size), Image.fromarray(gt8).resize(size))

        def host_metrics(imgs):
            mt, rt, gt_ = (torch.from_numpy(np.asarray(i).reshape(H2, W2, -1).copy()).permute(2, 0, 1).float().div(255) for i in imgs)
            return ref.metrics(rt, gt_, mt[0])

        imgs = host_resize()
        tr, tm = [], []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            imgs = host_resize()
            t1 = time.perf_counter()
            host_metrics(imgs)
            t2 = time.perf_counter()
            tr.append((t1 - t0) * 1e3)
            tm.append((t2 - t1) * 1e3)
        a, b = median_spread(tr), median_spread(tm)
        say("  host, same view (host clock, median of %d, %d torch threads): Pillow's three resizes %8.3f ms (spread %.3f)   torch "
            "CPU blend + float64 PSNR / SSIM / L1 %8.3f ms (spread %.3f)" % (HOST_REPS, torch.get_num_threads(), a[0], a[1], b[0], b[1]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "eval_files_timing.txt")
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        out = sys.argv[2]
    main(out)

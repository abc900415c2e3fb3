"""Developer tool: the cost of LPIPS (VGG16) per view pair at 400 x 300, 504 x 378 and 1920 x 1080, in two forms in the same
process on the same GPU, with the same seeded weights (tests/lpips_cases.py):
    hip     gsplat_amd.lpips.lpips_vgg - csrc/gs_lpips.hip, scratch allocated once, no read-back
    torch   the same chain written with torch on the device: z_score, F.conv2d + relu, F.max_pool2d and the reference's tail
            statements in float32 (tests/lpips_reference.py), both images as one batch of 2, under no_grad
Device events around ITERS calls, after warm-up, REPS windows with the forms alternating; median and spread (max - min over
the windows) of the per-call time.  The two results are printed beside each other (they differ by float32 rounding).

Then, at 1920 x 1080, each of the thirteen convolutions on its own through the stage entry gs_lpips_conv3x3_relu (weights
packed beforehand), timed the same way: ms per launch and achieved TFLOP/s = 2 x 2 H W 9 Cin Cout / time, to be read beside
the part's 157.3 TFLOP/s f32 matrix peak and the 122 TFLOP/s of an untuned LDS-tiled 4096^3 GEMM on the same instruction.
These are event times around back-to-back launches, not profiler kernel times.  Nothing is asserted.
Writes to stdout (kept as profiles/lpips_timing.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((300, 400), (378, 504), (1080, 1920))   # (H, W)
WARMUP, REPS = 2, 7
PEAK_TF, GEMM_TF = 157.3, 122.0


def iters_for(H, W):
    return 3 if H * W > 1000000 else 20


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
    assert torch.cuda.is_available(), "lpips_timing needs the GPU"
    import lpips_cases as cases
    import lpips_reference as ref
    from gsplat_amd import lpips as impl
    from gsplat_amd._lib import hip_api
    dev = torch.device("cuda:0")
    vgg_sd, lin_sd = cases.make_state_dicts()
    weights = impl.LpipsWeights.from_state_dicts(vgg_sd, lin_sd)
    vgg_dev = {k: v.to(dev) for k, v in vgg_sd.items()}
    lin_dev = {k: v.to(dev) for k, v in lin_sd.items()}

    def chain(render, gt):
        return ref.lpips(render, gt, vgg_dev, lin_dev, torch.float32)[0]

    print("per view pair: median ms (spread = max - min over %d windows)" % REPS, flush=True)
    with torch.no_grad():
        for H, W in SIZES:
            r8, g8 = cases.whole_images(H, W, seed=H)
            render, gt = cases.planar(r8).to(dev), cases.planar(g8).to(dev)
            tmp = torch.empty((impl.tmp_bytes(H, W),), dtype=torch.uint8, device=dev)
            fs = (("hip", lambda: impl.lpips_vgg(render, gt, weights, tmp=tmp)), ("torch", lambda: chain(render, gt)))
            iters = iters_for(H, W)
            for _, fn in fs:
                for _ in range(WARMUP):
                    fn()
            got, want = float(fs[0][1]()), float(fs[1][1]())
            times = {n: [] for n, _ in fs}
            for _ in range(REPS):
                for n, fn in fs:
                    times[n].append(per_call_ms(torch, fn, iters))
            h, t = median_spread(times["hip"]), median_spread(times["torch"])
            print("  %4d x %4d (%d calls per window, scratch %.1f MB): hip %9.3f ms (spread %.3f)   torch %9.3f ms (spread %.3f)"
                  "   torch / hip = %.2f   | lpips hip %.9f torch %.9f"
                  % (W, H, iters, tmp.numel() / 1e6, h[0], h[1], t[0], t[1], t[0] / h[0], got, want), flush=True)
            del tmp

        H, W = SIZES[-1]
        api = hip_api()
        packed, bias = weights.on(dev)[0], weights.on(dev)[1]
        stream = impl._stream(packed[0])
        print("the thirteen convolutions at %d x %d, N = 2 (ms per launch, spread over %d windows of 3 launches; peak %.1f, "
              "untuned GEMM %.0f TFLOP/s)" % (W, H, REPS, PEAK_TF, GEMM_TF), flush=True)
        h, w, layer, total = H, W, 0, 0.0
        for blk, n in enumerate(cases.BLOCK_CONVS):
            if blk:
                h, w = h // 2, w // 2
            for _ in range(n):
                cin, cout = cases.CONV_SHAPE[layer]
                x = torch.rand((2, cin, h, w), device=dev)
                y = torch.empty((2, cout, h, w), device=dev)

                def fn():
                    api.call("lpips_conv3x3_relu", x.data_ptr(), packed[layer].data_ptr(), bias[layer].data_ptr(), 2, cin, cout,
                             h, w, y.data_ptr(), stream)
                fn()
                ms, spread = median_spread([per_call_ms(torch, fn, 3) for _ in range(REPS)])
                flop = 2.0 * 2 * h * w * 9 * cin * cout
                total += ms
                print("  conv %2d  %3d -> %3d at %4d x %4d: %8.3f ms (spread %.3f)  %6.1f TFLOP/s  (%4.1f %% of peak)"
                      % (layer + 1, cin, cout, w, h, ms, spread, flop / ms / 1e9, 100.0 * flop / ms / 1e9 / PEAK_TF), flush=True)
                layer += 1
                del x, y
        print("  sum of the thirteen: %.3f ms" % total, flush=True)


if __name__ == "__main__":
    main()

"""Developer tool: one reference-shaped depth-regulariser call of a DNGaussian training step,
    0.1 * patch_norm_mse_loss(p_local) + 0.1 * loss_depth_smoothness + 1 * patch_norm_mse_loss_global(p_global), then backward,
at 378x504, 300x400, 400x400 and 1080x1920, in three forms in the same process on the same GPU:
    separate   dng_loss's three nodes (csrc/gs_depth_norm.hip), summed by torch
    fused      dng_loss.depth_regulariser: one forward, one backward
    eager      tests/dng_depth_reference.py in fp32 eager torch - what a DNGaussian user runs today (unfold-free, but the
               same dozens of small launches and the host synchronisation of the boolean-mask gather)
Device events around ITERS calls, after warm-up, REPS repetitions with the forms alternating; median and spread
(max - min) of the per-call time.  Nothing is asserted; where the fused form does not beat the eager one by more than
the two spreads combined, the line says so.  Writes to stdout (kept as profiles/dng_depth_timing.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import dng_depth_reference as ref  # noqa: E402
import dng_loss  # noqa: E402

SIZES = ((378, 504, 11, 7), (300, 400, 11, 7), (400, 400, 11, 7), (1080, 1920, 35, 23))  # H, W, p_local, p_global
MARGIN, ITERS, WARMUP, REPS = 0.01, 50, 10, 7


def per_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def main():
    assert torch.cuda.is_available(), "dng_depth_timing needs the GPU"
    dev = torch.device("cuda:0")
    print("depth regulariser, forward + backward, per call: median ms (spread = max - min over %d repetitions of %d calls)"
          % (REPS, ITERS))
    for H, W, pl, pg in SIZES:
        depth, mono = ref.scene(H, W, seed=H + W, dtype=torch.float32)
        x = depth.to(dev).requires_grad_(True)
        t = mono.to(dev)

        def separate():
            x.grad = None
            loss = 0.1 * dng_loss.patch_norm_mse_loss(x, t, pl, MARGIN)
            loss = loss + 0.1 * dng_loss.loss_depth_smoothness(x, t)
            loss = loss + 1.0 * dng_loss.patch_norm_mse_loss_global(x, t, pg, MARGIN)
            loss.backward()

        def fused():
            x.grad = None
            dng_loss.depth_regulariser(x, t, pl, pg, MARGIN, 0.1, 1.0, 0.1).backward()

        def eager():
            x.grad = None
            ref.depth_regulariser(x, t, pl, pg, MARGIN, 0.1, 1.0, 0.1).backward()

        forms = (("separate", separate), ("fused", fused), ("eager", eager))
        for _, fn in forms:
            for _ in range(WARMUP):
                fn()
        times = {name: [] for name, _ in forms}
        for _ in range(REPS):
            for name, fn in forms:
                times[name].append(per_call_ms(fn))
        stat = {}
        for name, v in times.items():
            v = sorted(v)
            stat[name] = (v[len(v) // 2], v[-1] - v[0])
        print("%dx%d  p_local=%d p_global=%d margin=%g" % (H, W, pl, pg, MARGIN))
        for name, _ in forms:
            print("  %-9s %8.4f ms  (spread %.4f)" % (name, *stat[name]))
        gain = stat["eager"][0] - stat["fused"][0]
        noise = stat["eager"][1] + stat["fused"][1]
        verdict = "beats eager by more than the two spreads" if gain > noise else "does NOT beat eager by more than the two spreads"
        print("  fused %s: %.4f ms faster, spreads combined %.4f ms, eager / fused = %.2f"
              % (verdict, gain, noise, stat["eager"][0] / stat["fused"][0]))


if __name__ == "__main__":
    main()

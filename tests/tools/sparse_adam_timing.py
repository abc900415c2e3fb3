"""Developer tool: what the one-launch optimizer step and the `dc=` rasterizer call cost on one MI355X.  Needs the GPU; nothing
is asserted.  Writes profiles/sparse_adam_timing.txt (or the path given with --out) and prints the same lines.

Method: device-event times (an event before and one behind a WINDOW of calls on the stream, at least MIN_WINDOW seconds long, after
WARMUP calls), every form measured REPS times with the forms alternating inside one process; median and spread (max - min) of the
per-call time.  First of all the spread of ONE form measured again and again: a difference between two forms counts when it is
larger than that.

(a) the optimizer alone: the reference's six tensors (P x {3,3,45,1,3,4} floats) at P = 1 000 000 with random gradients -
      torch.optim.Adam | FusedAdam (one launch per tensor: the form before gs_adam_step_tensors) | FusedAdam(fuse_groups=True) |
      SparseGaussianAdam under both rules at visible shares of 100, 30, 10 and 1 %, each share once as runs of RUN consecutive
      rows (what a camera sees of rows in Morton order) and once scattered at random.
    Beside each sparse figure the traffic model's bytes - P mask bytes + 28 B x the elements of the float4s that hold a stepped
    element (traffic_model below) - and that over the time, against COPY_RATE (the copy rate VERDICT.md records).
(b) DropInLoop at BASELINE config 3 (1 M Gaussians, 1920 x 1080, global + patch DWT), per iteration: optimizer="fused" | the same
    with separate_sh=True | optimizer="sparse_adam", separate_sh=True | the last with use_camera_key=True; rows as generated and
    in Morton order (gsplat_amd.synthetic.spatially_ordered)."""
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

P_OPT = 1_000_000
WIDTHS = (3, 3, 45, 1, 3, 4)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.025, 0.005, 0.001)
SHARES = (1.0, 0.3, 0.1, 0.01)
RUN = 2048
MIN_WINDOW, WARMUP, REPS = 0.2, 20, 3
COPY_RATE = 6.29e12
C3 = (1_000_000, 1920, 1080)

OUT = [None]


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(line + "\n")


def traffic_model(mask, widths=WIDTHS):
    """Bytes the masked one-launch step has to move: the P mask bytes + 28 B (g read; p, m, v read and written) for every element
    of a float4 that holds at least one stepped element; a tensor's last n % 4 elements count one by one."""
    mask = np.asarray(mask, bool)
    total = mask.size
    for w in widths:
        on = np.repeat(mask, w)
        body = on[:on.size // 4 * 4].reshape(-1, 4).any(axis=1)
        total += 28 * (4 * int(body.sum()) + int(on[on.size // 4 * 4:].sum()))
    return total


def window(torch, call, per_call_guess):
    """seconds per call over one window of >= MIN_WINDOW seconds, from device events"""
    n = max(5, int(MIN_WINDOW / max(per_call_guess, 1e-6)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def measure(torch, forms):
    """{name: call} -> {name: (median, spread)} in seconds per call; forms alternate, REPS windows each"""
    guess = {}
    for name, call in forms.items():
        for _ in range(WARMUP):
            call()
        guess[name] = window(torch, call, 1e-3)
    times = {name: [] for name in forms}
    gc.collect()
    gc.disable()
    try:
        for _ in range(REPS):
            for name, call in forms.items():
                times[name].append(window(torch, call, guess[name]))
    finally:
        gc.enable()
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in times.items()}


def make_groups(torch, dev, P, seed):
    g = torch.Generator().manual_seed(seed)
    groups = []
    for w, lr, name in zip(WIDTHS, LRS, NAMES):
        p = torch.nn.Parameter((torch.randn((P, w), generator=g)).to(dev))
        p.grad = (torch.randn((P, w), generator=g) * 1e-3).to(dev)
        groups.append({"params": [p], "lr": lr, "name": name})
    return groups


def masks(P, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for share in SHARES:
        blocks = (P + RUN - 1) // RUN
        runs = np.repeat(rng.random(blocks) < share, RUN)[:P] if share < 1.0 else np.ones(P, bool)
        scattered = rng.random(P) < share if share < 1.0 else np.ones(P, bool)
        out.append((share, "runs of %d rows" % RUN, runs))
        if share < 1.0:
            out.append((share, "scattered", scattered))
    return out


def optimizer_alone(torch, dev):
    from gsplat_amd.optim import FusedAdam, SparseGaussianAdam
    P = P_OPT
    say("(a) optimizer alone: six tensors, P = %d (%d floats), ms per step: median (spread = max - min) of %d windows of >= %.1f s, "
        "device events, forms alternating" % (P, P * sum(WIDTHS), REPS, MIN_WINDOW))
    fused_a = FusedAdam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15)
    fused_b = FusedAdam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15)
    same = measure(torch, {"FusedAdam, first instance": fused_a.step, "FusedAdam, second instance": fused_b.step,
                           "FusedAdam, first instance again": fused_a.step})
    vals = [v[0] for v in same.values()]
    spread = max(max(vals) - min(vals), max(v[1] for v in same.values()))
    for k, (med, sp) in same.items():
        say("  the same form repeated: %-34s %.4f (%.4f)" % (k, med * 1e3, sp * 1e3))
    say("  -> spread of the same form: %.4f ms; a difference below it is not one" % (spread * 1e3))
    del fused_b
    dense_bytes = 28 * P * sum(WIDTHS)
    forms = {"torch.optim.Adam": torch.optim.Adam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15).step,
             "FusedAdam (six launches)": fused_a.step,
             "FusedAdam(fuse_groups=True)": FusedAdam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15, fuse_groups=True).step}
    sparse = {False: SparseGaussianAdam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15),
              True: SparseGaussianAdam(make_groups(torch, dev, P, 1), lr=0.0, eps=1e-15, bias_correction=True)}
    forms["SparseGaussianAdam.step(), no-bias rule"] = sparse[False].step
    forms["SparseGaussianAdam.step(), torch's rule"] = sparse[True].step
    res = measure(torch, forms)
    for k, (med, sp) in res.items():
        say("  %-44s %.4f (%.4f)   %6.1f MB = %.2f TB/s = %.0f %% of the %.2f TB/s copy rate"
            % (k, med * 1e3, sp * 1e3, dense_bytes / 1e6, dense_bytes / med / 1e12, 100.0 * dense_bytes / med / COPY_RATE, COPY_RATE / 1e12))
    six, one = res["FusedAdam (six launches)"][0], res["FusedAdam(fuse_groups=True)"][0]
    say("  one launch - six launches = %+.4f ms (spread %.4f): %s" % ((one - six) * 1e3, spread * 1e3,
        "not slower" if one - six <= spread else "SLOWER than the six launches by more than the spread"))
    dense = res["SparseGaussianAdam.step(), no-bias rule"][0]
    for share, kind, mask in masks(P):
        vis = torch.from_numpy(mask).to(dev)
        r = measure(torch, {rule: (lambda o=opt: o.step(vis, P)) for rule, opt in sparse.items()})
        b = traffic_model(mask)
        for rule, (med, sp) in r.items():
            say("  SparseGaussianAdam %-13s %5.1f %% visible (%6.2f %% measured), %-17s %.4f (%.4f)   model %6.1f MB = %.2f TB/s = %3.0f %% "
                "of the copy rate;  dense - this = %+.4f ms" % ("torch's rule" if rule else "no-bias rule", 100 * share, 100.0 * mask.mean(), kind,
                                                                med * 1e3, sp * 1e3, b / 1e6, b / med / 1e12, 100.0 * b / med / COPY_RATE,
                                                                (dense - med) * 1e3))
    return spread


def drop_in(torch, dev):
    from gsplat_amd import hip_backend, synthetic
    from gsplat_amd.dropin import DropInLoop, DropInModel, render
    from gsplat_amd.trainer import camera_to
    from simple_knn._C import distCUDA2
    P, W, H = C3
    say("(b) DropInLoop at BASELINE config 3 (P = %d, %d x %d, global + patch DWT), ms per iteration (the loop's own loss.item() "
        "included): median (spread) of %d windows of >= %.1f s, forms alternating" % (P, W, H, REPS, MIN_WINDOW))
    knn = lambda x: distCUDA2(x.to(dev)).cpu()  # noqa: E731
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)]
    gt_model = DropInModel(synthetic.trained_like(P, seed=1, knn=knn), dev)
    gts = [(torch.round(render(c, gt_model, torch.zeros(3, device=dev))["render"].detach() * 255.0) / 255.0).contiguous() for c in cams]
    del gt_model
    base = synthetic.trained_like(P, seed=0, knn=knn)
    for label, scene in (("rows as generated", base), ("rows in Morton order", synthetic.spatially_ordered(base))):
        kinds = (("optimizer=fused", dict(optimizer="fused")),
                 ("optimizer=fused, separate_sh", dict(optimizer="fused", separate_sh=True)),
                 ("optimizer=sparse_adam, separate_sh", dict(optimizer="sparse_adam", separate_sh=True)),
                 ("optimizer=sparse_adam, separate_sh, camera_key", dict(optimizer="sparse_adam", separate_sh=True, use_camera_key=True)))
        loops, forms, counters = {}, {}, {}
        for name, kw in kinds:
            loop = loops[name] = DropInLoop(scene, cams, gts, dev, dwt=True, patch=True, **kw)
            counters[name] = 0
            for j in range(len(cams) + 2):      # every camera once (a keyed camera's limits exist from its second visit on)
                loop.iteration(j % len(cams))

            def call(loop=loop, name=name):
                counters[name] += 1
                loop.iteration(counters[name] % len(cams))
            forms[name] = call
        say("  %s" % label)
        same = measure(torch, {"optimizer=fused": forms["optimizer=fused"], "optimizer=fused, again": forms["optimizer=fused"]})
        vals = [v[0] for v in same.values()]
        spread = max(max(vals) - min(vals), max(v[1] for v in same.values()))
        say("    the same form repeated: %.4f and %.4f -> spread %.4f ms" % (vals[0] * 1e3, vals[1] * 1e3, spread * 1e3))
        res = measure(torch, forms)
        first = res["optimizer=fused"][0]
        for name, (med, sp) in res.items():
            say("    %-48s %.4f (%.4f)   fused - this = %+.4f ms" % (name, med * 1e3, sp * 1e3, (first - med) * 1e3))
        pkg = render(cams[1], loops["optimizer=fused"].pc, torch.zeros(3, device=dev))
        say("    visible share at camera 1: %.1f %%" % (100.0 * float((pkg["radii"] > 0).float().mean())))
        del loops, forms
        hip_backend().drop_camera_entries(("dropin",))
        torch.cuda.empty_cache()


def main():
    import torch
    assert torch.cuda.is_available(), "sparse_adam_timing needs the GPU"
    out = os.path.join(ROOT, "profiles", "sparse_adam_timing.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    dev = torch.device("cuda:0")
    open(out, "w").close()
    OUT[0] = out
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if "--skip-optimizer" not in sys.argv:
        optimizer_alone(torch, dev)
        torch.cuda.empty_cache()
    if "--skip-loop" not in sys.argv:
        drop_in(torch, dev)


if __name__ == "__main__":
    main()

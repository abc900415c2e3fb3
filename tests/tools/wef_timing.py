"""Developer tool: what one Wavelet Error Field costs per call at 504 x 378 and 1920 x 1080, both band sets, from the same pred and
gt images in device memory:

  torch chain   what a user had before gsplat_amd.wef: the reference's statements (LGDWT-GS/utils/loss_utils.py:165-221,
                284-329) as torch operations on the device, its two DWTs served by lgdwt_loss.get_dwt_subbands (two launches).
                This is the baseline, never the code under test.
  maps          lgdwt_loss.compute_wef_maps / compute_wef_all_subbands (csrc/gs_wef.hip: six launches)
  maps + grid   the same plus make_wef_grid_image (tile_cols=3): a stack of the tiles and one more launch; for the torch chain
                the reference's make_heatmap_rgb per tile and the byte conversion on the device (its host copy and Pillow
                paste left out, in its favour)

Device events around a window of calls, after warm-up: the call count is what fills WINDOW_S of device time, from a probe of
PROBE calls; the sides ALTERNATE, REPS windows each; median and spread (max - min) of the per-call time.  Launches per call are
counted by torch.profiler over one call (kernels and memcpys on the device), "not measured" if the profiler is unavailable.
Nothing is asserted.  Writes to stdout and to --out (default profiles/wef_timing.txt).

--parity PATH (default profiles/wef_parity.json) also writes, per case of tests/wef_cases.py and band set, the largest derived
bar, the HIP kernels' largest distance to the float64 twin and the reference's own float32 distance to its float64 result
(from tests/golden/wef_maps.npz, for the cases the fixture holds)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S, PROBE, WARMUP, REPS = 0.25, 50, 20, 9
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


def alternate(torch, fns):
    """fns {name: callable} -> {name: (median ms, spread ms, calls per window)}; the windows of the sides alternate"""
    iters = {}
    for n, fn in fns.items():
        for _ in range(WARMUP):
            fn()
        iters[n] = max(PROBE, int(WINDOW_S * 1e3 / per_call_ms(torch, fn, PROBE)) + 1)
    times = {n: [] for n in fns}
    for _ in range(REPS):
        for n, fn in fns.items():
            times[n].append(per_call_ms(torch, fn, iters[n]))
    return {n: median_spread(t) + (iters[n],) for n, t in times.items()}


def launches(torch, fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return str(n) if n > 0 else "not measured"
    except Exception as e:   # noqa: BLE001
        return "not measured (%s)" % type(e).__name__


def torch_chain(torch, lgdwt_loss, all_bands):
    import torch.nn.functional as F
    scale = {"LL1": 1.0, "LH1": 1.0, "HL1": 1.0, "HH1": 1.0, "LL2": 4.0, "LH2": 2.0, "HL2": 2.0, "HH2": 2.0}
    keys = ("LL1", "LH1", "HL1", "HH1", "LL2", "LH2", "HL2", "HH2") if all_bands else ("LL2", "LH2", "HL2")

    def norm(x, eps=1e-8):
        mn, mx = x.amin(dim=(-2, -1), keepdim=True), x.amax(dim=(-2, -1), keepdim=True)
        return (x - mn) / (mx - mn + eps)

    def maps(pred, gt):
        H, W = pred.shape[-2:]
        b = lgdwt_loss.get_dwt_subbands(pred - gt)
        out = {}
        for k in keys:
            e = b[k] * b[k]
            e = e * scale[k]
            e = e.mean(dim=1, keepdim=True)
            out[k] = norm(F.interpolate(e, size=(H, W), mode="bilinear", align_corners=False))
        combo = None
        for k in keys:
            combo = out[k] if combo is None else combo + out[k]
        out["COMBINED" if all_bands else "WEF"] = norm(combo / (8.0 if all_bands else 3.0))
        return out

    def grid(m):
        tiles = []
        for k in m:
            x = m[k].clamp(0, 1)
            g = (1.0 - (x - 0.5).abs() * 2.0).clamp(0, 1)
            hm = torch.cat([x, g, 1.0 - x], dim=1)[0]
            tiles.append((hm.permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8))
        H, W = tiles[0].shape[:2]
        rows = (len(tiles) + 2) // 3
        out = torch.zeros((rows * H, 3 * W, 3), dtype=torch.uint8, device=tiles[0].device)
        for i, t in enumerate(tiles):
            out[(i // 3) * H:(i // 3 + 1) * H, (i % 3) * W:(i % 3 + 1) * W] = t
        return out
    return maps, grid


def sides(torch, lgdwt_loss, pred, gt, all_bands):
    ref_maps, ref_grid = torch_chain(torch, lgdwt_loss, all_bands)
    hip_maps = lgdwt_loss.compute_wef_all_subbands if all_bands else lgdwt_loss.compute_wef_maps

    def hip_grid():
        m = hip_maps(pred, gt)
        return lgdwt_loss.make_wef_grid_image(m, list(m), tile_cols=3)
    fns = {"torch chain, maps": lambda: ref_maps(pred, gt), "kernels, maps": lambda: hip_maps(pred, gt),
           "torch chain, maps + grid": lambda: ref_grid(ref_maps(pred, gt)), "kernels, maps + grid": hip_grid}
    return fns, ref_maps, hip_maps


def timing(out_path):
    import torch
    assert torch.cuda.is_available(), "wef_timing needs the GPU"
    import lgdwt_loss
    dev = torch.device("cuda:0")
    lines, counted = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("Wavelet Error Field, per call: median ms (spread = max - min over %d alternating windows of at least %.2f s), device events"
        % (REPS, WINDOW_S))
    for H, W in SIZES:
        g = torch.Generator().manual_seed(H)
        gt = torch.rand((1, 3, H, W), generator=g).to(dev)
        pred = (gt + 0.1 * torch.randn((1, 3, H, W), generator=g).to(dev)).clamp(0, 1)
        for all_bands in (False, True):
            fns, ref_maps, hip_maps = sides(torch, lgdwt_loss, pred, gt, all_bands)
            res = alternate(torch, fns)
            a, b = ref_maps(pred, gt), hip_maps(pred, gt)
            dist = max(float((a[k] - b[k]).abs().max()) for k in a)
            say("  %4d x %4d %s (largest |torch chain - kernels| on a map %.2e)" % (W, H, "all bands" if all_bands else "level 2  ", dist))
            for n in fns:
                say("      %-26s %8.4f ms (spread %.4f, %d calls a window)" % (n, res[n][0], res[n][1], res[n][2]))
            if (H, W) == SIZES[0]:
                counted.append(("all bands" if all_bands else "level 2", fns))

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    write()   # (the timings are on disk before the profiler is touched)
    say("launches per call (kernels and copies on the device, torch.profiler over one call at %d x %d):" % (SIZES[0][1], SIZES[0][0]))
    for tag, fns in counted:
        say("  %-9s %s" % (tag, ", ".join("%s: %s" % (n, launches(torch, fn)) for n, fn in fns.items())))
    write()


def parity(out_path):
    import numpy as np
    import torch
    import lgdwt_loss
    import wef_cases as wc
    dev = torch.device("cuda:0")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "wef_maps.npz"))
    rows = []
    for c in wc.CASES:
        if c.kind == "nan":
            continue
        pred, gt = (t.to(dev) for t in wc.inputs(c))
        for all_bands, tag in ((False, "l2"), (True, "all")):
            keys = wc.keys_of(all_bands)
            maps = (lgdwt_loss.compute_wef_all_subbands if all_bands else lgdwt_loss.compute_wef_maps)(pred, gt)
            dist = wc.check_maps(c, all_bands, maps, "hip")
            bars = wc.bars(c, all_bands)
            row = {"case": c.name, "C": c.C, "H": c.H, "W": c.W, "bands": tag,
                   "bar_max": max([b for b in bars.values() if b is not None] or [0.0]),
                   "flat_maps": [k for k in keys if bars[k] is None],
                   "hip_to_float64_max": max(dist.values()), "reference_float32_to_float64_max": None}
            if c in wc.FIXTURE_CASES:
                r32, r64 = fx["maps32_%s_%s" % (c.name, tag)], fx["maps64_%s_%s" % (c.name, tag)]
                d = [float(np.abs(r32[i].astype(np.float64) - r64[i]).max()) for i, k in enumerate(keys)]
                row["reference_float32_to_float64_max"] = max(d)
                row["reference_float32_to_float64_max_not_flat"] = max([x for x, k in zip(d, keys) if bars[k] is not None] or [0.0])
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        json.dump({"device": torch.cuda.get_device_name(0), "cases": rows}, fp, indent=1)
        fp.write("\n")
    print("wrote %s (%d rows)" % (out_path, len(rows)))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "wef_timing.txt")
    par = os.path.join(ROOT, "profiles", "wef_parity.json")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    if "--parity" in args:
        par = args[args.index("--parity") + 1]
    parity(par)
    timing(out)

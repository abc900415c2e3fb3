"""Developer tool: what the depth priors' two stages cost, the module's own host numpy path against its device path, on the same
seeded inputs:

  depth_scales      at 24 images x 2 000 observations and at 300 images x 10 000 (maps of 189 x 252 for 756 x 1008 cameras):
                      host            depth_scales(on_device=False), host clock
                      device, call    depth_scales(on_device=True): packing the inputs, the uploads, ONE gs_depth_scales launch and
                                      the read-back that ends it, host clock - what a caller waits
                      device, kernel  the launch alone on inputs already in device memory, device events around a window of calls
  prepare_invdepth  a 1600 x 1200 uint16 map kept at its size and reduced to 800 x 600:
                      host            the numpy path, host clock
                      device, call    from the numpy array: upload + gs_invdepth_prepare, host clock with a synchronise after
                      device, kernel  from a device tensor, device events around a window of calls

One warm-up of every shape, then REPS windows; a device-event window holds as many calls as fill WINDOW_S of device time (from
a probe).  Median and spread (max - min) over the windows.  Nothing is asserted and no ratio is claimed; the reference's script
itself cannot run here (it needs cv2).  Writes to stdout and to --out (default profiles/depth_priors_timing.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S, PROBE, REPS = 0.25, 20, 5
SCENES = ((24, 2000), (300, 10000))


def median_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def host_clock(fn, sync=None):
    fn()                                  # the warm-up
    out = []
    for _ in range(REPS):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return median_spread(out)


def device_events(torch, fn):
    def per_call(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters
    fn()
    iters = max(PROBE, int(WINDOW_S * 1e3 / per_call(PROBE)) + 1)
    return median_spread([per_call(iters) for _ in range(REPS)]) + (iters,)


def scene(np, gio, n_images, n_obs, seed):
    rng = np.random.default_rng(seed)
    n_pts = 100000
    xyz = np.column_stack((rng.uniform(-3, 3, n_pts), rng.uniform(-3, 3, n_pts), rng.uniform(2, 12, n_pts)))
    ids = np.arange(1, n_pts + 1, dtype=np.int64)
    cams = {1: gio.ColmapCamera(1, "PINHOLE", 1008, 756, np.array([800.0, 800.0, 504.0, 378.0]))}
    images, maps = {}, {}
    for k in range(n_images):
        q = rng.normal(size=4) * 0.05 + np.array([1.0, 0, 0, 0])
        q /= np.linalg.norm(q)
        xys = np.column_stack((rng.uniform(0, 1008, n_obs), rng.uniform(0, 756, n_obs)))
        images[k + 1] = gio.ColmapImage(k + 1, q, rng.uniform(-0.2, 0.2, 3), 1, "im%04d.jpg" % k, xys,
                                        rng.integers(-1, n_pts + 1, n_obs).astype(np.int64))
        maps["im%04d" % k] = rng.integers(0, 65536, size=(189, 252)).astype(np.uint16)
    return images, cams, xyz, ids, maps


def main(out_path):
    import ctypes as C

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "depth_priors_timing needs the GPU"
    from gsplat_amd import depth_priors as dp
    from gsplat_amd import io as gio
    from gsplat_amd._lib import hip_api
    api = hip_api()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("depth priors from files: median ms (spread = max - min) over %d windows after one warm-up; host clock for whole calls, "
        "device events over windows of at least %.2f s for the kernels alone; %d torch threads"
        % (REPS, WINDOW_S, torch.get_num_threads()))
    for n_images, n_obs in SCENES:
        images, cams, xyz, ids, maps = scene(np, gio, n_images, n_obs, 10 + n_images)
        host = host_clock(lambda: dp.depth_scales(images, cams, xyz, ids, maps))
        call = host_clock(lambda: dp.depth_scales(images, cams, xyz, ids, maps, on_device=True))
        table = dp.dense_point_table(xyz, ids)
        items = [(im, cams[1], maps[dp.image_key(im.name)]) for im in images.values()]
        t, total, dtype = dp.pack_device_inputs(items, table, dev)
        nb = int(api.raw("depth_scales_tmp_bytes")(total))
        tmp = torch.empty((nb,), dtype=torch.uint8, device=dev)
        out = torch.empty((n_images, 8), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        kern = device_events(torch, lambda: api.call(
            "depth_scales", t["table"].data_ptr(), len(table), t["ids"].data_ptr(), t["xys"].data_ptr(), total, t["seg"].data_ptr(),
            t["cams"].data_ptr(), t["ptrs"].data_ptr(), t["hw"].data_ptr(), dtype, 5, n_images, tmp.data_ptr(), nb, out.data_ptr(),
            stream))
        a = dp.depth_scales(images, cams, xyz, ids, maps, return_stats=True)
        b = dp.depth_scales(images, cams, xyz, ids, maps, on_device=True, return_stats=True)
        worst = max(abs(a[k]["scale"] - b[k]["scale"]) / abs(a[k]["scale"]) for k in a if a[k]["scale"] != 0)
        same = sum(a[k]["n_valid"] == b[k]["n_valid"] and a[k]["t_colmap"] == b[k]["t_colmap"] and a[k]["t_mono"] == b[k]["t_mono"]
                   for k in a)
        say("  depth_scales %3d images x %5d observations   host %9.3f ms (spread %.3f)   device, call %9.3f ms (spread %.3f)   "
            "device, kernel %8.4f ms (spread %.4f, %d calls a window)   counts and medians equal on %d of %d images, "
            "worst relative scale distance %.2e" % (n_images, n_obs, host[0], host[1], call[0], call[1], kern[0], kern[1], kern[2],
                                                     same, len(a), worst))
    src = np.random.default_rng(4).integers(0, 65536, size=(1200, 1600)).astype(np.uint16)
    src_dev = torch.from_numpy(src.view(np.int16)).to(dev)
    entry = dict(scale=1.25, offset=0.125, med_scale=1.0)
    for size in ((1600, 1200), (800, 600)):
        host = host_clock(lambda: dp.prepare_invdepth(src, size, entry))
        call = host_clock(lambda: dp.prepare_invdepth(src, size, entry, device=dev), sync=torch.cuda.synchronize)
        kern = device_events(torch, lambda: dp.prepare_invdepth(src_dev, size, entry))
        differ = int((dp.prepare_invdepth(src_dev, size, entry)[0].cpu() != dp.prepare_invdepth(src, size, entry)[0]).sum())
        say("  prepare_invdepth 1600 x 1200 -> %4d x %4d       host %9.3f ms (spread %.3f)   device, call %9.3f ms (spread %.3f)   "
            "device, kernel %8.4f ms (spread %.4f, %d calls a window)   pixels differing %d"
            % (size[0], size[1], host[0], host[1], call[0], call[1], kern[0], kern[1], kern[2], differ))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "depth_priors_timing.txt")
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        out = sys.argv[2]
    main(out)

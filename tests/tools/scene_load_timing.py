"""Developer tool: what loading a scene's images costs, host path against device call (gsplat_amd/imageio.py::ingest_image,
csrc/gs_image_ingest.hip) - the measurement behind what Scene(ingest="auto") means (gsplat_amd/scene.py::AUTO_INGEST).

  per image, bytes already decoded (a uint8 array in host memory), until the camera's two tensors are in device memory:
    host    ingest_image on the array (numpy), then the two fp32 results copied to the device
    device  the bytes copied to the device, then ingest_image there (at most two launches)
  at two shapes: 4946 x 3286 RGB -> 1600 x 1063 (a Mip-NeRF 360 photograph at -r -1) and 800 x 800 RGBA composited onto white
  at its own size (a NeRF-synthetic frame).  Beside them the device call alone (bytes already on the device), by device events.
  the whole Scene(...) of a written NeRF-synthetic-like scene: 24 RGBA frames of 800 x 800 as PNG, transforms_train.json, white
  background - reading and decoding the files included - with ingest="host" and ingest="device".

Host clock around work that ends in a device synchronise; both sides alternate inside each of WINDOWS = 5 windows; median and
spread (max - min) over the windows.  The results of the two sides are compared bit for bit before anything is timed.  Nothing is
asserted about speed.  Writes to stdout and to --out (default profiles/scene_load_timing.txt)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))

WINDOWS = 5
SHAPES = (("4946 x 3286 RGB -> 1600 x 1063", (3286, 4946, 3), None, 1),
          ("800 x 800 RGBA, composite onto white, same size", (800, 800, 4), True, 8))


def median_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def main(out_path):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "scene_load_timing needs the GPU"
    from gsplat_amd import imageio, scene
    dev = torch.device("cuda:0")
    lines = ["scene load: median ms (spread = max - min over %d windows, host and device alternating inside a window), host clock "
             "to a device synchronise" % WINDOWS]

    def host(u8, size, wb):
        out = [torch.from_numpy(a).to(dev) for a in imageio.ingest_image(u8, size, white_background=wb)]
        torch.cuda.synchronize()
        return out

    def device(u8, size, wb):
        out = imageio.ingest_image(torch.from_numpy(u8).to(dev), size, white_background=wb)
        torch.cuda.synchronize()
        return out

    for label, shape, wb, per_window in SHAPES:
        u8 = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
        size = scene.image_resolution(shape[1], shape[0], -1)
        a, b = host(u8, size, wb), device(u8, size, wb)   # (warm-up of both, and the parity the timing rests on)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "host and device ingest differ"
        times = {"host": [], "device": []}
        for _ in range(WINDOWS):
            for name, fn in (("host", host), ("device", device)):
                t0 = time.perf_counter()
                for _ in range(per_window):
                    fn(u8, size, wb)
                times[name].append((time.perf_counter() - t0) * 1e3 / per_window)
        on_dev = torch.from_numpy(u8).to(dev)
        ev = []
        for _ in range(WINDOWS):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                imageio.ingest_image(on_dev, size, white_background=wb)
            e.record()
            torch.cuda.synchronize()
            ev.append(s.elapsed_time(e) / 20)
        (hm, hs), (dm, ds), (km, ks) = median_spread(times["host"]), median_spread(times["device"]), median_spread(ev)
        lines.append("  %-48s host %9.3f ms (spread %.3f)   device %8.3f ms (spread %.3f)   kernels alone %7.4f ms (spread %.4f)"
                     % (label, hm, hs, dm, ds, km, ks))

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "frames")
        os.makedirs(src)
        rng = np.random.default_rng(2)
        frames = []
        for i in range(24):
            y, x = np.mgrid[0:800, 0:800]
            img = np.stack([(x + 7 * i) & 255, (y + 3 * i) & 255, (x + y) & 255, np.where((x - 400) ** 2 + (y - 400) ** 2 < 300 ** 2, 255, 0)],
                           axis=2).astype(np.uint8)
            img[:, :, :3] ^= rng.integers(0, 8, size=(800, 800, 3), dtype=np.uint8)
            imageio.write_png(os.path.join(src, "r_%d.png" % i), img)
            frames.append({"file_path": "./r_%d" % i,
                           "transform_matrix": [[1, 0, 0, 0.1 * i], [0, 1, 0, 0.0], [0, 0, 1, 4.0], [0, 0, 0, 1]]})
        with open(os.path.join(src, "transforms_train.json"), "w") as fp:
            json.dump({"camera_angle_x": 0.69, "frames": frames}, fp)
        from gsplat_amd._lib import hip_api

        def load(how, k):
            p = argparse.Namespace(source_path=src, model_path=os.path.join(tmp, "m_%s_%d" % (how, k)), images="images", depths="",
                                   resolution=-1, white_background=True, train_test_exp=False, eval=False, n_views=0,
                                   point_cloud_type="dense")
            t0 = time.perf_counter()
            sc = scene.Scene(p, dev, api=hip_api(), ingest=how)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, sc
        (_, a), (_, b) = load("host", -1), load("device", -1)
        assert all(torch.equal(x, y) for x, y in zip(a.gt_images[1.0], b.gt_images[1.0])), "host and device scenes differ"
        del a, b
        times = {"host": [], "device": []}
        for k in range(WINDOWS):
            for how in ("host", "device"):
                times[how].append(load(how, k)[0])
        (hm, hs), (dm, ds) = median_spread(times["host"]), median_spread(times["device"])
        lines.append("  Scene(...) of 24 RGBA PNG frames of 800 x 800, white background (files read and decoded, 100 000 points): "
                     "ingest=host %9.1f ms (spread %.1f)   ingest=device %9.1f ms (spread %.1f)" % (hm, hs, dm, ds))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_load_timing.txt"))
    main(ap.parse_args().out)

"""Developer tool: what one densification costs on one MI355X, host path against device path.

GaussianModelLite.densify_and_prune on synthetic.trained_like at P = 1 000 000 and P = 10 000, spatial_order on and off, with
statistics and thresholds that clone, split and prune a few per cent of the rows each (the counts are printed):
    host    the torch expressions with their host read-backs (on_device=False: the parent commit's code, the baseline)
    device  the kernels of csrc/gs_densify.hip (on_device=True): one read-back, one gather pass
A HOST clock around the call and a torch.cuda.synchronize() - the host waits are the point -, on a fresh copy of the same model
every time (restored outside the timed window), the two forms alternating, REPS repetitions after WARMUP; median and spread
(max - min).  Beside them: the amortised cost per train step at densification_interval = 100, and the gather's compulsory
traffic, 1 416 B per output row (parameters + two moments of 59 floats, read and written), over 8 TB/s.  Nothing is asserted.
Writes to stdout (kept as profiles/densify_timing.txt).

Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/densify_timing.py --trace DIR
    python tests/tools/densify_timing.py --kernels DIR
--trace enqueues TRACE_CALLS device densifications at P = 1 000 000 (spatial order on) and leaves their P2 in DIR; --kernels reads the profiler's kernel
table and prints the average time of each kernel of csrc/gs_densify.hip, the gather's against 1 416 B x P2 / 8 TB/s."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1_000_000, 10_000)
WARMUP, REPS = 2, 11
INTERVAL = 100
HBM = 8e12
ROW_BYTES = 2 * 3 * 59 * 4   # 1 416
MAX_GRAD, MIN_OPACITY, SCREEN, N = 0.92, 0.03, 20, 2
TRACE_P, TRACE_CALLS = 1_000_000, 5
KERNELS = ("densify_plan_kernel", "densify_scan_kernel", "densify_emit_kernel", "morton_codes_kernel", "densify_gather_kernel")


class Case:
    """One model and the state a repetition starts from."""

    def __init__(self, torch, api, P, spatial_order):
        from gsplat_amd import synthetic
        from gsplat_amd.trainer import GaussianModelLite
        from simple_knn._C import distCUDA2
        self.torch = torch
        dev = torch.device("cuda:0")
        sc = synthetic.trained_like(P, seed=0, knn=lambda x: distCUDA2(x.to(dev)).cpu())
        m = GaussianModelLite(sc, dev, api=api, spatial_order=spatial_order)
        g = torch.Generator().manual_seed(P)
        n = m.flat.numel()
        self.m, self.P = m, P
        self.flat = m.flat.detach().clone()
        self.exp_avg = (torch.randn(n, generator=g) * 1e-3).to(dev)
        self.exp_avg_sq = (torch.rand(n, generator=g) * 1e-6).to(dev)
        self.accum = torch.rand((P, 1), generator=g).to(dev)   # g = accum / 1 >= 0.92 for 8 % of the rows
        # half of the rows count as small: clones and splits share the selected rows
        max_scale = torch.exp(m.params["scaling"].detach()).max(dim=1).values
        self.extent = float(max_scale.median()) / m.percent_dense

    def restore(self):
        torch, m = self.torch, self.m
        with torch.no_grad():
            m._allocate(self.P)
            m.flat.copy_(self.flat)
            m.optimizer.alloc_moments()
            m.optimizer.exp_avg.copy_(self.exp_avg)
            m.optimizer.exp_avg_sq.copy_(self.exp_avg_sq)
        m.xyz_gradient_accum = self.accum.clone()
        m.denom = torch.ones_like(self.accum)
        m.max_radii2D = torch.zeros((self.P,), device=m.device)
        torch.cuda.synchronize()

    def run(self, on_device):
        torch = self.torch
        self.restore()
        gen = torch.Generator().manual_seed(1)
        t0 = time.perf_counter()
        out = self.m.densify_and_prune(MAX_GRAD, MIN_OPACITY, self.extent, SCREEN, None, generator=gen, N=N, on_device=on_device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out, self.m.P


def main():
    import torch
    assert torch.cuda.is_available(), "densify_timing needs the GPU"
    from gsplat_amd import hip_backend
    api = hip_backend().api
    print("densify_and_prune: host clock around the call + synchronize, ms; median (spread = max - min) of %d repetitions, "
          "forms alternating, fresh copy of the model each time" % REPS)
    for P in SIZES:
        for so in (True, False):
            case = Case(torch, api, P, so)
            forms = (("host", False), ("device", True))
            res = {}
            for name, flag in forms:
                for _ in range(WARMUP):
                    _, res[name], P2 = case.run(flag)
            if res["host"] != res["device"]:   # (a row within an ulp of a threshold: torch's exp / sigmoid against the kernel's)
                print("  counts differ: host %s, device %s" % (res["host"], res["device"]))
            nc, ns, npr = res["host"]
            times = {name: [] for name, _ in forms}
            for _ in range(REPS):
                for name, flag in forms:
                    times[name].append(case.run(flag)[0])
            stat = {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in times.items()}
            h, d = stat["host"], stat["device"]
            print("P = %d, spatial_order %s: %d clones (%.1f %%), %d split (%.1f %%), %d pruned (%.1f %%) -> P2 = %d"
                  % (P, "on" if so else "off", nc, 100.0 * nc / P, ns, 100.0 * ns / P, npr, 100.0 * npr / P, P2))
            print("  host   %9.3f ms (spread %.3f)   = %.4f ms per train step at densification_interval = %d"
                  % (h[0], h[1], h[0] / INTERVAL, INTERVAL))
            print("  device %9.3f ms (spread %.3f)   = %.4f ms per train step;   host / device = %.2f"
                  % (d[0], d[1], d[0] / INTERVAL, h[0] / d[0]))
            print("  gather: %.1f MB compulsory (1 416 B x P2) = %.4f ms at 8 TB/s" % (ROW_BYTES * P2 / 1e6, ROW_BYTES * P2 / HBM * 1e3))
            del case
            torch.cuda.empty_cache()


def trace(where):
    import torch
    assert torch.cuda.is_available(), "densify_timing needs the GPU"
    from gsplat_amd import hip_backend
    case = Case(torch, hip_backend().api, TRACE_P, True)
    for _ in range(TRACE_CALLS):
        _, out, P2 = case.run(True)
    print("enqueued %d device densifications at P = %d (spatial order on): %s -> P2 = %d" % (TRACE_CALLS, TRACE_P, out, P2))
    open(os.path.join(where, "densify_trace_P2.txt"), "w").write("%d\n" % P2)


def kernels(where):
    rows = []
    for path in sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True)):
        rows += list(csv.DictReader(open(path)))
    assert rows, "no kernel table under %s" % where
    p2 = [int(open(p).read()) for p in glob.glob(os.path.join(where, "**", "densify_trace_P2.txt"), recursive=True)]
    print("kernels of csrc/gs_densify.hip at P = %d (rocprofv3 --kernel-trace --stats, a run of its own, %d calls)"
          % (TRACE_P, TRACE_CALLS))
    for row in rows:
        name = next((k for k in KERNELS if k in row["Name"]), None)
        if name is None:
            continue
        avg_us = float(row["AverageNs"]) / 1e3
        line = "  %-24s %4d calls  average %9.2f us" % (name, int(row["Calls"]), avg_us)
        if name == "densify_gather_kernel" and p2:
            least_us = ROW_BYTES * p2[0] / HBM * 1e6
            line += "   P2 = %d: 1 416 B x P2 / 8 TB/s = %.2f us = %.1f %% of the kernel's time" % (p2[0], least_us, 100.0 * least_us / avg_us)
        print(line)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        trace(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        main()

"""Developer tool: what one FSGS densification costs on one MI355X, host path against device path.

GaussianModelLite.densify_and_prune_fsgs at P = 1 000 000 and P = 10 000, spatial_order on and off, at iteration 600 (proximity
and prune both on), on the scene recipe of tests/fsgs_densify_reference.py - constant density, three classes of size - whose
extent (0.02) makes every rule select something: clone, grad split, distance split, proximity, prune (the counts are printed):
    host    the reference's statements in torch with the HIP kNN (on_device=False): every boolean index is a host stall
    device  the gs_densify_fsgs_* kernels of csrc/gs_densify.hip (on_device=True): three read-backs, one gather pass
A HOST clock around the call and a torch.cuda.synchronize() - the host waits are the point -, on a fresh copy of the same model
every time (restored outside the timed window), the two forms alternating, REPS repetitions after WARMUP; median and spread
(max - min), and the amortised cost per train step at FSGS's densification interval of 100.  Nothing is asserted.

Every case runs in a child process of its own under a time limit (CASE_LIMIT seconds); the first case that fails or runs out
of time ends the tool, nothing further is started.  Writes to stdout (kept as profiles/fsgs_densify_timing.txt)."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1_000_000, 10_000)
WARMUP, REPS = 2, 7
INTERVAL = 100
ITERATION, N = 600, 2
CASE_LIMIT = 240


class Case:
    """One model and the state a repetition starts from."""

    def __init__(self, torch, api, P, spatial_order):
        import fsgs_densify_reference as fr
        from gsplat_amd.trainer import GaussianModelLite
        self.torch, self.fr = torch, fr
        dev = torch.device("cuda:0")
        m = GaussianModelLite(fr._scene(P, fr.SEED), dev, api=api, spatial_order=spatial_order)
        g = torch.Generator().manual_seed(P)
        n = m.flat.numel()
        self.m, self.P = m, P
        self.flat = m.flat.detach().clone()
        self.exp_avg = (torch.randn(n, generator=g) * 1e-3).to(dev)
        self.exp_avg_sq = (torch.rand(n, generator=g) * 1e-6).to(dev)
        self.accum = (torch.rand((P, 1), generator=g) * 2.4e-4).to(dev)   # g = accum / 1 >= MAX_GRAD for one row in six

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
        torch, fr = self.torch, self.fr
        self.restore()
        gen = torch.Generator().manual_seed(1)
        t0 = time.perf_counter()
        out = self.m.densify_and_prune_fsgs(fr.MAX_GRAD, fr.MIN_OPACITY, fr.EXTENT, None, ITERATION, generator=gen, N=N,
                                            on_device=on_device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out, self.m.P


def one_case(P, so):
    import torch
    assert torch.cuda.is_available(), "fsgs_densify_timing needs the GPU"
    from gsplat_amd import hip_backend
    case = Case(torch, hip_backend().api, P, so)
    forms = (("host", False), ("device", True))
    res = {}
    for name, flag in forms:
        for _ in range(WARMUP):
            _, res[name], P2 = case.run(flag)
    if res["host"] != res["device"]:   # (a row within an ulp of a threshold, or two neighbours within an ulp of each other)
        print("  counts differ: host %s, device %s" % (res["host"], res["device"]))
    nc, ns, npx, npr = res["device"]
    times = {name: [] for name, _ in forms}
    for _ in range(REPS):
        for name, flag in forms:
            times[name].append(case.run(flag)[0])
    stat = {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in times.items()}
    h, d = stat["host"], stat["device"]
    print("P = %d, spatial_order %s: %d clones (%.1f %%), %d split (%.1f %%), %d proximity rows (%.1f %%), %d pruned (%.1f %%) "
          "-> P2 = %d" % (P, "on" if so else "off", nc, 100.0 * nc / P, ns, 100.0 * ns / P, npx, 100.0 * npx / P, npr,
                          100.0 * npr / P, P2))
    print("  host   %9.3f ms (spread %.3f)   = %.4f ms per train step at densification_interval = %d"
          % (h[0], h[1], h[0] / INTERVAL, INTERVAL))
    print("  device %9.3f ms (spread %.3f)   = %.4f ms per train step;   host / device = %.2f"
          % (d[0], d[1], d[0] / INTERVAL, h[0] / d[0]))
    # for scale: the two kNN searches both forms pay - here on the model's P centres (kNN #1 sees P + clones) and on the
    # densified model's P2 centres with indices (kNN #2 sees the set in front of proximity and the final prune)
    from gsplat_amd.knn import dist2, dist2_with_indices
    case.run(True)
    api = case.m.optimizer.api
    sets = (("P centres, distances only", dist2, case.flat[:3 * P].view(P, 3)),
            ("P2 centres, with indices ", dist2_with_indices, case.m.params["xyz"].detach()))
    for what, fn, pts in sets:
        t = []
        for _ in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(api, pts)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t = sorted(t[WARMUP:])
        print("  kNN alone, %s: %9.3f ms (spread %.3f)" % (what, t[len(t) // 2], t[-1] - t[0]))


def main():
    print("densify_and_prune_fsgs at iteration %d: host clock around the call + synchronize, ms; median (spread = max - min) of %d "
          "repetitions, forms alternating, fresh copy of the model each time" % (ITERATION, REPS), flush=True)
    for P in SIZES:
        for so in (True, False):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(P), "1" if so else "0"],
                                    timeout=CASE_LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("P = %d, spatial_order %s: ended with status %d - nothing further is started" % (P, "on" if so else "off", rc))
                return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--case":
        one_case(int(sys.argv[2]), sys.argv[3] == "1")
    else:
        sys.exit(main())

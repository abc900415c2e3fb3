"""Developer tool: three per-Gaussian pieces of a DNGaussian training step at P = 100 000 and P = 1 000 000, each in two forms
in the same process on the same GPU:
    fused        the dng_reg package (csrc/gs_dng_reg.hip)
    composition  the chain of small torch kernels the training scripts run today, written from the same formulas in fp32 on
                 the device: max / min / ratio / square / means and two boolean-index gathers (a blocking nonzero each) for the
                 regulariser (after exp and sigmoid for the raw form), repeat / subtract / norm / divide for the directions,
                 a Python loop over the K = 120 camera centres for the mask
    regulariser, regulariser raw, view_dirs: forward + backward;  near mask: forward (it has no backward).
Device events around ITERS calls, after warm-up, REPS repetitions with the forms alternating; median and spread (max - min)
of the per-call time.  Nothing is asserted.  Beside each fused time: the bytes its kernels move (computed from the shapes:
regulariser 16 B per row forward + 32 backward, directions 24 + 36, mask 13 + 12 K per workgroup) over the CALL's time, as a
fraction of 6.3 TB/s - an end-to-end rate that includes the launches and torch's autograd glue, not a kernel's share of peak.
A pass of its own, after the timed ones, counts device activities (kernels, copies, fills) per call with torch.profiler.
Writes to stdout (kept as profiles/dng_reg_timing.txt).

Kernel times and each kernel's share of the HBM rate come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/dng_reg_timing.py --trace
    python tests/tools/dng_reg_timing.py --kernels DIR
--trace enqueues TRACE_CALLS fused calls of each piece at P = 1 000 000 and nothing else of this library; --kernels reads the
profiler's kernel table and prints, per kernel of csrc/gs_dng_reg.hip, its average time and the bytes it moves over that time
as a fraction of 6.3 TB/s (the achievable rate; every one of these kernels is bound by bytes, not by operations)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (100_000, 1_000_000)
K, NEAR = 120, 0.5
ITERS, WARMUP, REPS, COUNT_CALLS = 200, 10, 11, 5
MASK_CHAIN_ITERS = 10   # the composition's mask is ~5 K launches per call
HBM = 6.3e12
TRACE_P, TRACE_CALLS = 1_000_000, 20
# bytes per row each kernel moves (reads + writes); the finishing kernel reads one 48-byte partial per workgroup
KERNEL_ROW_BYTES = {"dr_stats_kernel": 16, "dr_bwd_kernel": 32, "vd_fwd_kernel": 24, "vd_bwd_kernel": 36, "nm_kernel": 13}


def per_call_ms(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def forms(torch, P):
    """-> [(name, fused, composition, bytes the fused kernels move, composition calls per timing)]"""
    import dng_reg
    import dng_reg_reference as ref
    dev = torch.device("cuda:0")
    s64, o64 = ref.scene(4096, "mixed", seed=1)
    reps = (P + 4095) // 4096
    s = s64.float().repeat(reps, 1)[:P].to(dev).requires_grad_(True)
    o = o64.float().repeat(reps)[:P].reshape(P, 1).to(dev).requires_grad_(True)
    rs = s.detach().log().requires_grad_(True)
    ro = torch.logit(o.detach()).requires_grad_(True)
    g = torch.Generator().manual_seed(P)
    xyz = (torch.rand((P, 3), generator=g) * 5 - 2.5).to(dev).requires_grad_(True)
    centers = (torch.rand((K, 3), generator=g) * 4 - 2).to(dev)
    campos = centers[0].clone()
    gdirs = torch.randn((P, 3), generator=g).to(dev)
    w = ref.WEIGHTS

    def chain(sc, op):
        shape = (sc.max(dim=1).values / sc.min(dim=1).values).mean()
        scale = (sc.max(dim=1, keepdim=True).values ** 2).mean()
        opa = 1 - (op[op > 0.2] ** 2).mean() + ((1 - op[op < 0.2]) ** 2).mean()
        return w[0] * shape + w[1] * scale + w[2] * opa

    def reg_fused():
        s.grad = o.grad = None
        dng_reg.gaussian_regulariser(s, o).backward()

    def reg_chain():
        s.grad = o.grad = None
        chain(s, o).backward()

    def raw_fused():
        rs.grad = ro.grad = None
        dng_reg.gaussian_regulariser_raw(rs, ro).backward()

    def raw_chain():
        rs.grad = ro.grad = None
        chain(torch.exp(rs), torch.sigmoid(ro)).backward()

    def dirs_fused():
        xyz.grad = None
        dng_reg.view_dirs(xyz, campos).backward(gdirs)

    def dirs_chain():
        xyz.grad = None
        d = xyz - campos.repeat(P, 1)
        (d / d.norm(dim=1, keepdim=True)).backward(gdirs)

    def mask_fused():
        dng_reg.near_camera_mask(xyz, centers, NEAR)

    def mask_chain():
        x = xyz.detach()
        m = None
        for k in range(K):
            t = (x - centers[k].repeat(P, 1)).norm(dim=1, keepdim=True) < NEAR
            m = m + t if m is not None else t
        return m.squeeze()

    blocks = (P + 1023) // 1024
    return [("regulariser", reg_fused, reg_chain, 48 * P, ITERS), ("regulariser raw", raw_fused, raw_chain, 48 * P, ITERS),
            ("view_dirs", dirs_fused, dirs_chain, 60 * P, ITERS), ("near mask K=120", mask_fused, mask_chain, 13 * P + 12 * K * blocks,
                                                                   MASK_CHAIN_ITERS)]


def kernels_per_call(torch, fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(COUNT_CALLS):
            fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n / COUNT_CALLS


def main():
    import torch
    assert torch.cuda.is_available(), "dng_reg_timing needs the GPU"
    print("per call: median ms (spread = max - min over %d repetitions of %d calls; the near mask's composition: %d calls)"
          % (REPS, ITERS, MASK_CHAIN_ITERS))
    counted = []
    for P in SIZES:
        print("P = %d" % P)
        for name, fused, comp, nbytes, iters in forms(torch, P):
            fs = (("fused", fused, ITERS), ("composition", comp, iters))
            for _, fn, it in fs:
                for _ in range(WARMUP if it == ITERS else 2):
                    fn()
            times = {n: [] for n, _, _ in fs}
            for _ in range(REPS):
                for n, fn, it in fs:
                    times[n].append(per_call_ms(torch, fn, it))
            stat = {n: (sorted(v)[len(v) // 2], max(v) - min(v)) for n, v in times.items()}
            f, c = stat["fused"], stat["composition"]
            print("  %-16s fused %9.4f ms (spread %.4f)   composition %9.4f ms (spread %.4f)   composition / fused = %.2f"
                  % (name, f[0], f[1], c[0], c[1], c[0] / f[0]))
            print("  %-16s the fused kernels move %.2f MB: %.1f %% of 6.3 TB/s over the call's time"
                  % ("", nbytes / 1e6, 100.0 * nbytes / (f[0] * 1e-3) / HBM))
            if P == SIZES[0]:
                counted.append((name, fused, comp))
    print("device activities (kernels, copies, fills) per call (torch.profiler, a pass of its own, P = %d; torch's glue included: the gradient seed of "
          "backward(), the [P,1] views' copies)" % SIZES[0])
    for name, fused, comp in counted:
        try:
            print("  %-16s fused %6.1f   composition %6.1f" % (name, kernels_per_call(torch, fused), kernels_per_call(torch, comp)))
        except Exception as e:  # the profiler is a convenience here; the times above do not depend on it
            print("  %-16s not counted: %s: %s" % (name, type(e).__name__, e))


def trace():
    import torch
    assert torch.cuda.is_available(), "dng_reg_timing needs the GPU"
    fs = forms(torch, TRACE_P)
    for _ in range(TRACE_CALLS):
        for _, fused, _, _, _ in fs:
            fused()
    torch.cuda.synchronize()
    print("enqueued %d fused calls of each piece at P = %d" % (TRACE_CALLS, TRACE_P))


def kernels(where):
    rows = []
    for path in sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True)):
        rows += list(csv.DictReader(open(path)))
    assert rows, "no kernel table under %s" % where
    print("kernels of csrc/gs_dng_reg.hip at P = %d (rocprofv3 --kernel-trace --stats, a run of its own, %d calls of each piece)"
          % (TRACE_P, TRACE_CALLS))
    for row in rows:
        name = next((k for k in list(KERNEL_ROW_BYTES) + ["dr_finish_kernel"] if k in row["Name"]), None)
        if name is None:
            continue
        avg_us = float(row["AverageNs"]) / 1e3
        if name == "dr_finish_kernel":
            print("  %-18s %4d calls  average %8.2f us  (one workgroup, %d partials of 48 B)"
                  % (name, int(row["Calls"]), avg_us, min((TRACE_P + 1023) // 1024, 1024)))
            continue
        nbytes = KERNEL_ROW_BYTES[name] * TRACE_P + (12 * K * ((TRACE_P + 1023) // 1024) if name == "nm_kernel" else 0)
        print("  %-18s %4d calls  average %8.2f us  %6.2f MB  = %5.1f %% of 6.3 TB/s"
              % (name, int(row["Calls"]), avg_us, nbytes / 1e6, 100.0 * nbytes / (avg_us * 1e-6) / HBM))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
    elif len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        main()

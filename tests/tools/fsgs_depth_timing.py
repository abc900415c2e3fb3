"""Developer tool: the depth-correlation term of an FSGS training step (FSGS/train.py:105-108), forward plus backward, at
378x504 and 1080x1920, in two forms in the same process on the same GPU:
    fused        fsgs_loss.depth_pearson_loss (csrc/gs_pearson.hip): two launches forward, one backward, branch on the device
    composition  tests/fsgs_loss_reference.py run in fp32 on the device - the chain of small torch reductions torchmetrics'
                 pearson_corrcoef amounts to, twice, and Python's min over the two device scalars (a blocking read-back).
                 This is the baseline: what an FSGS user runs today.
Device events around ITERS calls, after warm-up, REPS repetitions with the forms alternating; median and spread (max - min)
of the per-call time.  Nothing is asserted; where the fused form does not beat the composition by more than the two spreads
combined, the line says so.  Writes to stdout (kept as profiles/fsgs_depth_timing.txt).

Launch counts come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/fsgs_depth_timing.py --trace
    python tests/tools/fsgs_depth_timing.py --launches DIR
--trace enqueues TRACE_CALLS fused forward + backward calls and nothing else that launches a kernel of this library;
--launches reads the profiler's kernel tables and prints launches per call."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((378, 504), (1080, 1920))
ITERS, WARMUP, REPS, TRACE_CALLS = 20, 10, 21, 10


def per_call_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def forms(torch, H, W):
    import fsgs_loss
    import fsgs_loss_reference as ref
    dev = torch.device("cuda:0")
    depth, midas = ref.scene(H, W, "A", seed=H + W, dtype=torch.float32)
    x = depth.to(dev).requires_grad_(True)
    m = midas.to(dev)

    def fused():
        x.grad = None
        fsgs_loss.depth_pearson_loss(x, m).backward()

    def composition():
        x.grad = None
        ref.depth_pearson_loss(x, m).backward()

    return (("fused", fused), ("composition", composition))


def time_all():
    import torch
    assert torch.cuda.is_available(), "fsgs_depth_timing needs the GPU"
    print("depth_pearson_loss, forward + backward, per call: median ms (spread = max - min over %d repetitions of %d calls)"
          % (REPS, ITERS))
    for H, W in SIZES:
        fs = forms(torch, H, W)
        for _, fn in fs:
            for _ in range(WARMUP):
                fn()
        times = {name: [] for name, _ in fs}
        for _ in range(REPS):
            for name, fn in fs:
                times[name].append(per_call_ms(torch, fn))
        stat = {}
        for name, v in times.items():
            v = sorted(v)
            stat[name] = (v[len(v) // 2], v[-1] - v[0])
        print("%dx%d" % (H, W))
        for name, _ in fs:
            print("  %-12s %8.4f ms  (spread %.4f)" % (name, *stat[name]))
        gain = stat["composition"][0] - stat["fused"][0]
        noise = stat["composition"][1] + stat["fused"][1]
        verdict = "beats the composition by more than the two spreads" if gain > noise else \
            "does NOT beat the composition by more than the two spreads"
        print("  fused %s: %.4f ms faster, spreads combined %.4f ms, composition / fused = %.2f"
              % (verdict, gain, noise, stat["composition"][0] / stat["fused"][0]))


def trace():
    import torch
    assert torch.cuda.is_available(), "fsgs_depth_timing needs the GPU"
    fused = forms(torch, *SIZES[0])[0][1]
    for _ in range(TRACE_CALLS):
        fused()
    torch.cuda.synchronize()
    print("enqueued %d fused forward + backward calls at %dx%d" % (TRACE_CALLS, *SIZES[0]))


def launches(where):
    counts = {}
    for path in sorted(glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            name = row.get("Kernel_Name") or row.get("Name") or ""
            counts[name] = counts.get(name, 0) + 1
    if not counts:
        for path in sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True)):
            for row in csv.DictReader(open(path)):
                counts[row["Name"]] = counts.get(row["Name"], 0) + int(row["Calls"])
    assert counts, "no kernel table under %s" % where
    print("kernel launches over %d fused forward + backward calls (a run of its own under the profiler)" % TRACE_CALLS)
    ours = {k: v for k, v in counts.items() if "pr_" in k and "_kernel" in k}
    for name, n in sorted(ours.items()):
        print("  %-70s %4d  = %g per call" % (name[:70], n, n / TRACE_CALLS))
    fwd = sum(n for k, n in ours.items() if "pr_stats" in k or "pr_finish" in k)
    bwd = sum(n for k, n in ours.items() if "pr_bwd" in k)
    print("  gs_pearson kernels per call: %g forward, %g backward" % (fwd / TRACE_CALLS, bwd / TRACE_CALLS))
    other = sum(counts.values()) - sum(ours.values())
    print("  every other kernel in the trace (torch: input upload, the gradient seed of backward()): %d = %g per call"
          % (other, other / TRACE_CALLS))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
    elif len(sys.argv) > 2 and sys.argv[1] == "--launches":
        launches(sys.argv[2])
    else:
        time_all()

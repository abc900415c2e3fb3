"""Developer tool: DNGaussian's two neural heads (sigma_net 32-64-64-65, color_net 80-64-3, sigmoid), forward plus backward
with gradients to both encodings and all five weights, at B = 100 000 and 1 000 000 rows, in two forms in the same process on
the same GPU:
    fused        gsplat_amd.neural.dng_heads (csrc/gs_mlp.hip): one MFMA launch forward, one plus a reduction backward
    torch chain  tests/neural_reference.py torch_chain in fp32 on the device - the Linear / relu / cat / slice / sigmoid
                 statements of tests/test_gpu_encoding.py's neural chain.  This is the baseline: what a user ran before.
Device events around ITERS calls, after warm-up, REPS repetitions with the forms alternating; median and spread (max - min)
of the per-call time.  Both forms are first compared on the timed inputs with each other and with the float64 restatement
(tests/neural_reference.py heads_ref) evaluated on the device: per tensor the error relative to the tensor's largest entry and,
for the per-row tensors, how many ROWS are further than 1e-4 of that entry from the float64 row.  At a million rows expect a
handful of such rows in the input gradients of either fp32 form: a hidden pre-activation within fp32 rounding of 0 lands on
either side of ReLU's kink depending on the order of the sum.
The achieved fraction of the 157 TF f32 matrix peak counts 3 x 2 x 15 616 flop per row (forward, and twice that backward)
over the CALL time - an end-to-end figure, not a kernel's share of peak.  Nothing is asserted; where the fused form does not
beat the chain by more than the two spreads combined, the line says so.  Writes to stdout (kept as
profiles/neural_heads_timing.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (100_000, 1_000_000)
ITERS, WARMUP, REPS = 10, 5, 11
FLOP_PER_ROW = 3 * 2 * 15616
PEAK_F32_MATRIX = 157e12
ROW_TOL = 1e-4


def per_call_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def forms(torch, B):
    import neural_reference as ref
    from gsplat_amd import neural
    from helpers import rel_err
    dev = torch.device("cuda:0")
    t = ref.make_inputs(B, seed=B, device=dev)
    names = ("enc_x", "enc_d") + ref.NAMES
    leaf = {k: t[k].requires_grad_(True) for k in names}
    w = [leaf[n] for n in ref.NAMES]
    gout = [t["g_sigma"], t["g_color"]]

    def clear():
        for k in names:
            leaf[k].grad = None

    def fused():
        clear()
        torch.autograd.backward(list(neural.dng_heads(leaf["enc_x"], leaf["enc_d"], *w)), gout)

    def chain():
        clear()
        torch.autograd.backward(list(ref.torch_chain(leaf["enc_x"], leaf["enc_d"], w)), gout)

    o = ref.run(ref.heads_ref, t, torch.float64)
    got = {}
    for name, fn, heads in (("fused", fused, lambda: neural.dng_heads(leaf["enc_x"], leaf["enc_d"], *w)),
                            ("torch chain", chain, lambda: ref.torch_chain(leaf["enc_x"], leaf["enc_d"], w))):
        fn()
        got[name] = {"g_" + k: leaf[k].grad.clone() for k in names}
        with torch.no_grad():
            got[name]["sigma"], got[name]["color"] = heads()
    worst = max(rel_err(got["fused"][k], got["torch chain"][k]) for k in got["fused"])
    report = []
    for name in got:
        for k in ("sigma", "color", "g_enc_x", "g_enc_d") + tuple("g_" + n for n in ref.NAMES):
            a, b = got[name][k].double(), o[k]
            scale = max(1e-12, float(b.abs().max()))
            line = "  %-12s %-8s against float64: rel err %.1e" % (name, k, float((a - b).abs().max()) / scale)
            if a.shape[0] == B:
                rows = (a - b).abs().reshape(B, -1).amax(1) > ROW_TOL * scale
                line += ", rows beyond %.0e: %d of %d" % (ROW_TOL, int(rows.sum()), B)
            report.append(line)
    return (("fused", fused), ("torch chain", chain)), worst, report


def time_all():
    import torch
    assert torch.cuda.is_available(), "neural_heads_timing needs the GPU"
    print("dng_heads, forward + backward (all gradients), per call: median ms (spread = max - min over %d repetitions of %d calls)"
          % (REPS, ITERS))
    for B in SIZES:
        fs, worst, report = forms(torch, B)
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
        print("B = %d  (fused against torch chain on these inputs: largest gradient rel err %.1e)" % (B, worst))
        for name, _ in fs:
            tf = B * FLOP_PER_ROW / (stat[name][0] * 1e-3)
            print("  %-12s %8.4f ms  (spread %.4f)  %6.2f TF = %4.1f %% of the 157 TF f32 matrix peak"
                  % (name, *stat[name], tf / 1e12, 100 * tf / PEAK_F32_MATRIX))
        print("\n".join(report))
        gain = stat["torch chain"][0] - stat["fused"][0]
        noise = stat["torch chain"][1] + stat["fused"][1]
        verdict = "beats the torch chain by more than the two spreads" if gain > noise else \
            "does NOT beat the torch chain by more than the two spreads"
        print("  fused %s: %.4f ms faster, spreads combined %.4f ms, torch chain / fused = %.2f"
              % (verdict, gain, noise, stat["torch chain"][0] / stat["fused"][0]))


if __name__ == "__main__":
    time_all()

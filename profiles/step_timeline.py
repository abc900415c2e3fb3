#!/usr/bin/env python3
"""One steady-state train step out of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 bench.py ...` run,
with what summarize.py's timeline leaves out: every launch in start order with its start (us from the step's first kernel), its
duration and its queue, so that which kernels lay beside which can be read off.
usage: python profiles/step_timeline.py DIR OUT.txt"""
import csv
import glob
import os
import sys

src, out = sys.argv[1], sys.argv[2]
trace = glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True)[0]
tr = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))


def short(name):
    name = name.split("(")[0]
    for cut in ("void ", "(anonymous namespace)::"):
        name = name.replace(cut, "")
    return name.split("<")[0][-48:]


idx = [i for i, r in enumerate(tr) if "render_bwd_wave_kernel" in r["Kernel_Name"]]
# the two-phase steps of the timed region (the bench ends with a few one-launch steps): the one two thirds of the way through
two = [j for j in range(1, len(idx)) if any("step_uninstanced_kernel" in r["Kernel_Name"] for r in tr[idx[j - 1]:idx[j]])]
j = two[(2 * len(two)) // 3]
a, b = idx[j - 1], idx[j]
t0, t_end = int(tr[a]["Start_Timestamp"]), int(tr[b]["Start_Timestamp"])
# (a side-stream kernel issued in the previous step may still be running at t0: it belongs to this picture)
seg = [r for r in tr if int(r["End_Timestamp"]) > t0 and int(r["Start_Timestamp"]) < t_end and r is not tr[b]]
iv = sorted((max(int(r["Start_Timestamp"]), t0), min(int(r["End_Timestamp"]), t_end)) for r in seg)
busy, cs, ce = 0, None, None
for s0, e0 in iv:
    if ce is None or s0 > ce:
        busy += (ce - cs) if ce is not None else 0
        cs, ce = s0, e0
    else:
        ce = max(ce, e0)
busy += (ce - cs) if ce is not None else 0
queues = {}
with open(out, "w") as f:
    f.write("one steady-state train step (render_bwd to render_bwd), rocprofv3 --kernel-trace; start and duration in us\n")
    f.write("wall %.3f ms, GPU busy %.3f ms, %d kernel launches\n" % ((t_end - t0) / 1e6, busy / 1e6, len(seg)))
    f.write("%9s %9s %5s  %s\n" % ("start", "duration", "queue", "kernel"))
    for r in seg:
        q = queues.setdefault(r.get("Queue_Id", "?"), len(queues))
        s0, e0 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        f.write("%9.1f %9.1f %5d  %s\n" % ((s0 - t0) / 1e3, (e0 - s0) / 1e3, q, short(r["Kernel_Name"])))
print(open(out).read())

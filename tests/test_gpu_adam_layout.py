"""gs_adam_step, gs_adam_step_masked and gs_adam_step_gated at their own layout edges, through the raw C-ABI bindings, on the
hand-made case table of tests/step_reference.py (validated on the CPU oracle by tests/test_step_layout_cpu.py): sizes around
the float4 tail and the workgroup, segment edges, gaps and ends inside a float4, the learning-rate phase at every place of a
float4, row masks that alternate inside float4s, the gate, guard words around every buffer.

The arbiter is the plain restatement: exp_avg and exp_avg_sq carry its float32 bits, the parameter lies within the bar
measured on the restatement (4 x max|p32 - p64| + one ulp) - and, as it turned out on an MI355X, carries the restatement's float32
bits as well, which is asserted.  The oracle's moments are the same bits too."""
import pytest
import torch

import step_reference as sr

pytestmark = pytest.mark.gpu

CASES = sr.adam_cases()
REPORT = {}


def _call(api):
    def call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, mask):
        stream = None
        if kind == "adam_step":
            api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, stream)
        elif kind == "adam_step_gated":
            api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, stream)
        else:
            api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, mask, stream)
    return call


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hip_adam_is_the_restatement_on_the_case_table(hip, oracle, case):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.default_stream()):   # (the raw call goes to the null stream)
        out = sr.run_adam_case(case, _call(hip.api), "cuda")
    sr.check_adam_case(case, out, report=REPORT)
    ref = sr.run_adam_case(case, _call(oracle.api), "cpu")
    assert sr.same_bits(out["m"], ref["m"]) and sr.same_bits(out["v"], ref["v"]), "moments differ from the oracle's"
    if case.gate is not None and case.gate != 0.0:    # a closed gate: not a bit moves
        p, g, m, v = out["inputs"]
        assert sr.same_bits(out["p"], p) and sr.same_bits(out["m"], m) and sr.same_bits(out["v"], v)


def test_an_open_gate_is_the_ungated_call_on_the_gpu(hip):
    for n in (5, 1025):
        a = sr.AdamCase("open", n, [sr._seg(1, n - 1, 0.01, 0.002, 5, 2, step=3)], gate=0.0)
        b = sr.AdamCase("none", n, a.segs)
        oa, ob = sr.run_adam_case(a, _call(hip.api), "cuda"), sr.run_adam_case(b, _call(hip.api), "cuda")
        for k in ("p", "m", "v"):
            assert sr.same_bits(oa[k], ob[k])
    r = REPORT.get("all")
    if r:
        print("stand-alone Adam over the case table: max|p32-p64| %.3e, largest bar %.3e, largest GPU deviation %.3e, "
              "%d of %d parameters off the float32 restatement's bits" % (r["own"], r["tol"], r["dev"], r["off32"], r["n"]))

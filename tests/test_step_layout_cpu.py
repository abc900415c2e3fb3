"""Proves the arbiter of the step-layout tests (tests/step_reference.py) and their inputs without a GPU:

  * adam_ref in float64 against torch.optim.Adam itself (float64 tensors, the reference's groups, a skipped group, a sparse mask);
  * the case table of the stand-alone kernel's test, on the CPU oracle through the C ABI: m and v carry the float32
    restatement's bits, p lies within the measured bar - the table and the rule are sound before a GPU sees them;
  * the scene of the fused-step tests at every P they use: visible and invisible rows, mixed float4s."""
import numpy as np
import pytest
import torch

import step_reference as sr
from gsplat_amd.trainer import FIELDS, LRS

STEP_SIZES = (1, 2, 3, 5, 7, 253, 254, 255, 257, 514, 771, 1021, 1022, 1023)   # tests/test_gpu_step_layout.py


@pytest.mark.parametrize("sparse", [False, True], ids=["all_rows", "sparse_mask"])
@pytest.mark.parametrize("P", [7, 257])
def test_float64_restatement_is_torch_adam(P, sparse):
    """Six steps; opacity has no gradient at step 4 (a reset iteration: torch leaves the parameter, its moments and its step
    count alone).  With the mask: torch's own step, then parameter and moments of the masked-off rows put back (the masked
    restatement of tests/test_sparse_adam.py).  Agreement to float64 rounding: torch forms m by lerp and the update by
    addcdiv, a handful of roundings of 1.1e-16 each per step - held to 1e-13 of max(1, |x|) after six steps."""
    g = torch.Generator().manual_seed(P)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    params = {k: torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True) for k, s in shapes.items()}
    opt = torch.optim.Adam([{"params": [params[k]], "lr": LRS[k], "name": k} for k in sr.GROUPS], lr=0.0, eps=1e-15)

    def flat(get):
        feat = torch.cat((get("f_dc"), get("f_rest")), dim=1)
        parts = {"xyz": get("xyz"), "features": feat, "opacity": get("opacity"), "scaling": get("scaling"), "rotation": get("rotation")}
        return torch.cat([parts[n].reshape(-1) for n, _ in FIELDS]).detach().numpy().copy()

    def moment(which):
        def get(k):
            st = opt.state.get(params[k])
            return torch.zeros_like(params[k]) if not st else st[which]
        return get
    p = flat(lambda k: params[k])
    m, v = np.zeros_like(p), np.zeros_like(p)
    counts = {n: 0 for n, _ in FIELDS}
    n = p.size
    for it in range(1, 7):
        skip = ("opacity",) if it == 4 else ()
        grads = {k: torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
                 for k, s in shapes.items()}
        visible = (torch.rand(P, generator=g) > 0.4) if sparse else torch.ones(P, dtype=torch.bool)
        visible[0] = True
        for k in sr.GROUPS:
            params[k].grad = None if k in skip else grads[k]
        before = {k: (params[k].detach().clone(), moment("exp_avg")(k).clone(), moment("exp_avg_sq")(k).clone()) for k in sr.GROUPS}
        opt.step()
        with torch.no_grad():
            keep = ~visible
            for k in sr.GROUPS:
                if k in skip:
                    continue
                params[k][keep] = before[k][0][keep]
                opt.state[params[k]]["exp_avg"][keep] = before[k][1][keep]
                opt.state[params[k]]["exp_avg_sq"][keep] = before[k][2][keep]
        for name, _ in FIELDS:
            counts[name] += name not in skip
        lr, t, on, row = sr.element_tables(P, counts, skip)
        gflat = flat(lambda k: grads[k])
        stepped = on & visible.numpy()[row]
        p, m, v = sr.adam_ref(p, gflat, m, v, lr, t, stepped, np.float64)
        for got, want, what in ((p, flat(lambda k: params[k]), "p"), (m, flat(moment("exp_avg")), "m"), (v, flat(moment("exp_avg_sq")), "v")):
            err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
            assert err <= 1e-13, (it, what, err)
    assert counts["opacity"] == 5 and counts["xyz"] == 6 and n == 59 * P
    # the two feature rates differ by 20, and the skipped group's count lags: both are in the tables
    lo, hi, _ = sr.field_offsets(P)["features"]
    assert lr[lo] == LRS["f_dc"] and lr[lo + 3] == LRS["f_rest"] and lr[lo + 48] == LRS["f_dc"] and lr[hi - 1] == LRS["f_rest"]
    o = sr.field_offsets(P)["opacity"][0]
    assert t[o] == 5 and t[0] == 6


CASES = sr.adam_cases()


def _oracle_call(oracle):
    def call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, mask):
        if kind == "adam_step":
            oracle.api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, None)
        elif kind == "adam_step_gated":
            oracle.api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, None)
        else:
            oracle.api.call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, mask, None)
    return call


def test_case_table_covers_what_it_claims():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.n for c in CASES} == set(sr.SIZES)
    edges = {(s["end"] % 4) for c in CASES if c.name.startswith("edge_") for s in c.segs[:1]}
    assert edges == {1, 2, 3}
    assert {c.segs[0]["begin"] % 4 for c in CASES if c.name.startswith("phase48_begin")} == {0, 1, 2, 3}
    assert any(c.segs[0]["period"] % 4 for c in CASES if c.name.startswith("phase5"))
    for c in CASES:   # every segment lies inside the buffer (a negative begin is a shifted table, clipped at 0 by the kernels' i >= begin)
        assert all(s["end"] <= c.n and s["begin"] < s["end"] for s in c.segs), c.name
        if c.mask is not None:
            s = c.segs[0]
            assert s["begin"] % 4 != 0 and (s["end"] - s["begin"]) == len(c.mask) * s["row_width"]
            r = np.repeat(c.mask, s["row_width"])
            pad = np.concatenate((np.full(s["begin"], -1.0, np.float32), r))
            q = pad[: pad.size // 4 * 4].reshape(-1, 4)
            assert int(((q == 1).any(axis=1) & (q == 0).any(axis=1)).sum()) > 0, c.name   # the mask alternates inside float4s


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_adam_is_the_restatement_on_the_case_table(oracle, case):
    out = sr.run_adam_case(case, _oracle_call(oracle), "cpu")
    sr.check_adam_case(case, out)
    if case.gate is not None and case.gate != 0.0:
        p, g, m, v = out["inputs"]
        assert sr.same_bits(out["p"], p) and sr.same_bits(out["m"], m) and sr.same_bits(out["v"], v)


def test_an_open_gate_is_the_ungated_call(oracle):
    for n in (5, 1025):
        a = sr.AdamCase("open", n, [sr._seg(1, n - 1, 0.01, 0.002, 5, 2, step=3)], gate=0.0)
        b = sr.AdamCase("none", n, a.segs)
        oa, ob = sr.run_adam_case(a, _oracle_call(oracle)), sr.run_adam_case(b, _oracle_call(oracle))
        for k in ("p", "m", "v"):
            assert sr.same_bits(oa[k], ob[k])


# ------------------------------------------------------------------------------------------------------------------ the scene
@pytest.fixture(scope="module")
def views(oracle):
    """radii and tiles_touched of cameras 0..2 on the initial scene of every P, from the oracle's forward"""
    from gsplat_amd.trainer import camera_to
    from test_gpu_raster_parity import forward_state
    cams = [camera_to(c, torch.device("cpu")) for c in sr.cameras(3)]
    out = {}
    for P in STEP_SIZES:
        sc = sr.scene(P)
        out[P] = [forward_state(oracle.backend, sc, cam, torch.device("cpu"), torch.zeros(3), False) for cam in cams]
    return out


@pytest.mark.parametrize("P", STEP_SIZES)
def test_scene_has_the_rows_the_step_tests_need(views, P):
    seen_mixed_op = seen_mixed_xyz = 0
    for ci, st in enumerate(views[P]):
        vis = (st["radii"] > 0).numpy()
        inst = (st["tiles_touched"] > 0).numpy()
        print("P %d camera %d: visible %d, with instances %d" % (P, ci, int(vis.sum()), int(inst.sum())))
        assert int(vis.sum()) >= 1 and int(inst.sum()) >= 1, "camera %d sees nothing" % ci
        if P >= 253:
            assert vis.any() and (~vis).any()
            # the wall of step_reference.scene: visible Gaussians the backward blend cannot reach on the reference's own lists
            # (tests/reached_scenes.py::list_sets: no entry up to their tile's largest n_contrib) - and ones it does reach
            import reached_scenes as rs
            must, may, listed = rs.list_sets(st, P, sr.W, sr.H)
            unreached = int((torch.from_numpy(vis) & ~may).sum())
            print("   reached for certain %d, visible and unreached %d, final T %.1e .. %.1e" % (
                int(must.sum()), unreached, float(st["final_T"].min()), float(st["final_T"].max())))
            assert unreached >= 1 and int(must.sum()) >= 1
            assert float(st["final_T"].max()) > 1e-3      # (not the whole image is saturated)
        seen_mixed_op += sr.mixed_float4s(vis, 1)
        seen_mixed_xyz += sr.mixed_float4s(vis, 3)
    if P >= 2:   # (one row cannot share a float4 with a row of the other kind)
        assert seen_mixed_op >= 1 and seen_mixed_xyz >= 1


def test_scene_is_a_prefix_and_lifts_rows_1_mod_3():
    a, b = sr.scene(7), sr.scene(1023)
    assert torch.equal(a["means3D"], b["means3D"][:7]) and torch.equal(a["shs"], b["shs"][:7])
    z = b["means3D"][:, 2]
    assert bool((z[1::3] > 40).all()) and bool((z[0::3].abs() < 2).all()) and bool((z[2::3].abs() < 2).all())

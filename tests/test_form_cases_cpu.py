"""The arbiter of tests/test_gpu_input_forms.py proven in every input form before the GPU is asked anything: the CPU checker
against the float64 model (tests/dense_reference.py) on each unsplit form of tests/form_cases.py, at test_oracle_dense's bars,
in both chain modes (the fp32 transcription and Oracle.exact_chain).  Under a scale modifier the checker's dL_dscales is
the analytic gradient divided by the modifier (the reference's behaviour, form_cases.analytic)."""
import pytest
import torch

import blend_cases
import dense_reference
import depth_pass_reference as dpr
import form_cases
from helpers import run_scene
from test_oracle_dense import dense_run

CPU = torch.device("cpu")
_DENSE = {}


def dense(form):
    if form["id"] not in _DENSE:
        sc, cam = form_cases.build(form)
        dc, di = form_cases.cotangents(form)
        dn, dg = dense_run(sc, cam, form_cases.BG, form["aa"], dc, di)
        _DENSE[form["id"]] = ({k: dn[k].detach() for k in ("color", "invdepth", "radii")}, dg)
    return _DENSE[form["id"]]


@pytest.mark.parametrize("exact", [False, True], ids=["fp32_chain", "exact_chain"])
@pytest.mark.parametrize("form", form_cases.UNSPLIT, ids=lambda f: f["id"])
def test_oracle_matches_dense_float64_in_every_form(oracle, form, exact):
    sc, cam = form_cases.build(form)
    dc, di = form_cases.cotangents(form)
    with oracle.exact_chain(exact):
        o = run_scene(oracle.Rasterizer, oracle.Settings, sc, cam, CPU, bg=form_cases.BG, antialiasing=form["aa"],
                      dL_dcolor=dc, dL_dinvdepth=di)
    dn, dg = dense(form)
    P = form["P"]
    assert torch.equal(o["radii"].long(), dn["radii"].long()), "radii differ"
    visible, culled = int((o["radii"] > 0).sum()), int((o["radii"] == 0).sum())
    print("%s: %d visible, %d culled of %d" % (form["id"], visible, culled, P))
    if P >= 255:   # the form itself is a real test: every wave holds both kinds
        assert visible >= 25 and culled >= 25, (visible, culled)
    err = (o["color"].double() - dn["color"]).abs().max().item()
    assert err < 2e-5, "colour max abs err %.3e" % err
    err = (o["invdepth"].double() - dn["invdepth"]).abs().max().item()
    assert err < 2e-5 * max(1.0, dn["invdepth"].abs().max().item()), "invdepth err %.3e" % err

    og = form_cases.analytic(o["grads"], sc)
    report = {}

    def chk(name, a, b, tol=2e-4):
        a, b = a.double(), b.double()
        scale = max(b.abs().max().item(), 1e-12)
        e = (a - b).abs().max().item() / scale
        report[name] = e
        assert e < tol, "%s: rel err %.3e (scale %.3e)" % (name, e, scale)

    for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"):
        if k in og:
            assert k in dg, k
            if visible:
                assert float(dg[k].abs().max()) > 0, "%s takes no gradient: the form tests nothing" % k
            chk("dL_d" + k, og[k], dg[k])
    chk("dL_dmeans2D", og["means2D"][:, :2], dg["ndc_probe"])
    assert float(og["means2D"][:, 2].abs().max()) == 0.0
    print("%s: %s" % (form["id"], {k: "%.1e" % v for k, v in report.items()}))
    if "shs" in og:
        used = (form["D"] + 1) ** 2
        assert not og["shs"][:, used:, :].any(), "rows above the active degree take a gradient"
        assert not og["shs"][o["radii"] == 0].any(), "a culled Gaussian's rows take a gradient"
        if form["M"] > 16:
            assert not og["shs"][:, 16:, :].any() and not dg["shs"][:, 16:, :].any()
    if form["mod"] != 1.0 and "scales" in og and visible:
        # the quirk is really there: without the factor the tensor is (1 - 1 / modifier) of itself away from float64
        scale = float(dg["scales"].abs().max())
        raw = float((o["grads"]["scales"].double() - dg["scales"]).abs().max()) / scale
        assert raw > 0.2, raw


@pytest.mark.parametrize("form", [f for f in form_cases.FORMS if f["twin"]], ids=lambda f: f["id"])
def test_modifier_changes_nothing_with_both_inputs_precomputed(oracle, form):
    dc, di = form_cases.cotangents(form)
    outs = []
    for f in (form, form["twin"]):
        sc, cam = form_cases.build(f)
        outs.append(run_scene(oracle.Rasterizer, oracle.Settings, sc, cam, CPU, bg=form_cases.BG, antialiasing=f["aa"],
                              dL_dcolor=dc, dL_dinvdepth=di))
    a, b = outs
    for k in ("color", "radii", "invdepth"):
        assert torch.equal(a[k], b[k]), k
    for k in b["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_split_forms_have_their_unsplit_twin():
    """the split forms are compared with the checker's concatenated call on the same rows: those row counts and degrees are
    among the unsplit forms proven above"""
    have = {(f["M"], f["D"]) for f in form_cases.UNSPLIT if not f["cov"] and not f["colors"] and f["mod"] == 1.0}
    for f in form_cases.SPLIT:
        assert (f["M"], f["D"]) in have, f["id"]
        sc, _ = form_cases.build(f)
        assert tuple(sc["shs"].shape) == (f["P"], f["M"], 3)


# ---- the depth pass under a scale modifier -------------------------------------------------------------------------
@pytest.mark.parametrize("mod", form_cases.DEPTH_MODIFIERS)
@pytest.mark.parametrize("name", form_cases.DEPTH_CASES)
def test_depth_pass_cases_keep_their_margins_under_a_modifier(oracle, name, mod):
    """The constructed scenes were built for modifier 1; the two taken for the depth pass under a modifier must still clear
    tests/blend_cases.py's margin condition there (no skip, stop or clamp decision near its threshold: an fp32 realisation
    has nothing to flip, so every pixel can be held to float64), and the checker must agree with float64 on them."""
    case = blend_cases.build(name)
    sc = dict(case.scene_sr, scale_modifier=mod)
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in sc.items()}
    out = dense_reference.render(d, case.cam, case.bg, False, detail=True)
    m = blend_cases.margins(out["detail"])
    print(name, mod, m)
    assert min(m.values()) > 1.0, m
    assert int((out["radii"] > 0).sum()) > 0
    r = dpr.oracle_case(oracle, name, modifier=mod)
    assert torch.equal(r["oracle"]["radii"].long(), r["dense"]["radii"].long())
    for k in ("depth", "alpha"):
        e = float((r["oracle"][k].double() - r["dense"][k]).abs().max()) / max(1.0, float(r["dense"][k].abs().max()))
        assert e <= 2e-5, (k, e)
    print(name, mod, "d_ref", r["d_ref"])
    # the modifier reaches the pass: the means' gradient is not the modifier-1 one
    r1 = dpr.oracle_case(oracle, name)
    assert dpr.distance(r["oracle"]["grads"]["means3D"], r1["dense_grads"]["means3D"], "means3D") > 1e-2

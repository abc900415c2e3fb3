"""The fused train step (gs_backward_step, gs_step_uninstanced) at row counts OFF the float4 grid, against two arbiters:

  A  the un-fused tail it replaces (gs_backward + gs_activations_bwd + gs_densify_stats + gs_adam_step[_masked]) on the same
     blend sums: parameters, both moments and the three statistics torch.equal after every step;
  R  the plain restatement of tests/step_reference.py, from the state before the step and A's exported gradient: exp_avg and
     exp_avg_sq carry its float32 bits, the parameters lie within the bar measured on the restatement (4 x max|p32 - p64| + one
     ulp of the field's largest magnitude) - on an MI355X they carry its float32 bits too, which is what is asserted -, the
     statistics are its statistics.  It shares no Adam code with the kernels.

With P % 4 != 0 the pieces of the field-major flat buffer (xyz at 0, features at 3P, opacity at 51P, scaling at 52P, rotation
at 55P) start off 16 bytes and adam_block / grad_block take their element-wise bodies; which ones depends on P % 4.  Why each P:

    1, 2, 3          fewer rows than a float4 (P % 4 = 1, 2, 3); one workgroup, one wave
    5, 7             one float4 and a tail; P % 4 = 1, 3
    253, 254, 255    one partial block just under 256 rows; P % 4 = 1, 2, 3
    257              a last block of ONE row behind a full one (its pieces: 3, 48, 1, 3, 4 floats)
    514, 771         last blocks of 2 and 3 rows behind two and three full ones; P % 4 = 2, 3
    1021, 1022, 1023 four blocks, every base unaligned in one field or another; P % 4 = 1, 2, 3

Rows 1::3 sit outside every frustum, so float4s of the xyz / opacity / scaling arrays hold elements of invisible, visible and
instanced Gaussians side by side - the float4s the two phases (and sparse_adam) split between them.

Figures of one run on an MI355X (every test prints its own): see DESIGN.md section 4.7.1."""
import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import lgdwt_loss
import step_reference as sr
from gsplat_amd.trainer import FIELDS, GaussianModelLite, Trainer, camera_to

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 7, 253, 254, 255, 257, 514, 771, 1021, 1022, 1023)
FORMS = ("one_launch", "two_phase_depth_limited", "two_phase_reference_lists")
REPORT = {}


@pytest.fixture(autouse=True)
def one_binning_path(hip):
    """(tests/test_gpu_fused_step.py's fixture) `binning = "auto"` picks the path from the sizes of the views rendered before
    (other tests'), so the two runs of a comparison could end up on different paths: pin it."""
    old = (hip.binning, hip._capacity_hint, hip._capacity_hint_limited, hip.tile_cull)
    hip.binning = "region"
    hip._cam_cache.clear()
    yield
    hip.binning, hip._capacity_hint, hip._capacity_hint_limited, hip.tile_cull = old
    for k in ("TWO_PHASE", "TWO_PHASE_MIN_P"):
        hip.__dict__.pop(k, None)     # (back to the class defaults)
    hip._cam_cache.clear()


def make(hip, P, fused, sparse=False, sc=None, spatial_order=False):
    dev = torch.device("cuda")
    sc = sr.scene(P) if sc is None else sc
    cams = [camera_to(c, dev) for c in sr.cameras(4)]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, sr.H, sr.W), generator=g).to(dev) for _ in cams]
    model = GaussianModelLite(sc, dev, api=hip.api, spatial_order=spatial_order)
    crit = lgdwt_loss.criterion(dwt_enable=True, patch_dwt_enable=True)
    tr = Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, torch.zeros(3, device=dev),
                 optimizer_step=True, optimizer_type="sparse_adam" if sparse else "default")
    tr.FUSED_STEP = fused
    return tr


def state(tr):
    m, o = tr.model, tr.model.optimizer
    return dict(flat=m.flat.detach().clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
                accum=m.xyz_gradient_accum.clone(), denom=m.denom.clone(), max_radii=m.max_radii2D.clone())


def host(s):
    return {k: v.detach().cpu().numpy().reshape(-1) for k, v in s.items()}


def unfused_step(hip, a, ci, skip=()):
    """One step of the un-fused trainer -> (its blend sums [P * 16] float64, flat gradient, radii, viewspace gradient), host
    copies but the sums."""
    seen = {}
    inner = a.model.update_view_statistics

    def spy(radii, viewspace_grad, into_delta=False):
        seen["mean2d"] = viewspace_grad.detach().clone()
        return inner(radii, viewspace_grad, into_delta=into_delta)
    a.model.update_view_statistics = spy
    hip.keep_workspace = True
    try:
        a._step_camera(ci, True, skip)
        torch.cuda.synchronize()
        P = a.model.P
        rows = hip.last_workspace[: P * 128].view(torch.float64).clone()
    finally:
        hip.keep_workspace, hip.last_workspace = False, None
        del a.model.update_view_statistics
    assert a.last["path"] == "unfused"
    return rows, a.model.flat_grad.detach().cpu().numpy().copy(), a.last["radii"].cpu().numpy().copy(), seen["mean2d"].cpu().numpy()


def classes(hip, b):
    """(invisible, visible without instances, instanced) of the fused trainer's last forward: the step's radii, the exported
    row mask (gs_export_row_mask: emitted an instance) and - where the tail splits on them - the forward blend's reached flags"""
    P = b.model.P
    radii = b.last["radii"]
    mask = torch.zeros((P,), dtype=torch.uint8, device=radii.device)
    assert hip.export_row_mask(mask)
    inst = mask.bool()
    if hip.REACHED_SPLIT and hip._last is not None:
        inst &= hip.export_reached(P, hip._last.geom).bool()
    vis = radii > 0
    inst &= vis
    return (~vis).cpu().numpy(), (vis & ~inst).cpu().numpy(), inst.cpu().numpy()


def check_against_restatement(before, after, grad, counts, skip, radii, mean2d, sparse, P, what, fields=FIELDS):
    """R: one step of the restatement from `before` with gradient `grad` against `after` (host dicts)."""
    lr, t, on, row = sr.element_tables(P, counts, skip, fields=fields)
    vis = radii > 0
    stepped = on & (vis[row] if sparse else True)
    slices = {name: (lo, hi) for name, (lo, hi, _) in sr.field_offsets(P, fields).items()}
    sr.check_against_restatement(after["flat"], after["exp_avg"], after["exp_avg_sq"], before["flat"], grad, before["exp_avg"],
                                 before["exp_avg_sq"], lr, t, stepped, slices, what=what, report=REPORT)
    accum, denom, max_radii = sr.stats_ref(before["accum"], before["denom"], before["max_radii"], radii, mean2d)
    assert np.array_equal(after["denom"], denom) and np.array_equal(after["max_radii"], max_radii), what
    # (the norm is one sqrtf of a sum of two squares: held to the last bit of the running total)
    assert bool((np.abs(after["accum"].astype(np.float64) - accum) <= np.spacing(np.abs(accum))).all()), what
    assert np.array_equal(after["accum"][~vis], before["accum"][~vis])
    if sparse:   # rows that are not visible keep all 59 floats and both moments, bit for bit
        frozen = ~vis[row]
        for k in ("flat", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(sr.bits(after[k])[frozen], sr.bits(before[k])[frozen]), (what, k)


def run_pair(hip, a, b, cams, what, sparse, skips=None, per_step=None):
    """The pattern of test_fused_tail_equals_the_three_kernels_bit_for_bit: A un-fused, B fused on A's blend sums; A and R after
    every step."""
    P = a.model.P
    assert torch.equal(a.model.flat, b.model.flat) and b.model.P == P
    counts = {name: int(a.model.optimizer.seg_steps[name]) for name, _ in FIELDS}
    for it, ci in enumerate(cams):
        skip = () if skips is None else skips[it]
        before = host(state(b))
        rows, grad, radii, mean2d = unfused_step(hip, a, ci, skip)
        b.rows_override = rows
        b._step_camera(ci, True, skip)
        b.sync()
        torch.cuda.synchronize()
        assert b.last["path"] in ("manual", "fused")
        sa, sb = state(a), state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (what, it, k, float((sa[k] - sb[k]).abs().max()))
        assert a.model.optimizer.seg_steps == b.model.optimizer.seg_steps
        for name, _ in FIELDS:
            counts[name] += name not in skip
        assert counts == {name: a.model.optimizer.seg_steps[name] for name, _ in FIELDS}
        assert np.array_equal(radii, b.last["radii"].cpu().numpy())
        check_against_restatement(before, host(sb), grad, counts, skip, radii, mean2d, sparse, P, "%s step %d" % (what, it + 1))
        if per_step is not None:
            per_step(it, ci)


@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("P", SIZES)
def test_fused_step_off_the_float4_grid(hip, P, form, sparse):
    a, b = make(hip, P, False, sparse), make(hip, P, True, sparse)
    two_phase = form != "one_launch"
    hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = two_phase, 0
    cams = [0, 1, 2]
    if form == "two_phase_reference_lists":    # GsView.tile_cull = 0: the reference's own lists
        hip.tile_cull = False
    if form == "two_phase_depth_limited":
        b.depth_limit = "deferred"
        cams = [0, 1, 2, 0, 1, 2]     # (a camera's first visit measures its stop depths: the second one's lists are cut)
    seen = []
    n0, used0, failed0 = hip.two_phase_launches, hip.depth_limit_stats["used"], hip.depth_limit_stats["failed"]

    def per_step(it, ci):
        inv, bare, inst = classes(hip, b)
        seen.append((int(inv.sum()), int(bare.sum()), int(inst.sum())))
        assert inst.any(), "step %d: no instanced Gaussian" % (it + 1)
    run_pair(hip, a, b, cams, "P %d %s%s" % (P, form, " sparse" if sparse else ""), sparse, per_step=per_step)
    print("P %d %s: (invisible, visible without instances, instanced) per step %s" % (P, form, seen))
    assert (hip.two_phase_launches - n0 >= len(cams)) == two_phase
    if P >= 253:
        for k, name in enumerate(("invisible", "visible without instances", "instanced")):
            assert sum(s[k] for s in seen) > 0, "no %s Gaussian in any step" % name
    if form == "two_phase_depth_limited":
        used, failed = hip.depth_limit_stats["used"] - used0, hip.depth_limit_stats["failed"] - failed0
        print("   depth limits used in %d forwards, failed in %d" % (used, failed))
        assert used >= 3      # the second visits ran on cut lists (a view whose limits fail is repeated without them)
        # (below 253 rows there is no wall: a handful of Gaussians saturates no tile, nothing visible is cut or unreached)
        assert all(s[1] >= 1 for s in seen[3:]) or P < 253, seen
    assert float(a.model.denom.max()) == len(cams)


def test_skipped_group_and_count_off_the_grid(hip):
    """Opacity without a gradient at step 2 (a reset iteration): the row, its moments and its step count stay; at step 3 its
    bias corrections are those of count 2 while every other row's are of count 3."""
    P = 1021
    a, b = make(hip, P, False), make(hip, P, True)
    run_pair(hip, a, b, [0, 1, 2], "P 1021 opacity skipped", False, skips=[(), ("opacity",), ()])
    assert a.model.optimizer.seg_steps["opacity"] == 2 and a.model.optimizer.seg_steps["xyz"] == 3


# ---------------------------------------------------------------------------------------------------------------- dormant blocks
@pytest.mark.parametrize("two_phase", [True, False], ids=["two_phase", "one_launch"])
def test_dormant_blocks_with_a_partial_last_block(hip, two_phase):
    """P = 1023 in spatial order with a third of the rows lifted: ceil(P / 256) = 4 flags, the last block 255 rows.  USE_DORMANT
    on against off bit for bit; the USE_DORMANT form against the un-fused tail and the restatement on pinned sums (a dormant
    block's rows have +0 moments and a zero gradient: the restatement leaves them at +0 and the parameters alone, which is what
    skipping the block does); every flag still standing is true of the moments."""
    P = 1023
    sc = sr.scene(P, lifted=slice(0, 0))
    sc["means3D"][: P // 3, 2] += 50.0           # (before the Morton sort: the lifted rows end up in blocks of their own)
    hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = two_phase, 0
    a, b, u = (make(hip, P, f, sc=sc, spatial_order=True) for f in (True, True, False))
    assert a.model.spatial_order and torch.equal(a.model.flat, b.model.flat) and torch.equal(a.model.flat, u.model.flat)
    b.model.optimizer.USE_DORMANT = False
    a.depth_limit = b.depth_limit = "deferred"
    for k in range(6):
        a.step(k)
        b.step(k)
    a.sync()
    b.sync()
    torch.cuda.synchronize()
    sa, sb = state(a), state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (k, float((sa[k] - sb[k]).abs().max()))
    opt = a.model.optimizer
    kept = opt.dormant_flags().clone()
    opt.invalidate_dormant()
    derived = opt.dormant_flags().clone()
    assert kept.numel() == 4
    assert bool(((kept == 0) | (derived == 1)).all()), "a block is flagged dormant although one of its moments is not +0"
    print("dormant flags kept %s derived %s" % (kept.tolist(), derived.tolist()))
    assert 1 <= int(kept.sum()) < 4          # the skip really happened, and not everywhere
    # the USE_DORMANT form against the un-fused tail and the restatement, on pinned sums
    c = make(hip, P, True, sc=sc, spatial_order=True)
    assert c.model.optimizer.USE_DORMANT
    run_pair(hip, u, c, [0, 1, 2], "P 1023 dormant %s" % ("two-phase" if two_phase else "one launch"), False)
    kept = c.model.optimizer.dormant_flags().clone()
    c.model.optimizer.invalidate_dormant()
    derived = c.model.optimizer.dormant_flags().clone()
    assert bool(((kept == 0) | (derived == 1)).all()) and int(kept.sum()) >= 1


# ---------------------------------------------------------------------------------------------------------------- densification
def _densified(hip, thr):
    """A trainer of tests/test_gpu_densify_device.py::make_trainer (P = 300, 96 x 80) after three fused steps and one
    densify_and_prune on the host path at gradient threshold `thr` -> (trainer, (n_clone, n_split, n_pruned))"""
    from test_gpu_densify_device import make_trainer
    tr = make_trainer(hip)
    tr.FUSED_STEP = True
    for k in range(3):
        tr.step(k)
    tr.sync()
    tr.gather_optimizer_state()
    res = tr.model.densify_and_prune(thr, 0.005, 4.4, None, None, generator=torch.Generator().manual_seed(1))
    return tr, res


def test_steps_after_a_real_densification(hip):
    """Two trainers through three fused steps and one real densification whose new P is off the float4 grid (the first
    threshold of a short list that gives one: the train step is reproducible, so both trainers get the same model).  Then
    three steps, fused against un-fused and against the restatement: new rows start from +0 moments beside old rows with
    history."""
    for thr in (1e-7, 2e-7, 5e-7, 1e-6, 2e-6, 5e-6, 1e-5, 2e-5, 5e-5):
        a, res = _densified(hip, thr)
        if a.model.P % 4 != 0 and res[0] + res[1] > 0:
            break
    P = a.model.P
    print("densified at threshold %g: %s -> P = %d (P %% 4 = %d)" % (thr, res, P, P % 4))
    assert P % 4 != 0 and res[0] + res[1] > 0, "no threshold leaves P off the float4 grid"
    b, res_b = _densified(hip, thr)
    assert res_b == res and b.model.P == P
    assert torch.equal(a.model.flat, b.model.flat) and torch.equal(a.model.optimizer.exp_avg, b.model.optimizer.exp_avg)
    m = a.model.optimizer.exp_avg
    rows_with_history = (a.model.optimizer.field_views(m)["features"] != 0).any(dim=1)
    assert bool(rows_with_history.any()) and bool((~rows_with_history).any())
    a.FUSED_STEP, b.FUSED_STEP = False, True
    run_pair(hip, a, b, [3, 0, 1], "after densification P %d" % P, False)


# ---------------------------------------------------------------------------------------------------------------- graph replay
def test_graphed_step_off_the_grid(hip):
    """GraphedStep (coef_dev: the step's constants read from device memory) at P = 1021 against the eager fused step on pinned
    sums, as tests/test_gpu_fused_step.py::test_graphed_step_equals_the_eager_fused_step does at 30 000."""
    from gsplat_amd.trainer import GraphedStep
    from test_gpu_fused_step import _camera_sequence
    P = 1021
    make(hip, P, True).step(0)     # (a first eager view sizes the binning-capacity hint)
    torch.cuda.synchronize()
    a, b = make(hip, P, True), make(hip, P, True)
    g = torch.Generator().manual_seed(11)
    rows = torch.zeros((P, 16), dtype=torch.float64)
    rows[:, :9] = (torch.randn((P, 9), generator=g) * 1e-3).double()
    rows = rows.cuda()
    a.rows_override = b.rows_override = rows
    gs = GraphedStep(b)
    for k in range(8):
        gs.step(k)
    seq = _camera_sequence(8)
    for c in seq:
        a._step_camera(c, True, ())
    gs.sync()
    torch.cuda.synchronize()
    assert gs.captures == 4 and gs.replays == 4 and gs.eager_steps == 0
    sa, sb = state(a), state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (k, float((sa[k] - sb[k]).abs().max()))
    assert a.model.optimizer.t == b.model.optimizer.t == len(seq) == 14


# ---------------------------------------------------------------------------------------------------------------- multispectral
def make_nir(hip, P, fused):
    from gsplat_amd.losses import LossOps
    from gsplat_amd.trainer import NirCriterion, TrainerNIR
    dev = torch.device("cuda")
    cams = [camera_to(c, dev) for c in sr.cameras(4)]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, sr.H, sr.W), generator=g).to(dev) for _ in cams]
    nirs = [torch.rand((1, sr.H, sr.W), generator=g).to(dev) for _ in cams]
    model = GaussianModelLite(sr.scene(P), dev, api=hip.api, with_nir=True)
    crit = NirCriterion(LossOps(hip.api), fused=fused)
    return TrainerNIR(model, cams, gts, nirs, crit, dgr.GaussianRasterizationSettings, torch.zeros(3, device=dev))


# relative distance granted between the un-fused and the fused GRADIENT of the 60th row and of the gain: the un-fused step forms
# them in torch (sigmoid and its derivative, the clamp, a sum over Gaussians), the fused one in the kernels - a chain of about
# ten float32 roundings (6e-8 each) on either side
NIR_GRAD_DELTA = 1e-5


def sensitivity_bar(p0, g, m0, v0, lr, t):
    """Per element: how far the float64 restatement's parameter moves when the gradient moves by NIR_GRAD_DELTA of itself,
    plus the restatement's own bar."""
    on = np.ones(p0.shape, bool)
    p64 = sr.adam_ref(p0, g, m0, v0, lr, t, on, np.float64)[0]
    p32 = sr.adam_ref(p0, g, m0, v0, lr, t, on, np.float32)[0]
    hi = sr.adam_ref(p0, g.astype(np.float64) * (1 + NIR_GRAD_DELTA), m0, v0, lr, t, on, np.float64)[0]
    lo = sr.adam_ref(p0, g.astype(np.float64) * (1 - NIR_GRAD_DELTA), m0, v0, lr, t, on, np.float64)[0]
    return p64, np.maximum(np.abs(hi - p64), np.abs(lo - p64)) + sr.param_tolerance(p32, p64)[0]


@pytest.mark.parametrize("two_phase", [False, True], ids=["one_launch", "two_phase"])
def test_multispectral_step_off_the_grid(hip, two_phase):
    """TrainerNIR at P = 1021: 60 floats per row, the sixth row array and the gain.  The fused step (gs_backward_step_x) on the
    blend sums of its un-fused form (gs_backward_x, torch's criterion and activations, gs_adam_step, torch's Adam for the gain):
    the 59 floats of the RGB model, their moments and the statistics bit for bit and against the restatement.  The 60th row's
    and the gain's gradients are formed in torch on one side and in the kernels on the other; they are held to the float64
    restatement with the room a gradient NIR_GRAD_DELTA away would need (at 30 000 rows tests/test_nir_trainer.py compares whole
    trajectories at 1e-4 rms, a bar that one flipped opacity step would break at this size)."""
    from gsplat_amd.trainer import LRS, NIR_FIELD
    P = 1021
    hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = two_phase, 0
    a, b = make_nir(hip, P, False), make_nir(hip, P, True)
    assert not a._fused_step_ok(a._backend(), True) and b._fused_step_ok(b._backend(), True)
    fields = FIELDS + (NIR_FIELD,)
    n59 = 59 * P
    counts = {name: 0 for name, _ in fields}
    n0 = hip.two_phase_launches

    def gain_state(tr):
        gs = tr.model.nir_gain_optimizer.state[tr.model.nir_gain]
        return [float(x.detach().double().cpu()) for x in (tr.model.nir_gain, gs["exp_avg"], gs["exp_avg_sq"])]
    for it, ci in enumerate([0, 1, 2]):
        before, gain_before = host(state(b)), gain_state(b)
        rows, grad, radii, mean2d = unfused_step(hip, a, ci)
        gain_grad = float(a.model.nir_gain.grad.detach().cpu())
        b.rows_override = rows
        b._step_camera(ci, True, ())
        b.sync()
        torch.cuda.synchronize()
        sa, sb = state(a), state(b)
        for k in ("flat", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k][:n59], sb[k][:n59]), (it, k, float((sa[k][:n59] - sb[k][:n59]).abs().max()))
        for k in ("accum", "denom", "max_radii"):
            assert torch.equal(sa[k], sb[k]), (it, k)
        for name in counts:
            counts[name] += 1
        after = host(sb)
        cut = {k: (v[:n59] if k in ("flat", "exp_avg", "exp_avg_sq") else v) for k, v in after.items()}
        cut0 = {k: (v[:n59] if k in ("flat", "exp_avg", "exp_avg_sq") else v) for k, v in before.items()}
        check_against_restatement(cut0, cut, grad[:n59], counts, (), radii, mean2d, False, P, "NIR P 1021 step %d" % (it + 1))
        # the 60th row and the gain
        lr = np.full(P, LRS["nir_albedo"], np.float64)
        t = np.full(P, counts["nir_albedo"], np.int64)
        p64, bar = sensitivity_bar(before["flat"][n59:], grad[n59:], before["exp_avg"][n59:], before["exp_avg_sq"][n59:], lr, t)
        dev = np.abs(after["flat"][n59:].astype(np.float64) - p64)
        print("NIR step %d: 60th row largest deviation %.3e (largest bar %.3e), moved by up to %.3e" % (
            it + 1, float(dev.max()), float(bar.max()), float(np.abs(after["flat"][n59:] - before["flat"][n59:]).max())))
        assert bool((dev <= bar).all()), (it, float((dev - bar).max()))
        assert float(np.abs(after["flat"][n59:] - before["flat"][n59:]).max()) > 0
        one = np.ones(1)
        g64, gbar = sensitivity_bar(np.float32(gain_before[0]) * one.astype(np.float32), np.float32(gain_grad) * one.astype(np.float32),
                                    np.float32(gain_before[1]) * one.astype(np.float32), np.float32(gain_before[2]) * one.astype(np.float32),
                                    LRS["nir_gain"] * one, (it + 1) * one.astype(np.int64))
        assert abs(gain_state(b)[0] - float(g64[0])) <= float(gbar[0]), (it, gain_state(b)[0], float(g64[0]), float(gbar[0]))
    assert (hip.two_phase_launches - n0 >= 3) == two_phase
    assert gain_state(b)[0] != 1.0 and b.model.optimizer.seg_steps["nir_gain"] == 3

"""The fused train step of the FSGS rasterizer generation on an MI355X: gs_backward_step_fsgs against the kernels it replaces
(gs_backward_fsgs + gs_activations_bwd + gs_densify_stats + gs_adam_step) bit for bit on pinned blend sums, raw activations
against activated inputs, FsgsCriterion's one node against its un-fused form and the torch restatement, the un-fused HIP
gradients against the checker's, TrainerFSGS fused against un-fused, and train_iteration across a densification and a pseudo
iteration."""
import ctypes as C
import random

import pytest
import torch

import fsgs_loss
import fsgs_loss_reference as flr
import fsgs_train_reference as ftr
import step_reference as sr
from gsplat_amd import synthetic
from gsplat_amd.capi import GsError
from gsplat_amd.fsgs_criterion import FsgsCriterion
from gsplat_amd.losses import LossOps
from gsplat_amd.trainer import FsgsOptions, GaussianModelLite, TrainerFSGS, camera_to, expon_lr
from helpers import TOL, check_grads, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def one_binning_path(hip):
    """(tests/test_gpu_fused_step.py's fixture) the two runs of a comparison must build their lists the same way"""
    old = (hip.binning, hip._capacity_hint, hip._capacity_hint_limited)
    hip.binning = "region"
    hip._cam_cache.clear()
    yield
    hip.binning, hip._capacity_hint, hip._capacity_hint_limited = old
    hip._cam_cache.clear()


def estimator(image):
    """stands for estimate_depth(render, mode='train'): any differentiable map image [3,H,W] -> depth [H,W]"""
    return 40.0 * image[0] - 25.0 * image[1] + 10.0 * image[2] * image[2] + 3.0


def scene_of(P, seed=3):
    """P <= 1024: tests/step_reference.py's scene, rows 1::3 outside every frustum; larger: a trained-like scene whose first
    quarter sits 50 units above it - outside every frustum too"""
    if P <= 1024:
        return sr.scene(P, wall=False)
    if (P, seed) not in _SCENES:     # (built once: its kNN is the expensive part)
        from simple_knn._C import distCUDA2
        sc = synthetic.trained_like(P, seed=seed, sh_degree=3, knn=lambda x: distCUDA2(x.to("cuda")).cpu())
        sc["means3D"][: P // 4, 2] += 50.0
        _SCENES[(P, seed)] = sc
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in _SCENES[(P, seed)].items()}


_SCENES = {}


def make(hip, fused, P=30000, W=480, H=320, deg=3, n_cams=4, pseudo=False, sc=None, device="cuda", oracle=None):
    dev = torch.device(device)
    sc = scene_of(P) if sc is None else sc
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:n_cams]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g).to(dev) for _ in cams]
    midas = [(1000.0 - 100.0 * (2.0 + 6.0 * torch.rand((H, W), generator=g))).to(dev) for _ in cams]
    kw = {}
    if pseudo:
        kw = dict(pseudo_cameras=[camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[n_cams:n_cams + 3]], depth_estimator=estimator)
    if oracle is not None:   # the checker: its rasterizer, the restated Pearson terms
        model = GaussianModelLite(sc, dev, api=oracle.api)
        crit = FsgsCriterion(LossOps(oracle.api))
        kw.update(Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings, pearson=flr.depth_pearson_loss,
                  pseudo_pearson=flr.pseudo_depth_pearson_loss)
    else:
        model = GaussianModelLite(sc, dev, api=hip.api)
        crit = fsgs_loss.criterion()
        assert crit.fused
    model.active_sh_degree = deg
    tr = TrainerFSGS(model, cams, gts, midas, crit, torch.zeros(3, device=dev), **kw)
    tr.FUSED_STEP = fused
    return tr


def state(tr):
    m, o = tr.model, tr.model.optimizer
    return dict(flat=m.flat.detach().clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
                accum=m.xyz_gradient_accum.clone(), denom=m.denom.clone(), max_radii=m.max_radii2D.clone())


def unfused_step_with_rows(hip, a, ci):
    """one un-fused step of `a` -> the float64 blend sums its backward left [P, 16]"""
    hip.keep_workspace = True
    try:
        a._step_camera(ci, True, ())
        torch.cuda.synchronize()
        rows = hip.last_workspace[: a.model.P * 128].view(torch.float64).clone()
    finally:
        hip.keep_workspace, hip.last_workspace = False, None
    assert a.last["path"] == "unfused"
    return rows


# ---- the step kernel -----------------------------------------------------------------------------------------------------
def fused_equals_the_four_kernels(hip, a, b, steps=3):
    """`a` un-fused, `b` fused on a's blend sums, `steps` consecutive steps from the same model: parameters, both moments and the
    three statistics torch.equal after every one -> a's last state.  (tests/test_gpu_model_ops.py runs it on its own rows.)"""
    assert torch.equal(a.model.flat, b.model.flat)
    for it in range(steps):
        b.rows_override = unfused_step_with_rows(hip, a, it)
        b._step_camera(it, True, ())
        torch.cuda.synchronize()
        assert b.last["path"] == "fused"
        sa, sb = state(a), state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (it, k, float((sa[k] - sb[k]).abs().max()))
        assert a.model.optimizer.t == b.model.optimizer.t and a.model.optimizer.seg_steps == b.model.optimizer.seg_steps
    return sa


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("size", [(160, 128), (150, 100)], ids=["160x128", "150x100"])
@pytest.mark.parametrize("P", [1, 3, 1023, 30000])
def test_fused_step_equals_the_four_kernels_bit_for_bit(hip, P, size, deg):
    """gs_backward_step_fsgs against gs_backward_fsgs + gs_activations_bwd + gs_densify_stats + gs_adam_step on the same blend
    sums: parameters, both moments and the three statistics, torch.equal over three consecutive steps.  Row counts off the
    float4 grid, images whose tiles are cut by the border, a share of the Gaussians outside every frustum."""
    W, H = size
    a, b = make(hip, False, P=P, W=W, H=H, deg=deg), make(hip, True, P=P, W=W, H=H, deg=deg)
    start = a.model.flat.detach().clone()
    sa = fused_equals_the_four_kernels(hip, a, b)
    assert float((sa["flat"] - start).abs().max()) > 0 and float(sa["denom"].max()) >= 1.0
    if P >= 3:   # some rows are outside every frustum: never seen
        assert float(sa["denom"].min()) == 0.0


def test_raw_activations_render_the_same_image_and_step_within_rounding(hip):
    """GsGaussians.raw_activations through gs_forward_render_fsgs / gs_backward_step_fsgs against the activated tensors of
    gs_activations_fwd: the same images bit for bit (the kernels apply that kernel's arithmetic), and the same step on
    pinned sums - held to the bar of two runs that differ in rounding only (tests/test_gpu_fused_step.py: parameter rms within
    1e-4 of the parameters' rms, equal statistics)."""
    a = make(hip, False, P=1023, W=160, H=128)
    b, c = make(hip, True, P=1023, W=160, H=128), make(hip, True, P=1023, W=160, H=128)
    c.RAW_ACTIVATIONS = False
    with torch.no_grad():
        hip.raw_activations = True
        raw = b._render_camera(b.cameras[0], True)
        act = c._render_camera(c.cameras[0], False)
    for k in ("render", "depth", "alpha", "radii"):
        assert torch.equal(raw[k], act[k]), k
    assert float(raw["render"].abs().max()) > 0
    for it in range(3):
        rows = unfused_step_with_rows(hip, a, it)
        for tr in (b, c):
            tr.rows_override = rows
            tr._step_camera(it, True, ())
            assert tr.last["path"] == "fused"
    torch.cuda.synchronize()
    sb, sc_ = state(b), state(c)
    d = (sb["flat"] - sc_["flat"]).double()
    print("raw against activated: max |dp| %.3e" % float(d.abs().max()))
    assert float(d.pow(2).mean().sqrt()) <= 1e-4 * float(sb["flat"].double().pow(2).mean().sqrt())
    assert torch.equal(sb["denom"], sc_["denom"]) and torch.equal(sb["max_radii"], sc_["max_radii"])
    assert torch.equal(sb["accum"], sc_["accum"])     # (the norm of two pinned sums: no activation enters it)


def forward_for_errors(hip, tr):
    """a raw-rows FSGS forward of `tr`'s model -> the arguments of gs_backward_step_fsgs for it"""
    import math
    m, cam = tr.model, tr.cameras[0]
    st = m.optimizer.fused_request(())
    H, W = int(cam.image_height), int(cam.image_width)
    p = m.params
    hip.raw_activations = True
    out = hip.rasterize_gaussians(tr.bg, p["xyz"].detach(), torch.Tensor([]), p["opacity"].detach(), p["scaling"].detach(),
                                  p["rotation"].detach(), 1.0, torch.Tensor([]), cam.world_view_transform, cam.full_proj_transform,
                                  math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), H, W, p["features"].detach(), m.active_sh_degree,
                                  cam.camera_center, False, False, False, fsgs=True)
    R, color, radii, geom, binning, img, depth, alpha = out
    last = hip._last
    s = hip._scratch(geom, img, binning, hip._capacity_for(binning, m.P, W, H, R))
    wsb = hip.scratch_bytes(m.P, W, H, R)[3]
    ws = torch.zeros((wsb,), dtype=torch.uint8, device=geom.device)
    g3 = torch.zeros((3, H, W), device=geom.device)
    g1 = torch.zeros((1, H, W), device=geom.device)
    keep = (out, last.keep, ws, g3, g1)
    return dict(view=last.view, g=last.g, radii=radii, s=s, R=int(R), g3=g3, g1=g1, st=st, ws=ws, keep=keep)


def call_step(hip, f, view=None, g=None, gcolor=True, gdepth=True, galpha=True, st=True):
    fn = hip.api.raw("backward_step_fsgs")
    return fn(C.byref(f["view"] if view is None else view), C.byref(f["g"] if g is None else g), f["radii"].data_ptr(),
              C.byref(f["s"]), f["R"], f["g3"].data_ptr() if gcolor else None, f["g1"].data_ptr() if gdepth else None,
              f["g1"].data_ptr() if galpha else None, C.byref(f["st"]) if st is True else st, f["ws"].data_ptr(), f["ws"].numel(),
              None)


def copy_of(struct):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
    return c


def test_argument_errors_of_the_new_entry_point(hip):
    """one case per rule of include/gsplat.h; every one is answered before anything is enqueued"""
    tr = make(hip, True, P=1023, W=160, H=128)
    before = state(tr)
    f = forward_for_errors(hip, tr)
    NULL, SHAPE, UNSUPPORTED = -1, -2, -5
    assert call_step(hip, f, gdepth=False) == NULL
    assert call_step(hip, f, galpha=False) == NULL
    assert call_step(hip, f, st=None) == NULL
    assert call_step(hip, f, gcolor=False) == NULL
    v = copy_of(f["view"])
    v.antialiasing = 1
    assert call_step(hip, f, view=v) == UNSUPPORTED
    g = copy_of(f["g"])
    g.extra_channel = f["radii"].data_ptr()
    assert call_step(hip, f, g=g) == UNSUPPORTED
    ok = f["st"]
    for field, value, want in (("extra", f["radii"].data_ptr(), UNSUPPORTED), ("phase", 2, UNSUPPORTED), ("phase", 1, UNSUPPORTED),
                               ("xyz", None, NULL), ("denom", None, NULL), ("rows_clean", 3, SHAPE)):
        bad = copy_of(ok)
        setattr(bad, field, value)
        f["st"] = bad
        assert call_step(hip, f) == want, field
    bad = copy_of(ok)
    bad.step[0] = -1
    f["st"] = bad
    assert call_step(hip, f) == SHAPE
    bad = copy_of(ok)
    bad.features = f["radii"].data_ptr()          # g->shs must BE st->features
    f["st"] = bad
    assert call_step(hip, f) == SHAPE
    torch.cuda.synchronize()
    after = state(tr)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # the backend's refusals: a 4th channel, depth limits and the capture-safe forward with a fused step armed
    hip.fused_step = tr.model.optimizer.fused_request(())
    hip.depth_limit_request = "defer"
    with pytest.raises(RuntimeError, match="depth-limited lists are closed"):
        tr._render_camera(tr.cameras[0], True)
    assert hip.fused_step is None and hip.depth_limit_request is None
    hip.fused_step = tr.model.optimizer.fused_request(())
    hip.static_capacity = 1 << 20
    try:
        with pytest.raises(RuntimeError, match="GraphedStep"):
            tr._render_camera(tr.cameras[0], True)
    finally:
        hip.static_capacity = None
    assert hip.fused_step is None
    hip.raw_activations = False


def test_a_confidence_that_is_not_all_ones_is_refused_on_the_fused_path(hip):
    tr = make(hip, True, P=1023, W=160, H=128)
    before = state(tr)
    tr._confidence()[5] = 0.5
    with pytest.raises(RuntimeError, match="confidence"):
        tr._step_camera(0, True, ())
    assert hip.fused_step is None and not hip.raw_activations
    tr.FUSED_STEP = False
    tr.model.optimizer.t, tr.model.optimizer.seg_steps = 0, {k: 0 for k in tr.model.optimizer.seg_steps}
    tr._step_camera(0, True, ())     # the un-fused step scales the gradients by it, as the reference does
    assert tr.last["path"] == "unfused" and not torch.equal(before["flat"], tr.model.flat)


# ---- the criterion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("size", [(64, 48), (504, 378)], ids=["64x48", "504x378"])
def test_the_criterions_one_node_is_its_unfused_form_and_the_restatement(hip, size, kind):
    W, H = size
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    gt = torch.rand((3, H, W), generator=g)
    img0 = gt + 0.2 * torch.randn((3, H, W), generator=g)      # (leaves [0, 1]: the criterion must not clamp)
    x, m = flr.scene(H, W, kind, 3, dtype=torch.float32)
    crit = fsgs_loss.criterion()
    out = {}
    for form in ("fused", "unfused"):
        img = img0.to(dev).requires_grad_(True)
        depth = x.reshape(1, H, W).to(dev).requires_grad_(True)
        if form == "fused":
            loss, parts = crit.fused_call(img, depth, gt.to(dev), m.to(dev), 0.05)
            torch.autograd.backward(loss, crit.ops.unit_grad(dev))
            branch = int(parts["branch"])
        else:
            loss, parts = crit(img, depth, gt.to(dev), m.to(dev), 0.05)
            loss.backward()
        out[form] = (float(loss.detach()), img.grad.cpu(), depth.grad.cpu())
    i64, d64 = img0.double().requires_grad_(True), x.double().reshape(1, H, W).requires_grad_(True)
    want, want_branch = ftr.train_loss(i64, d64[0], gt.double(), m.double(), 0.05)
    want.backward()
    assert branch == want_branch == (0 if kind == "A" else 1)
    for form, (loss, gi, gd) in out.items():
        print("%s %dx%d %s: loss %.3e image %.3e depth %.3e" % (form, W, H, kind, abs(loss - float(want.detach())) / float(want.detach()),
                                                                rel_err(gi, i64.grad), rel_err(gd, d64.grad)))
        assert abs(loss - float(want.detach())) <= TOL * abs(float(want.detach())), form
        assert rel_err(gi, i64.grad) <= TOL and rel_err(gd, d64.grad) <= TOL, form
    assert abs(out["fused"][0] - out["unfused"][0]) <= TOL * abs(out["unfused"][0])
    assert rel_err(out["fused"][1], out["unfused"][1]) <= TOL and rel_err(out["fused"][2], out["unfused"][2]) <= TOL
    # an upstream gradient that is not the cached unit: both halves scale by it
    img = img0.to(dev).requires_grad_(True)
    depth = x.reshape(1, H, W).to(dev).requires_grad_(True)
    loss, _ = crit.fused_call(img, depth, gt.to(dev), m.to(dev), 0.05)
    (loss * 3.0).backward()
    # (the same products with the factor applied at another place: a few fp32 roundings, 6e-8 each)
    assert rel_err(img.grad.cpu(), 3.0 * out["fused"][1]) <= 1e-5 and rel_err(depth.grad.cpu(), 3.0 * out["fused"][2]) <= 1e-5


def test_a_constant_depth_image_gives_nan_and_leaves_the_image_gradient_alone(hip):
    W, H = 64, 48
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(12)
    gt = torch.rand((3, H, W), generator=g).to(dev)
    img0 = (gt.cpu() + 0.2 * torch.randn((3, H, W), generator=g)).to(dev)
    x, m = flr.scene(H, W, "A", 3, dtype=torch.float32)
    crit = fsgs_loss.criterion()
    grads = []
    for depth0 in (x.reshape(1, H, W), torch.full((1, H, W), 3.25)):
        img, depth = img0.clone().requires_grad_(True), depth0.to(dev).requires_grad_(True)
        loss, parts = crit.fused_call(img, depth, gt, m.to(dev), 0.05)
        torch.autograd.backward(loss, crit.ops.unit_grad(dev))
        grads.append((loss.detach(), img.grad, depth.grad, parts))
    assert bool(torch.isfinite(grads[0][0])) and bool(torch.isnan(grads[1][0]))
    assert torch.equal(grads[0][1], grads[1][1]) and float(grads[1][1].abs().max()) > 0
    assert not bool(grads[1][2].any()) and float(grads[0][2].abs().max()) > 0
    assert bool(torch.isfinite(grads[1][3]["base"])) and bool(torch.isnan(grads[1][3]["depth"]))


# ---- the trainer ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def product_T(oracle):
    """The checker's FSGS backward with T_final as the transmittance product - what the HIP path keeps - instead of the
    reference's `1 - alpha` read-back, whose fp32 cancellation alone moves the gradients by 1e-4 .. 1e-3
    (tests/test_gpu_fsgs.py: only the product form is held to TOL)."""
    oracle.lib.gso_set_fsgs_exact_T(1)
    yield
    oracle.lib.gso_set_fsgs_exact_T(0)


def test_unfused_hip_gradients_are_the_checkers(hip, oracle, product_T):
    """One un-fused iteration of TrainerFSGS on the HIP kernels against the same on the CPU checker (its FSGS rasterizer, the
    restated Pearson term): every parameter gradient within TOL - with the bit-for-bit case above this ties the fused step to
    the checker."""
    sc = scene_of(1023)
    h = make(hip, False, P=1023, W=160, H=128, sc=sc)
    o = make(hip, False, P=1023, W=160, H=128, sc=sc, device="cpu", oracle=oracle)
    lh, lo = h._step_camera(1, False, ()), o._step_camera(1, False, ())
    assert h.last["path"] == o.last["path"] == "unfused"
    assert abs(float(lh) - float(lo)) <= TOL * abs(float(lo))
    names = {"xyz": "means3D", "features": "shs", "opacity": "opacities", "scaling": "scales", "rotation": "rotations"}
    hg = {names[k]: v.grad.detach().cpu() for k, v in h.model.params.items()}
    og = {names[k]: v.grad.detach().cpu() for k, v in o.model.params.items()}
    check_grads(hg, og, "fsgs_trainer_unfused_1023")
    assert torch.equal(h.last["radii"].cpu(), o.last["radii"]) and int((h.last["radii"] > 0).sum()) > 300


def test_fused_train_step_tracks_the_unfused_one(hip):
    """Without pinning both paths run their own blend backward: the bounds of tests/test_gpu_fused_step.py's LGDWT case."""
    a, b = make(hip, False), make(hip, True)
    la, lb = [], []
    for k in range(8):
        la.append(float(a.step(k % 4)))
        lb.append(float(b.step(k % 4)))
    assert a.last["path"] == "unfused" and b.last["path"] == "fused"
    assert max(abs(x - y) for x, y in zip(la, lb)) <= 1e-3 * max(la)
    d = (a.model.flat - b.model.flat).double()
    assert float(d.pow(2).mean().sqrt()) <= 1e-4 * float(a.model.flat.double().pow(2).mean().sqrt())
    assert torch.equal(a.model.denom, b.model.denom) and torch.equal(a.model.max_radii2D, b.model.max_radii2D)
    assert a.model.optimizer.t == b.model.optimizer.t == 8


def test_two_fused_runs_are_the_same_bits(hip):
    runs = []
    for rep in range(2):
        tr = make(hip, True)
        losses = [tr.step(k) for k in range(8)]
        torch.cuda.synchronize()
        assert tr.last["path"] == "fused"
        runs.append((state(tr), [float(x) for x in losses]))
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), (k, float((runs[0][0][k] - runs[1][0][k]).abs().max()))
    assert runs[0][1] == runs[1][1]


def expected_trace(opt, n_iters, n_cams, n_pseudo):
    """the schedule of FSGS/train.py:81-176 without a model: cameras, SH degree, rates, weights, events, path"""
    rng = random.Random(opt.seed)
    stack, pstack, sh, lr, w = [], [], 0, 0.00016, opt.depth_weight
    out = []
    for it in range(1, n_iters + 1):
        if it % opt.sh_increase_interval == 0:
            sh = min(sh + 1, 3)
        if not stack:
            stack = list(range(n_cams))
        ci = stack.pop(rng.randint(0, len(stack) - 1))
        pseudo = it % opt.sample_pseudo_interval == 0 and opt.start_sample_pseudo < it < opt.end_sample_pseudo
        if pseudo:
            if not pstack:
                pstack = list(range(n_pseudo))
            pstack.pop(rng.randint(0, len(pstack) - 1))
        dens = it < opt.densify_until_iter and it > opt.densify_from_iter and it % opt.densification_interval == 0
        stepped = it < opt.iterations and not dens
        reset = (it - opt.start_sample_pseudo - 1) % opt.opacity_reset_interval == 0 and it > opt.start_sample_pseudo
        out.append(dict(camera=ci, sh_degree=sh, xyz_lr=lr, depth_weight=w, stepped=stepped, densified=dens, reset=reset,
                        pseudo=pseudo, path="fused" if stepped and not pseudo else "unfused"))
        if it > opt.end_sample_pseudo:
            w = 0.001
        lr = expon_lr(it, 0.00016, opt.position_lr_final, lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
    return out


def test_train_iteration_through_a_densification_and_a_pseudo_iteration(hip):
    """The compressed schedule, fused: iteration 4 densifies (un-fused, no step), 5 resets the opacities after its step, 6 is a
    pseudo iteration (un-fused on purpose: two views, one Adam step), 7 and 8 are stepped fused again - with the
    densification on the host and on the device: the same counts and the same P (the input conditions of
    tests/test_fsgs_densify_cpu.py are asserted in front of it)."""
    from test_gpu_fsgs_densify import conditions_hold
    import fsgs_densify_reference as fr
    extent, thr = 0.015, dict(dist_thres=8.0, prune_from_iter=2, proximity_until_iter=100)
    runs = []
    for flag in (False, True):
        tr = make(hip, True, P=300, W=96, H=80, deg=0, pseudo=True, sc=synthetic.trained_like(300, seed=0, scale_mult=1.5))
        inner = tr.model.densify_and_prune_fsgs

        def checked(max_grad, min_opacity, ext, screen, it, *, _inner=inner, _m=tr.model, **kw):
            info = conditions_hold(hip, _m, it, screen=screen, max_grad=max_grad, min_opacity=min_opacity, extent=ext,
                                   generator=kw["generator"], **{k: kw[k] for k in thr})
            assert fr.neighbours_are_separated(info["knn1"]) and fr.neighbours_are_separated(info["knn2"])
            assert fr.smallest_margin(info, _m.xyz_gradient_accum.cpu(), _m.denom.cpu(), 2, screen, _m.percent_dense, ext,
                                      kw["dist_thres"], max_grad, min_opacity, constructed=False) > 1e-5
            return _inner(max_grad, min_opacity, ext, screen, it, **kw)
        tr.model.densify_and_prune_fsgs = checked
        opt = FsgsOptions(iterations=40, position_lr_max_steps=40, densify_from_iter=3, densification_interval=4, densify_until_iter=7,
                          opacity_reset_interval=100, start_sample_pseudo=4, end_sample_pseudo=9, sample_pseudo_interval=3,
                          sh_increase_interval=5, cameras_extent=extent, densify_grad_threshold=1e-7, seed=3,
                          densify_on_device=flag, **thr)
        log = [tr.train_iteration(it, opt) for it in range(1, 9)]
        torch.cuda.synchronize()
        runs.append((log, state(tr), tr, opt))
    (off, s_off, tr_off, opt), (on, s_on, tr_on, _) = runs
    want = expected_trace(opt, 8, 4, 3)
    assert [w["path"] for w in want] == ["fused", "fused", "fused", "unfused", "fused", "unfused", "fused", "fused"]
    for log in (off, on):
        got = [dict(camera=r["camera"], sh_degree=r["sh_degree"], xyz_lr=r["xyz_lr"], depth_weight=r["depth_weight"],
                    stepped=r["stepped"], densified=r["densified"] is not None, reset=r["reset"], pseudo=r["pseudo"], path=r["path"])
               for r in log]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]
        assert all(bool(torch.isfinite(torch.as_tensor(r["loss"]))) for r in log)
        assert [r["P"] for r in log[:3]] == [300] * 3 and log[3]["P"] != 300 and all(r["P"] == log[3]["P"] for r in log[4:])
    assert on[3]["densified"] == off[3]["densified"] and len(on[3]["densified"]) == 4 and on[3]["P"] == off[3]["P"]
    for tr in (tr_off, tr_on):
        o = tr.model.optimizer
        assert o.t == 7 and o.seg_steps["xyz"] == 7       # iteration 4 took no step
        assert float(tr.model.denom.max()) >= 1.0


def test_what_is_closed_to_this_trainer_on_the_gpu(hip):
    from gsplat_amd.trainer import GraphedStep
    tr = make(hip, True, P=1023, W=160, H=128)
    with pytest.raises(RuntimeError, match="GraphedStep"):
        GraphedStep(tr)
    # the side launch is never armed for this generation, however small the two-phase threshold
    hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = True, 0
    n0 = hip.two_phase_launches
    try:
        tr.step(0)
        torch.cuda.synchronize()
    finally:
        del hip.TWO_PHASE, hip.TWO_PHASE_MIN_P
    assert tr.last["path"] == "fused" and hip.two_phase_launches == n0

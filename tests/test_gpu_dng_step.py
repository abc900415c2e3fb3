"""gs_depth_backward_step on the GPU: a DNGaussian depth leg's backward with Adam on the leg's one tensor in the per-Gaussian
tail (csrc/gs_depth_pass.hip: depth_point_step_kernel) against what it replaces - gs_depth_backward, gs_activations_bwd's
opacity line for the soft leg, gs_adam_step on that tensor - bit for bit.

Every comparison is torch.equal: the two sides evaluate the same expressions on the same float64 blend sums (rows-given form:
literally the same rows; live form: rows of a second blend backward over the same lists and cotangents)."""
import ctypes as C

import pytest
import torch

import blend_cases
import dense_reference
import depth_pass_reference as dpr
from gsplat_amd import synthetic
from gsplat_amd.capi import DEPTH_STEP_ROWS_GIVEN, GsAdamSeg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = (1, 3, 255, 257, 1023, 4099)   # one thread, a partial wave, one row short of / past a 256-row block, several blocks
IMAGES = ((160, 128), (150, 100))      # on and off the 16-pixel tile grid
BETAS, EPS, GUARD = (0.9, 0.999), 1e-15, 64
LR = {1: 0.00016, 2: 0.05}


@pytest.fixture(params=[False, True], ids=["lists_reference", "lists_culled"])
def cull(hip, request):
    old = hip.tile_cull
    hip.tile_cull = request.param
    yield request.param
    hip.tile_cull = old


def make_scene(P, cam, seed):
    """P Gaussians in the orbit cameras' box, every third one mirrored behind the camera (outside every frustum: radius 0,
    zero gradient), raw opacities, and a moment state with signs and magnitudes of a run in progress."""
    g = torch.Generator().manual_seed(1000 * seed + P)
    xyz = torch.rand((P, 3), generator=g) * 2.6 - 1.3
    out = torch.arange(P) % 3 == 2
    xyz[out] = xyz[out] * 0.2 + 2.0 * cam.camera_center[None]
    scales = torch.exp(torch.log(torch.tensor(0.08)) + 0.6 * torch.randn((P, 3), generator=g))
    q = torch.randn((P, 4), generator=g)
    raw_op = 2.0 * torch.randn((P, 1), generator=g)
    return dict(means3D=xyz, scales=scales, rotations=q / q.norm(dim=1, keepdim=True), raw_opacity=raw_op, outside=out)


def covariance(sc):
    R = dense_reference.quat_to_rot(sc["rotations"].double())
    S = torch.diag_embed(sc["scales"].double())
    Sig = (R @ S @ S @ R.transpose(1, 2)).float()
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], dim=1).contiguous()


def activate(hip, raw_op):
    """sigmoid through gs_activations_fwd: the activated row whose bits gs_activations_bwd recomputes from the raw one"""
    P = raw_op.shape[0]
    s3, r4 = torch.zeros((P, 3), device=DEV), torch.ones((P, 4), device=DEV)
    o_s, o_r, o_o = torch.empty_like(s3), torch.empty_like(r4), torch.empty_like(raw_op)
    hip.api.call("activations_fwd", s3.data_ptr(), r4.data_ptr(), raw_op.data_ptr(), P, o_s.data_ptr(), o_r.data_ptr(),
                 o_o.data_ptr(), hip._stream(DEV))
    return o_o


def sigmoid_backward(hip, raw_op, g_act):
    """gs_activations_bwd's opacity line (the scale and rotation lines run on dummies)"""
    P = raw_op.shape[0]
    s3, r4 = torch.zeros((P, 3), device=DEV), torch.ones((P, 4), device=DEV)
    d_s, d_r, d_o = torch.empty_like(s3), torch.empty_like(r4), torch.empty_like(raw_op)
    hip.api.call("activations_bwd", s3.data_ptr(), r4.data_ptr(), raw_op.data_ptr(), P, s3.data_ptr(), r4.data_ptr(),
                 g_act.contiguous().data_ptr(), d_s.data_ptr(), d_r.data_ptr(), d_o.data_ptr(), hip._stream(DEV))
    return d_o


def adam_step(hip, p, g, m, v, lr, step):
    seg = (GsAdamSeg * 1)()
    seg[0].begin, seg[0].end, seg[0].lr_a, seg[0].step = 0, p.numel(), float(lr), int(step)
    hip.api.call("adam_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), seg, 1, BETAS[0], BETAS[1], EPS,
                 int(step), hip._stream(DEV))


class Guarded:
    """a tensor of `shape` between two runs of GUARD words that nobody may write"""
    WORD = 0x7FC0DE01

    def __init__(self, src):
        n = src.numel()
        self.buf = torch.full((n + 2 * GUARD,), self.WORD, dtype=torch.int32, device=DEV).view(torch.float32)
        self.t = self.buf[GUARD:GUARD + n].view(src.shape)
        self.t.copy_(src)

    def intact(self):
        w = self.buf.view(torch.int32)
        return bool((w[:GUARD] == self.WORD).all()) and bool((w[-GUARD:] == self.WORD).all())


def forward(hip, sc, cam, means, act_op, which, form):
    op = act_op if which == 2 else torch.full_like(act_op, 0.95)
    shape = (sc["scales"].to(DEV), sc["rotations"].to(DEV), None) if form == "scales_rotations" else (None, None, covariance(sc).to(DEV))
    return hip.depth_forward(means, op, *shape, 1.0, torch.zeros(3, device=DEV), cam.world_view_transform.to(DEV),
                             cam.full_proj_transform.to(DEV), cam.camera_center.to(DEV), cam.tanfovx, cam.tanfovy, cam.image_height,
                             cam.image_width)


def workspace(P):
    return torch.zeros((((P * 128 + 255) // 256) * 256 + 2 * GUARD * 4,), dtype=torch.uint8, device=DEV)


def one_comparison(hip, P, W, H, which, form, steps):
    cam = synthetic.orbit_cameras(W, H)[3]
    sc = make_scene(P, cam, seed=which + (0 if form == "scales_rotations" else 2))
    g = torch.Generator().manual_seed(77 + P)
    n = 3 if which == 1 else 1
    dd, da = (t.to(DEV) for t in dpr.cotangents(H, W, 9))
    means0, raw0 = sc["means3D"].to(DEV), sc["raw_opacity"].to(DEV)
    m0 = (1e-3 * torch.randn((P, n), generator=g)).to(DEV)
    v0 = (1e-6 * torch.rand((P, n), generator=g)).to(DEV)
    out = sc["outside"].to(DEV)
    still = out & (torch.arange(P, device=DEV) % 2 == 0)   # culled rows without a history: every bit must stay
    m0[still], v0[still] = 0.0, 0.0
    state = ((means0 if which == 1 else raw0).clone(), m0, v0)
    saw_gradient = False
    for step in steps:
        p0, m0, v0 = state
        means = p0 if which == 1 else means0
        raw = p0 if which == 2 else raw0
        act = activate(hip, raw)
        # -- what the entry replaces: gs_depth_backward -> [sigmoid backward] -> gs_adam_step
        depth, alpha, radii, rec = forward(hip, sc, cam, means.clone(), act, which, form)
        ws = workspace(P)
        wsv = ws[GUARD * 4: ws.numel() - GUARD * 4]
        dm3, dm2, dop = hip.depth_backward(rec, dd, da, which, workspace=wsv)
        grad = dm3 if which == 1 else sigmoid_backward(hip, raw, dop)
        saw_gradient |= bool((grad != 0).any())
        assert not bool((grad[out] != 0).any()), "a Gaussian behind the camera has a gradient"
        ref = [t.clone() for t in (p0, m0, v0)]
        adam_step(hip, ref[0], grad.contiguous(), ref[1], ref[2], LR[which], step)
        # -- rows-given form: the rows that call left in the workspace, no cotangents
        given = [Guarded(t) for t in (p0, m0, v0)]
        rows_before = wsv.clone()
        hip.depth_backward_step(rec, None, None, which, given[0].t, given[1].t, given[2].t, LR[which], step, BETAS, EPS,
                                flags=DEPTH_STEP_ROWS_GIVEN, workspace=wsv)
        assert torch.equal(wsv, rows_before), "ROWS_GIVEN: the rows were written"
        # -- live form: its own forward and blend, the parameter being the very tensor the forward read
        live = [Guarded(t) for t in (p0, m0, v0)]
        lmeans = live[0].t if which == 1 else means0.clone()
        lact = act.clone()
        inputs = [t.clone() for t in (lmeans, lact, dd, da)]
        _, _, lradii, lrec = forward(hip, sc, cam, lmeans, lact, which, form)
        lws = workspace(P)
        lws.fill_(0x5A)   # (the live form zeroes what it reads)
        hip.depth_backward_step(lrec, dd, da, which, live[0].t, live[1].t, live[2].t, LR[which], step, BETAS, EPS,
                                workspace=lws[GUARD * 4: lws.numel() - GUARD * 4])
        torch.cuda.synchronize()
        assert torch.equal(lradii, radii)
        for name, a, b in (("rows given", given, ref), ("live", live, ref)):
            for what, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
                diff = int((x.t.view(torch.int32) != y.view(torch.int32)).sum())
                assert diff == 0, "%s, P=%d %dx%d which=%d %s step %d: %s differs in %d of %d elements (max %.3e)" % (
                    name, P, W, H, which, form, step, what, diff, y.numel(), float((x.t - y).abs().max()))
                assert x.intact(), "%s: a word next to %s was written" % (name, what)
        for wsb in (ws, lws):
            for edge in (wsb[:GUARD * 4], wsb[-GUARD * 4:]):
                assert bool((edge == edge[0]).all()), "a byte next to the workspace was written"
        if which == 2:   # nothing but param / moments: the inputs of the live call keep their bits
            assert torch.equal(lmeans, inputs[0])
        assert torch.equal(lact, inputs[1]) and torch.equal(dd, inputs[2]) and torch.equal(da, inputs[3])
        # -- rows without a gradient
        moved = out & ~still
        if bool(moved.any()):   # zero gradient, a history: the moments decay and the parameter moves, as Adam says
            assert bool((ref[1][moved] != m0[moved]).any()) and bool((ref[0][moved] != p0[moved]).any())
            assert torch.equal(live[1].t[moved], (BETAS[0] * m0[moved]))
        if bool(still.any()):   # zero gradient, no history: every bit stays
            for x, y in zip(live, (p0, m0, v0)):
                assert torch.equal(x.t[still].view(torch.int32), y[still].view(torch.int32))
        state = tuple(ref)
    return saw_gradient


@pytest.mark.parametrize("P", SIZES)
def test_the_fused_tail_is_backward_plus_adam_bit_for_bit(hip, cull, P):
    """parameters and both moments after gs_depth_backward_step - rows given and live - equal gs_depth_backward [+ the sigmoid
    line] + gs_adam_step over steps 1, 2, 3 of one evolving state, for both legs, both image sizes, both input forms"""
    seen = 0
    for (W, H) in IMAGES:
        for which in (1, 2):
            for form in ("scales_rotations", "cov3D_precomp"):
                seen += one_comparison(hip, P, W, H, which, form, (1, 2, 3))
    assert P < 255 or seen == 8, "a combination never produced a gradient: it checked only the zero-gradient update"


@pytest.mark.parametrize("which", [1, 2])
def test_a_late_step_count(hip, cull, which):
    """step = 1000: both bias corrections are far from their first values"""
    assert one_comparison(hip, 1023, 150, 100, which, "scales_rotations", (1000,))


def test_status_codes(hip):
    """the C ABI's argument rules, straight through the entry point: status codes, no launch"""
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
    case = blend_cases.build("len_65")
    sc, cam = case.scene_sr, case.cam
    W, H, P = case.W, case.H, sc["means3D"].shape[0]
    keep = []
    means = sc["means3D"].to(DEV)

    def structs(antialiasing=False, **gkw):
        view = hip._view(keep, DEV, case.bg, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, cam.tanfovx,
                         cam.tanfovy, H, W, 1.0, 0, False, antialiasing, False, tile_cull=0)
        g = hip._gauss(keep, DEV, means, None, means, sc["opacities"], sc["scales"], sc["rotations"], None)
        for k, v in gkw.items():
            setattr(g, k, v)
        return view, g
    gb, ib, _, _ = hip.scratch_bytes(P, W, H, 0)
    geom = torch.zeros((gb,), dtype=torch.uint8, device=DEV)
    img = torch.zeros((ib,), dtype=torch.uint8, device=DEV)
    s = hip._scratch(geom, img, None, 0)
    f = lambda n: torch.zeros((n,), device=DEV)   # noqa: E731
    depth, alpha, radii = f(W * H), f(W * H), torch.zeros((P,), dtype=torch.int32, device=DEV)
    p, m, v, ws = f(3 * P), f(3 * P), f(3 * P), torch.zeros((P * 128 + 256,), dtype=torch.uint8, device=DEV)
    fn = hip.api.raw("depth_backward_step")
    stream = hip._stream(DEV)

    def call(view, g, which=1, step=1, flags=0, p=p, m=m, v=v, w=ws, wbytes=None, rad=radii):
        q = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        return fn(C.byref(view), C.byref(g), q(rad), C.byref(s), 0, depth.data_ptr(), alpha.data_ptr(), which, q(p), q(m), q(v),
                  1e-3, step, 0.9, 0.999, 1e-15, flags, q(w), ws.numel() if wbytes is None else wbytes, stream)
    view, g = structs()
    va, _ = structs(antialiasing=True)
    assert call(va, g) == E_UNSUPPORTED
    assert call(view, g, p=None) == E_NULL and call(view, g, m=None) == E_NULL and call(view, g, v=None) == E_NULL
    for which in (0, 3, -1):
        assert call(view, g, which=which) == E_SHAPE
    assert call(view, g, step=0) == E_SHAPE and call(view, g, step=-5) == E_SHAPE
    for flags in (2, 4, 3, -2):
        assert call(view, g, flags=flags) == E_UNSUPPORTED
    x = f(P)
    for gkw in (dict(raw_activations=1), dict(shs_rest=x.data_ptr()), dict(extra_channel=x.data_ptr())):
        _, gx = structs(**gkw)
        assert call(view, gx) == E_UNSUPPORTED, gkw
    assert call(view, g, w=None) == E_NULL and call(view, g, rad=None) == E_NULL
    assert call(view, g, wbytes=P * 128 - 1) == -3    # GS_E_SCRATCH
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert float(t.abs().max()) == 0, "a refused call wrote"
    # P == 0: GS_OK without a launch, in both forms, with nothing to point at
    _, g0 = structs(P=0)
    assert call(view, g0, w=None, rad=None) == 0 and call(view, g0, which=2, flags=DEPTH_STEP_ROWS_GIVEN) == 0
    # the accepted forms answer GS_OK (no instances: num_rendered 0 skips the blend, every row gets its zero-gradient update)
    assert call(view, g) == 0 and call(view, g, which=2, flags=DEPTH_STEP_ROWS_GIVEN) == 0


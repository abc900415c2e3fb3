"""csrc/gs_model.hip on an MI355X, and the copies of its activation arithmetic, held to tests/model_ops_reference.py:

  * gs_activations_fwd / gs_activations_bwd against the float64 restatement at the per-element bars, on every row of the case
    table (clamp, tie, saturation, overflow, subnormal results) at every row count, and on an ordinary random draw;
  * the copy in csrc/gs_math.h (GsGaussians.raw_activations): a scene whose raw rows come from the case table, rendered on the
    raw rows and on the tensors gs_activations_fwd wrote - images, radii and the exported per-Gaussian state bit for bit, both
    rasterizer generations;
  * the copy in csrc/gs_preprocess_bwd.hip: the same rows as a trainer's model, three fused steps against the four kernels on
    pinned blend sums, bit for bit (the harnesses of tests/test_gpu_fsgs_step.py and tests/test_gpu_step_layout.py);
  * gs_densify_stats at workgroup edges with radii and gradients at the ends of their ranges, exact;
  * the depth legs' opacity step (csrc/gs_depth_pass.hip), the sigmoid's backward on the stored s, at saturated opacities;
  * gs_rows_pack / gs_rows_unpack called directly, against numpy indexing, bit for bit.

Every test prints the largest distance it saw, in units of its bar (DESIGN.md section 4.15 keeps one run's figures)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dc_cases
import model_ops_reference as mr
from gsplat_amd import synthetic
from gsplat_amd.trainer import _stream_of, camera_to
from test_gpu_step_layout import one_binning_path  # noqa: F401  (autouse here too: both runs of a pair on the same lists)
from test_model_ops import raw, run_api, stats_reference
from test_model_ops_cases_cpu import api_outputs, tie_example

pytestmark = pytest.mark.gpu


def show(what, worst):
    print("%s: largest distance / bar  %s" % (what, "  ".join("%s %.3f" % (k, v) for k, v in worst.items())))


# ---- the kernels themselves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", mr.SIZES)
def test_activation_kernels_on_the_case_table(hip, P):
    c = mr.cases(P)
    show("P = %d" % P, mr.check_all(api_outputs(hip.api, c, P, "cuda"), c, "hip "))


def test_activation_kernels_on_an_ordinary_draw(hip):
    """tests/test_model_ops.py's inputs (P = 100003, one draw), each element at its own bar"""
    scaling, rotation, opacity, grads = raw(100003, 2)
    outs, d = run_api(hip.api, scaling.cuda(), rotation.cuda(), opacity.cuda(), grads)
    got = dict(zip(mr.OUTPUTS, (x.cpu().numpy() for x in (outs[0], outs[1], outs[2], d[0], d[1], d[2]))))
    args = [t.numpy() for t in (scaling, rotation, opacity) + tuple(grads)]
    ref = mr.restate(*args)
    show("P = 100003", mr.check_all(got, dict(ref=ref, bar=mr.bars(*args, ref))))


def test_the_kernel_projects_at_the_tie(hip):
    q, g = tie_example()
    z3, z1 = torch.zeros((1, 3)).cuda(), torch.zeros((1, 1)).cuda()
    _, d = run_api(hip.api, z3, torch.from_numpy(q).cuda(), z1, (z3, torch.from_numpy(g), z1))
    d = d[1].cpu().numpy()[0]
    print("act_bwd_kernel at q = (eps32, 0, 0, 0), g = (1, 2, 3, 4):", d)
    assert abs(float(d[0])) <= 48 * mr.U * 1.0 / mr.EPS       # (g / eps32 would be 1e12)
    assert np.all(np.abs(d[1:] - g[0, 1:] / mr.EPS) <= 2 * mr.U * g[0, 1:] / mr.EPS)


# ---- a scene of the table's rows ------------------------------------------------------------------------------------------
RENDER_OPACITIES = (-20.0, -5.0, 0.0, 5.0, 20.0)
RENDER_SCALINGS = (-6.0, -5.0, -4.0, -3.0, -2.0, -1.0, -30.0)
EYE, TARGET = np.array([0.1, -0.2, 0.15]), np.array([1.3, 0.3, 0.0])     # dc_cases.inside_camera


def render_rows(P, W, H):
    """P raw rows in the model's flat order, every one in front of dc_cases.inside_camera(W, H): every rotation row of the table,
    the raw opacities and scales of it that leave something to render (cycles of 57, 5 and 7 rows).  -> flat [59 P] fp32"""
    g = np.random.default_rng(7)
    flat = (g.standard_normal(59 * P) * 0.3).astype(np.float32)
    t = mr.views(flat, P)
    fwd = (TARGET - EYE) / np.linalg.norm(TARGET - EYE)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    tanx = np.tan(0.5 * 0.6911112070083618)
    d = g.uniform(1.5, 4.0, P)
    x, y = g.uniform(-0.8, 0.8, P) * d * tanx, g.uniform(-0.8, 0.8, P) * d * tanx * H / W
    t["xyz"][:] = EYE + d[:, None] * fwd + x[:, None] * right + y[:, None] * down
    i, e = np.arange(P), np.arange(3 * P)
    t["rotation"][:] = mr.ROTATIONS[i % len(mr.ROTATIONS)]
    t["opacity"][:, 0] = np.float32(RENDER_OPACITIES)[i % 5]
    t["scaling"][:] = np.float32(RENDER_SCALINGS)[e % 7].reshape(P, 3)
    return flat


def branch_of(P):
    kind = mr.ROTATION_KINDS[np.arange(P) % len(mr.ROTATIONS)]
    return {"tie": kind == "tie", "clamped": np.isin(kind, ("below", "clamped")), "projected": np.isin(kind, ("above", "projected"))}


def forward(hip, cam, W, H, t, activated, fsgs):
    """One forward on the raw rows `t` (activated = None) or on the activated tensors -> its images, radii and exported state"""
    e = torch.empty(0)
    op, sc, rot = (t["opacity"], t["scaling"], t["rotation"]) if activated is None else activated
    hip.raw_activations = activated is None
    out = hip.rasterize_gaussians(torch.tensor([0.1, 0.2, 0.3]).cuda(), t["xyz"], e, op, sc, rot, 1.0, e, cam.world_view_transform,
                                  cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, t["features"].view(-1, 16, 3), 3,
                                  cam.camera_center, False, False, False, fsgs=fsgs)
    R, color, radii, geom, binning, img, depth = out[:7]
    got = dict(color=color, radii=radii)
    got["depth" if fsgs else "invdepth"] = depth
    if fsgs:
        got["alpha"] = out[7]
    st = hip.export_state(t["xyz"].shape[0], W, H, R, geom, binning, img)
    got.update({"state." + k: v for k, v in st.items()})
    assert not hip.raw_activations and R > 0
    return got


@pytest.mark.parametrize("fsgs", [False, True], ids=["plain", "fsgs"])
@pytest.mark.parametrize("size", [(64, 48), (37, 53)], ids=["64x48", "37x53"])
def test_raw_rows_render_the_bits_of_the_activated_tensors(hip, size, fsgs):
    W, H = size
    P = 257     # (the rotation rows start at byte 220 P: off the 16-byte grid)
    t = mr.views(torch.from_numpy(render_rows(P, W, H)).cuda(), P)
    cam = camera_to(dc_cases.inside_camera(W, H), torch.device("cuda"))
    outs = [torch.empty_like(t[k]) for k in ("scaling", "rotation", "opacity")]
    hip.api.call("activations_fwd", t["scaling"].data_ptr(), t["rotation"].data_ptr(), t["opacity"].data_ptr(), P,
                 *[o.data_ptr() for o in outs], _stream_of(t["scaling"]))
    old = hip.scratch_fill
    hip.scratch_fill = lambda kind, buf: buf.zero_()      # (rows the geometry phase culls export what the buffer held)
    try:
        a = forward(hip, cam, W, H, t, None, fsgs)
        b = forward(hip, cam, W, H, t, (outs[2], outs[0], outs[1]), fsgs)
    finally:
        hip.scratch_fill = old
    assert set(a) == set(b)
    for k in a:
        assert dc_cases.same_bits(a[k], b[k]), "%s differs" % k
    radii = a["radii"].cpu().numpy()
    seen = {k: int((radii[rows] > 0).sum()) for k, rows in branch_of(P).items()}
    print("%dx%d %s: Gaussians with radii > 0 per rotation branch %s, %d instances" % (W, H, "fsgs" if fsgs else "plain", seen,
                                                                                    a["state.point_list"].numel()))
    assert all(n > 0 for n in seen.values()) and float(a["color"].abs().max()) > 0


# ---- the copy in the fused tails ------------------------------------------------------------------------------------------
def install(tr, P, W, H):
    """the case rows as the trainer's model, three cameras around dc_cases.inside_camera in place of its orbit"""
    t = mr.views(torch.from_numpy(render_rows(P, W, H)), P)
    with torch.no_grad():
        for k, v in t.items():
            tr.model.params[k].copy_(v.view_as(tr.model.params[k]))
    dev = tr.model.flat.device
    eyes = [EYE, EYE + [0.0, 0.05, 0.0], EYE + [0.0, 0.0, -0.05]]
    cams = [camera_to(synthetic.look_at_camera(tuple(eye), W, H, target=tuple(TARGET)), dev) for eye in eyes]
    tr.cameras = cams + list(tr.cameras[len(cams):])
    return tr


@pytest.mark.parametrize("P", [3, 257])
def test_fused_tail_of_the_fsgs_generation_on_the_case_rows(hip, P):
    import test_gpu_fsgs_step as fs
    W, H = 64, 48
    a, b = (install(fs.make(hip, fused, P=P, W=W, H=H), P, W, H) for fused in (False, True))
    start = a.model.flat.detach().clone()
    sa = fs.fused_equals_the_four_kernels(hip, a, b)
    moved = (sa["flat"] != start).view(-1)
    rot = mr.views(moved, P)["rotation"].any(1).cpu().numpy()
    seen = {k: int(rot[rows].sum()) for k, rows in branch_of(P).items()}
    print("P = %d: rotation rows that moved per branch %s" % (P, seen))
    assert float(sa["denom"].max()) == 3.0 and bool(torch.isfinite(sa["flat"]).all())
    assert seen["tie"] > 0 and (P == 3 or (seen["clamped"] > 0 and seen["projected"] > 0))


@pytest.mark.parametrize("P", [3, 257])
def test_fused_tail_on_the_case_rows(hip, P):
    """gs_backward_step (one launch and two phases) against gs_backward + gs_activations_bwd + gs_densify_stats + gs_adam_step:
    form A of tests/test_gpu_step_layout.py, its restatement R included"""
    import step_reference as sr
    import test_gpu_step_layout as sl
    for two_phase in (False, True):
        hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = two_phase, 0
        a, b = (install(sl.make(hip, P, fused), P, sr.W, sr.H) for fused in (False, True))
        sl.run_pair(hip, a, b, [0, 1, 2], "case rows P %d two_phase %d" % (P, two_phase), False)
        assert float(a.model.denom.max()) == 3.0 and bool(torch.isfinite(a.model.flat).all())


def test_the_depth_legs_opacity_step_on_saturated_opacities(hip, monkeypatch):
    """depth_point_step_kernel (csrc/gs_depth_pass.hip) holds one more copy of the sigmoid's backward, g (1 - s) s on the STORED
    s: tests/test_gpu_dng_step.py's comparison - gs_depth_backward_step against gs_depth_backward + gs_activations_bwd's opacity
    line + gs_adam_step, bit for bit over three steps - with the table's raw opacities that render, out to where s rounds to 1."""
    import test_gpu_dng_step as ds
    inner = ds.make_scene
    values = torch.tensor(RENDER_OPACITIES + (16.6, -16.6, 17.5, -17.5, 30.0, -30.0, 1e-8, 10.0))

    def scene(P, cam, seed):
        sc = inner(P, cam, seed)
        sc["raw_opacity"] = values[torch.arange(P) % len(values)].reshape(P, 1).clone()
        return sc
    monkeypatch.setattr(ds, "make_scene", scene)
    old = hip.tile_cull
    try:
        for cull in (False, True):
            hip.tile_cull = cull
            assert ds.one_comparison(hip, 257, 150, 100, 2, "scales_rotations", (1, 2, 3))
    finally:
        hip.tile_cull = old


# ---- gs_densify_stats -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_densify_stats_at_the_ends_of_its_ranges(hip, P):
    g = np.random.default_rng(P)
    i = np.arange(P)
    radii = np.array([1, 2 ** 31 - 1, 0, -1, 2], np.int32)[i % 5]
    grad = (g.standard_normal((P, 3)) * 1e-3).astype(np.float32)
    vis = radii > 0
    kind = i % 7
    grad[kind == 0, :2] = (3e-3, 4e-3)
    grad[kind == 1, :2] = (1e-40, 2e-41)          # subnormal: the squares underflow to 0
    grad[kind == 2, :2] = (1e30, -1e30)           # the squares overflow: the norm is inf
    grad[~vis & (kind >= 3), :2] = np.nan         # an invisible row is never read
    mr0 = (g.random(P) * 30).astype(np.float32)
    mr0[kind == 4] = 3e9                          # above float(2^31 - 1) = 2147483648: max keeps it
    acc0, den0 = g.random((P, 1)).astype(np.float32), g.integers(0, 5, (P, 1)).astype(np.float32)
    want_mr, _, want_den = stats_reference(torch.from_numpy(radii), torch.from_numpy(grad), torch.from_numpy(mr0.copy()),
                                           torch.from_numpy(acc0.copy()), torch.from_numpy(den0.copy()))
    with np.errstate(over="ignore", under="ignore"):
        gx, gy = grad[:, 0], grad[:, 1]
        norm = np.sqrt((gx * gx).astype(np.float32) + (gy * gy).astype(np.float32), dtype=np.float32)
        want_acc = np.where(vis[:, None], (acc0[:, 0] + norm).astype(np.float32)[:, None], acc0)
    dev = [torch.from_numpy(x.copy()).cuda() for x in (radii, grad, mr0, acc0, den0)]
    hip.api.call("densify_stats", dev[0].data_ptr(), dev[1].data_ptr(), P, dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                 _stream_of(dev[0]))
    got_mr, got_acc, got_den = (x.cpu() for x in dev[2:])
    assert torch.equal(got_mr, want_mr) and torch.equal(got_den, want_den)
    assert np.array_equal(got_acc.numpy().view(np.int32), want_acc.view(np.int32))
    for got, before in ((got_mr.numpy(), mr0), (got_acc.numpy()[:, 0], acc0[:, 0]), (got_den.numpy()[:, 0], den0[:, 0])):
        assert np.array_equal(got.view(np.int32)[~vis], before.view(np.int32)[~vis])
    if P >= 255:
        assert float(got_mr.max()) == 3e9 and (got_mr == 2147483648.0).any() and np.isinf(want_acc).any()
        assert np.isnan(grad[~vis]).any() and not np.isnan(got_acc.numpy()).any()


# ---- gs_rows_pack / gs_rows_unpack ----------------------------------------------------------------------------------------
MODEL_WIDTHS = (3, 48, 1, 3, 4)
PACK_CASES = [
    # name, widths, P, mask kind, K kind
    ("model", MODEL_WIDTHS, 257, "half", "some"),
    ("model + 60th column", MODEL_WIDTHS + (1,), 257, "half", "some"),
    ("eight fields, empty ones in the middle and at the end", (2, 3, 0, 5, 1, 4, 7, 0), 257, "half", "some"),
    ("one row", MODEL_WIDTHS, 1, "ones", "some"),
    ("mask all 0", MODEL_WIDTHS, 257, "zeros", "some"),
    ("mask all 1", MODEL_WIDTHS, 257, "ones", "some"),
    ("K = 1", MODEL_WIDTHS, 257, "half", "one"),
    ("more elements than one pass of the grid", MODEL_WIDTHS, 300_000, "half", "some"),   # 59 P > 65536 * 256
]


def pack_case(widths, P, mask_kind, k_kind, seed):
    """-> flat [P W] fp32, mask [P] uint8, pos [P] int32, K.  Selected rows get distinct positions; a few of them get -1 or K
    (skipped); rows outside the mask hold positions that would be valid (the mask alone must keep them out)."""
    g = np.random.default_rng(seed)
    W = sum(widths)
    flat = g.standard_normal(P * W).astype(np.float32)
    mask = {"half": (g.random(P) < 0.5), "ones": np.ones(P, bool), "zeros": np.zeros(P, bool)}[mask_kind].astype(np.uint8)
    n = int(mask.sum())
    K = 1 if k_kind == "one" else max(n, 1)
    pos = g.integers(0, K, P).astype(np.int32)
    order = g.permutation(n).astype(np.int32)
    pos[mask != 0] = order if k_kind != "one" else np.where(order == 0, 0, K)      # (K = 1: one row lands, the rest are out of range)
    chosen = np.nonzero(mask)[0]
    if k_kind != "one" and n >= 8:
        pos[chosen[::5]] = -1
        pos[chosen[1::7]] = K
    return flat, mask, pos, K


def blocks(buf, rows, widths):
    out, off = [], 0
    for w in widths:
        out.append(buf[off:off + rows * w].reshape(rows, w))
        off += rows * w
    return out


def call_pack(hip, name, flat, P, widths, mask, pos, K, packed):
    w = (C.c_int32 * len(widths))(*widths)
    hip.api.call(name, flat.data_ptr(), P, len(widths), w, mask.data_ptr(), pos.data_ptr(), K, packed.data_ptr(), _stream_of(flat))


@pytest.mark.parametrize("case", PACK_CASES, ids=[c[0].replace(" ", "_") for c in PACK_CASES])
def test_rows_pack_and_unpack_against_numpy_indexing(hip, case):
    name, widths, P, mask_kind, k_kind = case
    flat, mask, pos, K = pack_case(widths, P, mask_kind, k_kind, seed=len(name) + P)
    W = sum(widths)
    rows = np.nonzero((mask != 0) & (pos >= 0) & (pos < K))[0]
    assert len(np.unique(pos[rows])) == len(rows) and (mask_kind == "zeros") == (len(rows) == 0)
    # pack: the reference is numpy indexing into a NaN-filled destination
    want = np.full(K * W, np.nan, np.float32)
    for src, dst in zip(blocks(flat, P, widths), blocks(want, K, widths)):
        dst[pos[rows]] = src[rows]
    d_flat, d_mask, d_pos = (torch.from_numpy(x).cuda() for x in (flat, mask, pos))
    packed = torch.full((K * W,), float("nan"), device="cuda")
    call_pack(hip, "rows_pack", d_flat, P, widths, d_mask, d_pos, K, packed)
    assert np.array_equal(packed.cpu().numpy().view(np.int32), want.view(np.int32)), name
    assert np.array_equal(d_flat.cpu().numpy().view(np.int32), flat.view(np.int32))      # (the source is not written)
    # unpack into a NaN-filled model: the union's rows come back, no other element is touched
    want_flat = np.full(P * W, np.nan, np.float32)
    for dst, src in zip(blocks(want_flat, P, widths), blocks(want, K, widths)):
        dst[rows] = src[pos[rows]]
    back = torch.full((P * W,), float("nan"), device="cuda")
    call_pack(hip, "rows_unpack", back, P, widths, d_mask, d_pos, K, packed)
    got = back.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want_flat.view(np.int32)), name
    for mine, theirs in zip(blocks(got, P, widths), blocks(flat, P, widths)):          # unpack(pack(x)) == x on the union
        assert np.array_equal(mine[rows].view(np.int32), theirs[rows].view(np.int32))
    print("%s: P %d, W %d, K %d, %d rows travel" % (name, P, W, K, len(rows)))

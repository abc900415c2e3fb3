"""The blend kernels' two-deep gather pipeline (csrc/gs_render_fwd_wave.hip, gs_render_bwd_wave.hip) at the list lengths
where it can go wrong, against the dense float64 model.

The kernels keep the records of batch i + 1 and the ids of batch i + 2 in flight under the blend loop of batch i, gather
from positions clamped into the list and run their last round without a gather.  What that can break depends on the
number of 64-entry batches of a tile and on where in them the tile stops, so the scenes here are the smallest with

  * per-tile list lengths 0, 1, 63, 64, 65, 127, 128, 129 and 193 (no batch, one partial / full batch, a second batch of one
    entry, ..., a fourth batch of one entry: prologue only, prologue + peeled round, one to three pipelined rounds), on a
    one-tile (16x16) and a two-tile (32x16) image, low opacities so that every batch is walked;
  * a 24x24 image whose four tiles are cut by the border, and a two-tile image whose tiles hold 1 and 129 entries (one wave
    leaves in the peeled round while its neighbour runs the pipeline);
  * a stop of the whole image at entry 64, 65 and 128 with 130 entries behind it: the batch gathered behind the stop is
    never staged, and the backward starts at a last contributor on a batch edge (entry 63, 64, 127).

Built with tests/blend_cases.py's Builder, so every scene is on its lattice; the margin condition (blend_cases.margins) is
asserted for each of them on the CPU (test_margin_condition, no GPU needed): no skip, stop or clamp decision lies within
1e-3 of its threshold, and the GPU tests exempt nothing.  Per case and instantiation (plain, 4-channel, FSGS; on the
reference's lists = the forward's CULL form, and on the culled region lists the benchmark runs): last contributors equal
the float64 model's, outputs within helpers.TOL, all gradients through helpers.check_grads, every forward output planted
with a NaN pattern first, and the forward bit-equal across two runs.
"""
import pytest
import torch

import blend_cases
import dense_reference
from helpers import TOL, check_grads, run_scene, settings_for

gpu = pytest.mark.gpu
CPU = torch.device("cpu")
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 193)
STOPS = (64, 65, 128)
SIZES = {"1tile": (16, 16), "2tile": (32, 16)}
MODES = {"reference": (False, "lsd"), "culled_region": (True, "region")}


def _len(W, H, n, name):
    """n wide low-opacity entries (blend_cases._len's rule): every tile holds them all, nothing saturates"""
    b = blend_cases.Builder(W, H)
    if n == 0:
        b.add(8, 8, 4.0, 0.5, visible=False)
    b.wide(max(blend_cases.FILL, min(0.3, 6.0 / max(n, 1))), n)
    return b.case(name, group="length", n=n, tile_len=[n] * (b.gx * b.gy))


def _stop(W, H, k, name):
    """every pixel saturates at entry k, 130 half-opaque entries with loud colours behind it"""
    b = blend_cases.Builder(W, H)
    b.stop_all_at(k)
    b.trailers()
    return b.case(name, group="stop", stop=k, tile_len=[k + 130] * (b.gx * b.gy))


def _one_and_129():
    """32x16: one wide entry on both tiles, then 128 narrow blobs (blend_cases._quad_only's half-pixel lattice; radius 4, so
    centres at x >= 21 keep their rectangles off tile 0) inside tile 1 only: list lengths 1 and 129"""
    b = blend_cases.Builder(32, 16)
    b.wide(0.02, 1)
    for i in range(128):
        b.add(16 + 5.0 + 0.5 * (i % 4), 3.0 + 0.5 * ((i // 4) % 4), blend_cases.VAR_BLOB, 0.05)
    return b.case("mixed_1_129", group="mixed", tile_len=[1, 129])


def _table():
    t = {}
    for tag, (W, H) in SIZES.items():
        for n in LENGTHS:
            t["len_%s_%d" % (tag, n)] = lambda W=W, H=H, n=n, tag=tag: _len(W, H, n, "len_%s_%d" % (tag, n))
        for k in STOPS:
            t["stop_%s_%d" % (tag, k)] = lambda W=W, H=H, k=k, tag=tag: _stop(W, H, k, "stop_%s_%d" % (tag, k))
    t["len_24x24_129"] = lambda: _len(24, 24, 129, "len_24x24_129")
    t["stop_24x24_65"] = lambda: _stop(24, 24, 65, "stop_24x24_65")
    t["mixed_1_129"] = _one_and_129
    return t


TABLE = _table()
NAMES = list(TABLE)
_CASES, _REF = {}, {}


def build(name):
    if name not in _CASES:
        _CASES[name] = TABLE[name]()
    return _CASES[name]


def cotangents(case):
    """colour [3], inverse depth / FSGS depth [1], 4th channel / FSGS alpha [1]"""
    g = torch.Generator().manual_seed(4000 + NAMES.index(case.name))
    H, W = case.H, case.W
    return torch.randn((3, H, W), generator=g), torch.randn((1, H, W), generator=g) * 0.3, torch.randn((1, H, W), generator=g)


def extra_values(case):
    return torch.rand((case.scene["means3D"].shape[0],), generator=torch.Generator().manual_seed(77))


def reference(name):
    """float64, once per case and shared by every test of it: the outputs (with `detail`), the 4th-channel image, and the
    gradients of the three instantiations' losses - plain: colour + inverse depth; extra: colour + 4th channel; fsgs:
    colour + depth + alpha"""
    if name not in _REF:
        case = build(name)
        P = case.scene["means3D"].shape[0]
        dc, dd, dx = (t.double() for t in cotangents(case))
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
        leaves["ndc_probe"] = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
        leaves["extra"] = extra_values(case).double().requires_grad_(True)
        d = dict(case.scene, **{k: v for k, v in leaves.items() if k != "extra"})
        a = dense_reference.render(d, case.cam, case.bg, False, detail=True)
        b = dense_reference.render(dict(d, colors_precomp=leaves["extra"][:, None].repeat(1, 3)), case.cam, case.bg, False)
        ximg = b["color"][0:1]
        losses = dict(plain=(a["color"] * dc).sum() + (a["invdepth"] * dd).sum(),
                      extra=(a["color"] * dc).sum() + (ximg * dx).sum(),
                      fsgs=(a["color"] * dc).sum() + (a["depth"] * dd).sum() + (a["alpha"] * dx).sum())
        names = list(leaves)
        grads = {}
        for which, loss in losses.items():
            g = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True, allow_unused=True)
            grads[which] = {k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in zip(names, g)}
        out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in a.items()}
        out["extra_img"] = ximg.detach()
        _REF[name] = (out, grads)
    return _REF[name]


def reference_grads(hg, dg):
    og = {k: dg[k] for k in hg if k in dg}
    og["means2D"] = torch.cat([dg["ndc_probe"], torch.zeros_like(dg["ndc_probe"][:, :1])], dim=1)
    return og


@pytest.mark.parametrize("name", NAMES)
def test_margin_condition(name):
    """on the CPU: the construction is the intended one (list lengths, stop entries, last contributors on the batch
    edges) and clears blend_cases' margin condition, so that nothing below is exempt from anything"""
    case = build(name)
    out, _ = reference(name)
    m = blend_cases.margins(out["detail"])
    print(name, {k: "%.3g" % v for k, v in m.items()})
    for k, v in m.items():
        assert v > 1.0, "%s: %s margin is %.3g of the required one" % (name, k, v)
    assert case.tile_len.tolist() == case.meta["tile_len"], (case.tile_len, case.meta["tile_len"])
    W, H = case.W, case.H
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    assert torch.equal(out["detail"]["tile_len"], torch.tensor(case.tile_len)[tile])
    n = out["n_contrib"]
    stopped = out["detail"]["tested"] & (out["detail"]["test_T"] < 1e-4)
    stop_at = (stopped.to(torch.int64) * torch.arange(1, stopped.shape[1] + 1)[None]).sum(1).reshape(H, W)
    if case.meta["group"] == "length":
        assert int(stop_at.max()) == 0 and int(n.min()) == int(n.max()) == case.meta["n"]
    elif case.meta["group"] == "stop":
        k = case.meta["stop"]
        for t in range(len(case.tile_len)):
            assert int(stop_at[tile == t].min()) > 0 and int(stop_at[tile == t].max()) == k
            assert int(n[tile == t].max()) == k - 1       # the backward's deepest last contributor: 63, 64, 127
    else:
        assert int(stop_at.max()) == 0 and int(n[tile == 0].max()) == 1 and int(n[tile == 1].max()) == 129


@pytest.fixture()
def blend(hip):
    """the backend in a known state, every forward output planted with a NaN pattern (test_gpu_blend_cases.py's rule)"""
    from test_gpu_blend_cases import plant
    names = ("tile_cull", "binning", "depth_limit_on", "_capacity_hint", "_capacity_hint_limited", "scratch_fill", "output_fill")
    old = {k: getattr(hip, k) for k in names}
    hip.depth_limit_on = False
    hip.output_fill = plant
    hip._cam_cache.clear()
    hip._region_off.clear()
    yield hip
    for k, v in old.items():
        setattr(hip, k, v)
    hip._cam_cache.clear()
    hip._region_off.clear()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_plain(blend, name, mode):
    from test_gpu_blend_cases import check_forward, planted_forward_state, written
    import diff_gaussian_rasterization as dgr
    case = build(name)
    blend.tile_cull, blend.binning = MODES[mode]
    tag = "prefetch_%s_%s" % (name, mode)
    dn, dg = reference(name)
    h = planted_forward_state(blend, case)
    assert h["num_rendered"] <= int(case.tile_len.sum())
    if mode == "reference":
        rng = h["ranges"].reshape(-1, 2).long()
        assert (rng[:, 1] - rng[:, 0]).tolist() == case.tile_len.tolist()
    check_forward(h, dn, case, tag)
    h2 = planted_forward_state(blend, case)
    for k in ("color", "invdepth", "final_T", "n_contrib"):
        assert torch.equal(_bits(h[k]), _bits(h2[k])), "%s: %s differs between two runs" % (tag, k)
    dc, di, _ = cotangents(case)
    r = run_scene(dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, case.scene, case.cam, torch.device("cuda"), bg=case.bg,
                  dL_dcolor=dc, dL_dinvdepth=di)
    written(r["color"], "color")
    written(r["invdepth"], "invdepth")
    assert torch.equal(_bits(r["color"]), _bits(h["color"])), "%s: the autograd path's image differs from the state path's" % tag
    hg = {k: v.cpu() for k, v in r["grads"].items()}
    assert float(hg["means2D"][:, 2].abs().max()) == 0.0
    check_grads(hg, reference_grads(hg, dg["plain"]), tag)


def _leaves(case, dev):
    p = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
    return p, torch.zeros_like(p["means3D"], requires_grad=True)


def _grads(p, m2, **more):
    hg = {k: (v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()) for k, v in p.items()}
    hg["means2D"] = m2.grad.cpu()
    hg.update({k: v.grad.cpu() for k, v in more.items()})
    return hg


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_four_channel(blend, name, mode):
    """HAS_EXTRA forward and backward (gsplat_amd.nir.GaussianRasterizerX)"""
    from gsplat_amd.nir import GaussianRasterizerX
    from test_gpu_blend_cases import written
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda")
    case = build(name)
    blend.tile_cull, blend.binning = MODES[mode]
    dn, dg = reference(name)
    dc, _, dx = cotangents(case)
    rs = settings_for(dgr.GaussianRasterizationSettings, case.cam, case.bg, 0, dev)
    runs = []
    for _ in range(2):
        p, m2 = _leaves(case, dev)
        xp = extra_values(case).to(dev).requires_grad_(True)
        rgb, radii, invd, ximg = GaussianRasterizerX(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], extra=xp,
                                                          colors_precomp=p["colors_precomp"], cov3D_precomp=p["cov3D_precomp"])
        for t, what in ((rgb, "color"), (invd, "invdepth"), (ximg, "extra"), (radii, "radii")):
            written(t, what)
        runs.append([_bits(t) for t in (rgb, invd, ximg)])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "%s/%s: the forward differs between two runs" % (name, mode)
    ((rgb * dc.to(dev)).sum() + (ximg * dx.to(dev)).sum()).backward()
    assert float((rgb.detach().cpu().double() - dn["color"]).abs().max()) <= TOL * max(1.0, float(dn["color"].abs().max()))
    assert float((invd.detach().cpu().double() - dn["invdepth"]).abs().max()) <= TOL * max(1.0, float(dn["invdepth"].abs().max()))
    assert float((ximg.detach().cpu().double() - dn["extra_img"]).abs().max()) <= TOL, "extra channel"
    hg = _grads(p, m2, extra=xp)
    check_grads(hg, reference_grads(hg, dg["extra"]), "prefetch_%s_%s_extra" % (name, mode))


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_fsgs(blend, name, mode):
    """the FSGS instantiations (dgr_fsgs): colour, depth = sum depth alpha T, alpha = sum alpha T and their gradients"""
    import dgr_fsgs
    from test_gpu_blend_cases import written
    dev = torch.device("cuda")
    case = build(name)
    blend.tile_cull, blend.binning = MODES[mode]
    W, H, P = case.W, case.H, case.scene["means3D"].shape[0]
    dn, dg = reference(name)
    dc, dd, da = cotangents(case)
    cam = case.cam
    rs = dgr_fsgs.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=case.bg.to(dev), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=0,
        campos=cam.camera_center.to(dev), prefiltered=False, debug=False, confidence=torch.ones((P, 1), device=dev))
    runs = []
    for _ in range(2):
        p, m2 = _leaves(case, dev)
        color, radii, depth, alpha = dgr_fsgs.GaussianRasterizer(rs)(
            means3D=p["means3D"], means2D=m2, opacities=p["opacities"], colors_precomp=p["colors_precomp"],
            cov3D_precomp=p["cov3D_precomp"])
        for t, what in ((color, "color"), (depth, "depth"), (alpha, "alpha"), (radii, "radii")):
            written(t, what)
        runs.append([_bits(t) for t in (color, depth, alpha)])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "%s/%s: the forward differs between two runs" % (name, mode)
    ((color * dc.to(dev)).sum() + (depth * dd.to(dev)).sum() + (alpha * da.to(dev)).sum()).backward()
    for k, v in (("color", color), ("depth", depth), ("alpha", alpha)):
        e = float((v.detach().cpu().double().reshape(dn[k].shape) - dn[k]).abs().max()) / max(1.0, float(dn[k].abs().max()))
        assert e <= TOL, "%s/%s: %s off by %.3e" % (name, mode, k, e)
    hg = _grads(p, m2)
    check_grads(hg, reference_grads(hg, dg["fsgs"]), "prefetch_%s_%s_fsgs" % (name, mode))

"""DNGaussian's fused neural heads on the GPU (csrc/gs_mlp.hip, gsplat_amd/neural.py, dng_neural) against the float64
restatement of tests/neural_reference.py: outputs and every gradient within 1e-4 of each tensor's largest entry (the
standing tolerance of this generation of kernels; tests/test_dng_neural_cpu.py shows the fp32 torch chain meets it with a
tenfold margin on the same inputs), exact-integer layout checks, the ReLU edge, saturation, the null combinations,
bitwise reproducibility, and GridRenderer end to end into dgr_dng."""

import pytest
import torch
import torch.nn.functional as F

import neural_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda")
TILE_ROWS, MAX_BLOCKS = 128, 256   # GS_DNG_HEADS_TILE_ROWS, GS_DNG_HEADS_MAX_BLOCKS (test_dng_neural_cpu.py holds them)
MULTI_PASS_B = TILE_ROWS * MAX_BLOCKS + 37  # 257 tiles: one more than the largest grid (its first workgroup takes two), ragged end
CAPS = (1, 3, 5)                            # max_blocks for CAPPED_B rows: every workgroup strides over 7 to 33 tiles
CAPPED_B = 32 * TILE_ROWS + 37              # 33 tiles, the last one ragged
PARITY_B = (1, 31, 32, 33, 63, 64, 65, 255, 4000, MULTI_PASS_B)
SIGMA_GRADS = ("g_enc_x", "g_w_s0", "g_w_s1", "g_w_s2")
ALL = ("sigma", "color", "g_enc_x", "g_enc_d") + tuple("g_" + n for n in ref.NAMES)


def hip_run(t, g_sigma=True, g_color=True, sigma_only=False, frozen=(), max_blocks=0):
    """The fused node forward + backward on the dict t (CPU tensors) -> dict like neural_reference.run (CPU tensors)."""
    from gsplat_amd import neural
    leaf = {k: t[k].detach().to(DEV).requires_grad_(k not in frozen) for k in ("enc_x", "enc_d") + ref.NAMES}
    if sigma_only:
        sigma, color = neural.dng_heads_sigma(leaf["enc_x"], leaf["w_s0"], leaf["w_s1"], leaf["w_s2"], max_blocks), None
    else:
        sigma, color = neural.dng_heads(leaf["enc_x"], leaf["enc_d"], *[leaf[n] for n in ref.NAMES], max_blocks=max_blocks)
    outs, grads = [], []
    if g_sigma:
        outs.append(sigma); grads.append(t["g_sigma"].to(DEV))
    if g_color:
        outs.append(color); grads.append(t["g_color"].to(DEV))
    torch.autograd.backward(outs, grads)
    res = {"sigma": sigma.detach().cpu(), "color": None if color is None else color.detach().cpu()}
    for k in ("enc_x", "enc_d") + ref.NAMES:
        res["g_" + k] = None if leaf[k].grad is None else leaf[k].grad.cpu()
    return res


_REF = {}


def reference(B):
    """The float64 restatement on make_inputs(B, seed=B): computed once, shared, never modified."""
    if B not in _REF:
        t = ref.make_inputs(B, seed=B)
        _REF[B] = (t, ref.run(ref.heads_ref, t, torch.float64))
    return _REF[B]


def assert_parity(h, o, names, what):
    for k in names:
        e = rel_err(h[k], o[k])
        print("%s: %s rel err %.2e" % (what, k, e))
        assert e < TOL, "%s: %s rel err %.2e" % (what, k, e)


@pytest.mark.parametrize("B", PARITY_B)
def test_heads_match_the_float64_restatement(B):
    t, o = reference(B)
    for k in ALL[2:]:
        assert float(o[k].abs().max()) > 0, k
    assert_parity(hip_run(t), o, ALL, "B=%d" % B)


@pytest.mark.parametrize("cap", CAPS)
def test_capped_grid_every_workgroup_takes_many_tiles(cap):
    """The persistent loops of all four kernels (forward and backward, colour and sigma-only form): with the grid capped at
    `cap` workgroups each one strides over 33 / cap tiles.  Parity as everywhere; per-row results do not depend on which
    workgroup computed them, so they are the uncapped run's bits; the weight gradients are the same bits run after run."""
    t, o = reference(CAPPED_B)
    h = hip_run(t, max_blocks=cap)
    assert_parity(h, o, ALL, "B=%d, %d workgroups" % (CAPPED_B, cap))
    again, free = hip_run(t, max_blocks=cap), hip_run(t)
    for k in ALL:
        assert torch.equal(h[k], again[k]), k
    for k in ("sigma", "color", "g_enc_x", "g_enc_d"):
        assert torch.equal(h[k], free[k]), k
    only = hip_run(t, g_color=False, sigma_only=True, max_blocks=cap)
    osig = ref.run(ref.heads_ref, t, torch.float64, g_color=False)
    assert torch.equal(only["sigma"], free["sigma"])
    assert_parity(only, osig, ("sigma",) + SIGMA_GRADS, "sigma only, %d workgroups" % cap)


def test_rows_that_are_not_16_byte_aligned():
    """Contiguous [B,32] / [B,16] views that start one float into an allocation: the kernels' element-wise loads and stores
    (every 16-byte access of a row needs an aligned base).  The same bits as the aligned run."""
    from gsplat_amd import neural
    B = 300
    t, o = reference(B)
    flat_x = torch.zeros(B * 32 + 1, device=DEV)
    flat_d = torch.zeros(B * 16 + 1, device=DEV)
    flat_x[1:] = t["enc_x"].to(DEV).reshape(-1)
    flat_d[1:] = t["enc_d"].to(DEV).reshape(-1)
    flat_x.requires_grad_(True)
    flat_d.requires_grad_(True)
    x, d = flat_x[1:].view(B, 32), flat_d[1:].view(B, 16)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 and d.data_ptr() % 16 == 4
    w = [t[n].to(DEV).requires_grad_(True) for n in ref.NAMES]
    sigma, color = neural.dng_heads(x, d, *w)
    torch.autograd.backward([sigma, color], [t["g_sigma"].to(DEV), t["g_color"].to(DEV)])
    got = {"sigma": sigma.detach().cpu(), "color": color.detach().cpu(), "g_enc_x": flat_x.grad[1:].view(B, 32).cpu(),
           "g_enc_d": flat_d.grad[1:].view(B, 16).cpu()}
    got.update({"g_" + n: p.grad.cpu() for n, p in zip(ref.NAMES, w)})
    assert_parity(got, o, ALL, "misaligned rows")
    aligned = hip_run(t)
    for k in ALL:
        assert torch.equal(got[k], aligned[k]), k
    s_only = neural.dng_heads_sigma(x, *w[:3])
    assert torch.equal(s_only.detach().cpu(), aligned["sigma"])


def integer_inputs(B, identity_s0):
    """Small integers for which every partial sum of the sigma path is an integer below 2^24, with ASYMMETRIC weights."""
    g = torch.Generator().manual_seed(B)
    t = {"enc_x": torch.randint(-1, 2, (B, 32), generator=g).float(), "enc_d": torch.randint(-1, 2, (B, 16), generator=g).float()}
    for n, (no, ni) in zip(ref.NAMES, ref.SHAPES):
        o, i = torch.meshgrid(torch.arange(no), torch.arange(ni), indexing="ij")
        t[n] = (((3 * o + 5 * i) % 7) - 3).float()
    if identity_s0:
        t["w_s0"] = torch.eye(64, 32)
    t["w_c0"] = t["w_c0"] / 65536  # (the colour path is not part of this check; keep its sigmoid away from saturation)
    t["g_sigma"] = torch.randint(-2, 3, (B,), generator=g).float()
    t["g_color"] = torch.zeros((B, 3))
    return t


@pytest.mark.parametrize("identity_s0", [False, True], ids=["asymmetric", "identity-s0"])
@pytest.mark.parametrize("B", [100, 300])
def test_exact_integer_layout(B, identity_s0):
    """A swapped row / column or a wrong k permutation changes these integers; nothing is rounded, so torch.equal."""
    t = integer_inputs(B, identity_s0)
    o = ref.run(ref.heads_ref, t, torch.float64, g_color=False)
    assert float(o["sigma"].abs().max()) < 2 ** 24 and float(o["g_w_s2"].abs().max()) < 2 ** 24
    for sigma_only in (False, True):
        h = hip_run(t, g_color=False, sigma_only=sigma_only)
        for k in ("sigma",) + SIGMA_GRADS:
            assert float(o[k].abs().max()) > 0, k
            assert torch.equal(h[k], o[k].float()), "%s (sigma_only=%s)" % (k, sigma_only)


def test_relu_edge_rows_of_zeros():
    """Rows of zeros have every pre-activation exactly 0: ReLU'(0) = 0 gives them zero input gradients, and they add nothing to
    a weight gradient.  B <= TILE_ROWS, so one workgroup sums all rows in row order and removing rows that add exact zeros
    leaves the same chain of roundings: the weight gradients with and without them are the same bits."""
    B = 100
    t = ref.make_inputs(B, seed=77)
    zero = torch.zeros(B, dtype=torch.bool)
    zero[[0, 3, 31, 32, 33, 50, 64, 65, 98, 99]] = True
    t["enc_x"][zero] = 0
    t["enc_d"][zero] = 0
    h = hip_run(t)
    assert torch.equal(h["g_enc_x"][zero], torch.zeros((int(zero.sum()), 32)))
    assert torch.equal(h["g_enc_d"][zero], torch.zeros((int(zero.sum()), 16)))
    assert_parity(h, ref.run(ref.heads_ref, t, torch.float64), ALL, "zero rows")
    keep = {k: (v[~zero] if v.shape[0] == B and k in ("enc_x", "enc_d", "g_sigma", "g_color") else v) for k, v in t.items()}
    hk = hip_run(keep)
    for n in ref.NAMES:
        assert float(h["g_" + n].abs().max()) > 0
        assert torch.equal(h["g_" + n], hk["g_" + n]), n
    assert torch.equal(h["g_enc_x"][~zero], hk["g_enc_x"]) and torch.equal(h["sigma"][~zero], hk["sigma"])


def test_saturated_colours():
    """w_c1 scaled so that the colour pre-activations reach beyond +-40 on both sides: the -0.001 / 1.001 ends."""
    B = 257
    t = dict(ref.make_inputs(B, seed=5))
    o = ref.run(ref.heads_ref, t, torch.float64)
    pre = torch.log((o["color"] + 0.001) / (1.001 - o["color"]))
    t["w_c1"] = t["w_c1"] * (45.0 / min(float(pre.max()), -float(pre.min())))
    o = ref.run(ref.heads_ref, t, torch.float64)
    assert float(o["color"].min()) < -0.001 + 1e-12 and float(o["color"].max()) > 1.001 - 1e-12  # pre-activations beyond +-40
    h = hip_run(t)
    assert_parity(h, o, ("sigma", "color"), "saturated")
    assert float(h["color"].min()) == pytest.approx(-0.001, abs=1e-7) and float(h["color"].max()) == pytest.approx(1.001, abs=1e-6)
    for k in ALL[2:]:
        assert bool(torch.isfinite(h[k]).all()), k
    assert_parity(h, o, ALL[2:], "saturated")


def test_null_combinations():
    B = 333
    t = ref.make_inputs(B, seed=B)
    o = ref.run(ref.heads_ref, t, torch.float64)
    # sigma-only node == full node with a zero colour gradient, bit for bit
    tz = dict(t, g_color=torch.zeros((B, 3)))
    full = hip_run(tz)
    only = hip_run(t, g_color=False, sigma_only=True)
    assert torch.equal(full["sigma"], only["sigma"])
    for k in SIGMA_GRADS:
        assert torch.equal(full[k], only[k]), k
    assert not bool(full["g_w_c0"].any()) and not bool(full["g_w_c1"].any()) and not bool(full["g_enc_d"].any())
    # the full node whose colour is never used: the same sigma-path gradients, zeros elsewhere
    unused = hip_run(t, g_color=False)
    for k in SIGMA_GRADS:
        assert torch.equal(unused[k], only[k]), k
    assert not bool(unused["g_w_c0"].any()) and not bool(unused["g_enc_d"].any())
    # g_sigma = None
    osig = ref.run(ref.heads_ref, t, torch.float64, g_sigma=False)
    assert_parity(hip_run(t, g_sigma=False), osig, ALL, "g_sigma=None")
    # frozen weights; frozen enc_d
    fw = hip_run(t, frozen=ref.NAMES)
    assert all(fw["g_" + n] is None for n in ref.NAMES)
    assert_parity(fw, o, ("sigma", "color", "g_enc_x", "g_enc_d"), "frozen weights")
    fd = hip_run(t, frozen=("enc_d",))
    assert fd["g_enc_d"] is None
    assert_parity(fd, o, [k for k in ALL if k != "g_enc_d"], "frozen enc_d")
    fx = hip_run(t, frozen=("enc_x", "enc_d"))
    assert fx["g_enc_x"] is None
    assert_parity(fx, o, ("sigma", "color") + tuple("g_" + n for n in ref.NAMES), "frozen inputs")


def test_non_contiguous_enc_x():
    from gsplat_amd import neural
    B = 200
    t = ref.make_inputs(B, seed=21)
    o = ref.run(ref.heads_ref, t, torch.float64)
    wide = torch.zeros((B, 40))
    wide[:, 3:35] = t["enc_x"]
    wide = wide.to(DEV).requires_grad_(True)
    w = [t[n].to(DEV).requires_grad_(True) for n in ref.NAMES]
    sigma, color = neural.dng_heads(wide[:, 3:35], t["enc_d"].to(DEV), *w)
    torch.autograd.backward([sigma, color], [t["g_sigma"].to(DEV), t["g_color"].to(DEV)])
    assert rel_err(sigma, o["sigma"]) < TOL and rel_err(color, o["color"]) < TOL
    assert rel_err(wide.grad[:, 3:35], o["g_enc_x"]) < TOL
    assert not bool(wide.grad[:, :3].any()) and not bool(wide.grad[:, 35:].any())
    assert rel_err(w[3].grad, o["g_w_c0"]) < TOL


def test_same_bits_twice_at_the_multi_pass_size():
    t, _ = reference(MULTI_PASS_B)
    a, b = hip_run(t), hip_run(t)
    for k in ALL:
        assert torch.equal(a[k], b[k]), k


def test_empty_batch():
    from gsplat_amd import neural
    t = ref.make_inputs(0, seed=1, device=DEV)
    w = [t[n].requires_grad_(True) for n in ref.NAMES]
    sigma, color = neural.dng_heads(t["enc_x"], t["enc_d"], *w)
    assert sigma.shape == (0,) and color.shape == (0, 3)
    (sigma.sum() + color.sum()).backward()
    for p in w:
        assert p.grad is not None and not bool(p.grad.any())


# ---- GridRenderer end to end ----
class _MLP(torch.nn.Module):
    """scene/neural_renderer.py MLP as tests/test_gpu_encoding.py restates it."""

    def __init__(self, dim_in, dim_out, dim_hidden, num_layers):
        super().__init__()
        self.net = torch.nn.ModuleList([torch.nn.Linear(dim_in if l == 0 else dim_hidden,
                                                        dim_out if l == num_layers - 1 else dim_hidden, bias=False)
                                        for l in range(num_layers)])

    def forward(self, x):
        for l, layer in enumerate(self.net):
            x = layer(x)
            if l != len(self.net) - 1:
                x = F.relu(x)
        return x


class _TorchRenderer(torch.nn.Module):
    """What a user of the encoders ran before the fused node: the HIP encoders with torch statements between them."""

    def __init__(self, bound, center):
        super().__init__()
        import gridencoder
        import shencoder
        self.register_buffer("bound", torch.as_tensor(bound, dtype=torch.float32))
        self.register_buffer("coord_center", torch.as_tensor(center, dtype=torch.float32))
        self.encoder_x = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16,
                                                 log2_hashmap_size=19, desired_resolution=512 * float(bound))
        self.sigma_net = _MLP(32, 65, 64, 3)
        self.color_net = _MLP(16 + 64, 3, 64, 2)
        self.sh = [shencoder.SHEncoder(degree=4)]  # (no parameters; kept out of the state_dict like encoder_dir's)

    def forward(self, x, d):
        h = self.sigma_net(self.encoder_x(x - self.coord_center, bound=self.bound))
        sigma, geo = h[:, 0], h[:, 1:]
        color = torch.sigmoid(self.color_net(torch.cat([self.sh[0](d), geo], dim=-1))) * (1 + 2 * 0.001) - 0.001
        return sigma, color


def test_grid_renderer_end_to_end():
    import dgr_dng
    import dng_neural
    from gsplat_amd import synthetic
    P, W, H = 4000, 256, 192
    sc = synthetic.trained_like(P, seed=3, sh_degree=0)
    cam = synthetic.orbit_cameras(W, H)[2]
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(5)).to(DEV)
    xyz0 = sc["means3D"].to(DEV)
    center = xyz0.mean(0)
    bound = float((xyz0.max(0).values - xyz0.min(0).values).max()) / 2 * 1.2
    torch.manual_seed(0)
    plain = _TorchRenderer(bound, center.cpu()).to(DEV)
    with torch.no_grad():
        plain.encoder_x.embeddings.uniform_(-0.1, 0.1)
    fused = dng_neural.GridRenderer(bound=bound, coord_center=center.cpu().tolist()).to(DEV)
    # a state_dict of the torch-statement model loads into GridRenderer, and back
    assert set(fused.state_dict()) == set(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    plain.load_state_dict(fused.state_dict())

    def chain(model):
        xyz = xyz0.clone().requires_grad_(True)
        model.zero_grad(set_to_none=True)
        d = xyz - cam.camera_center.to(DEV)
        d = d / d.norm(dim=1, keepdim=True)
        sigma, color = model(xyz, d)
        rs = dgr_dng.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=DEV),
            scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV),
            sh_degree=0, campos=cam.camera_center.to(DEV), prefiltered=False, debug=False)
        m2 = torch.zeros_like(xyz, requires_grad=True)
        img, radii, depth, alpha = dgr_dng.GaussianRasterizer(rs)(
            means3D=xyz, means2D=m2, opacities=torch.sigmoid(sigma)[:, None], colors_precomp=color,
            scales=sc["scales"].to(DEV), rotations=sc["rotations"].to(DEV))
        loss = (img - gt).abs().mean()
        loss.backward()
        out = {"xyz": xyz.grad, "embeddings": model.encoder_x.embeddings.grad.clone()}
        for name, net in (("sigma", model.sigma_net), ("color", model.color_net)):
            for i, layer in enumerate(net.net):
                out["%s%d" % (name, i)] = layer.weight.grad.clone()
        return float(loss), out

    lf, gf = chain(fused)
    lp, gp = chain(plain)
    assert abs(lf - lp) <= 1e-5 * max(1.0, abs(lp))
    assert len(gp) == 7
    for k in gp:
        assert float(gp[k].abs().max()) > 0, k
        e = rel_err(gf[k], gp[k])
        print("GridRenderer: %s rel err %.2e" % (k, e))
        assert e < 2e-4, "%s rel err %.2e" % (k, e)


def test_grid_renderer_density_color_and_keep_sigma():
    import dng_neural
    torch.manual_seed(1)
    r = dng_neural.GridRenderer(bound=1.5).to(DEV)
    with torch.no_grad():
        r.encoder_x.embeddings.uniform_(-0.1, 0.1)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand((777, 3), generator=g) * 2 - 1).to(DEV)
    d = F.normalize(torch.randn((777, 3), generator=g), dim=1).to(DEV)
    sigma, color = r(x, d)
    res = r.density(x)
    assert torch.equal(res["sigma"], sigma)               # the sigma-only form computes the same sigma
    assert torch.equal(r.color(res, d), color)            # ... and color() of that result is the fused node again
    # until geo_feat is read only 'sigma' has been computed; every other dict operation sees both entries
    lazy = r.density(x)
    assert not lazy.has_geo_feat() and lazy["sigma"] is lazy.get("sigma") and not lazy.has_geo_feat()
    assert len(lazy) == 2 and lazy.has_geo_feat() and list(lazy) == ["sigma", "geo_feat"]
    for view in (r.density(x).get("geo_feat"), dict(r.density(x))["geo_feat"], dict(r.density(x).items())["geo_feat"],
                 list(r.density(x).values())[1], r.density(x).copy()["geo_feat"]):
        assert view is not None and view.shape == (777, 64)
    assert "geo_feat" in r.density(x) and "other" not in r.density(x) and r.density(x).get("other", 5) == 5
    assert sorted(r.density(x).keys()) == ["geo_feat", "sigma"]
    enc = r.encode_x(x)
    h = r.sigma_net(enc)
    assert res["geo_feat"].shape == (777, 64) and rel_err(res["geo_feat"], h[:, 1:]) < 1e-6   # on request, through torch
    assert rel_err(sigma, h[:, 0]) < TOL
    assert rel_err(r.color(res, d), color) < TOL          # with geo_feat materialised: the reference's statements
    k = dng_neural.GridRenderer(bound=1.5, keep_sigma=True).to(DEV)
    k.load_state_dict(r.state_dict())
    s1, c1 = k(x, d)
    s2, c2 = k(x, d)
    assert s2 is s1 and k.density(x) is k.sigma_results_static   # cached: no launch for sigma on the second call
    assert torch.equal(s1, sigma) and torch.equal(c2, color)

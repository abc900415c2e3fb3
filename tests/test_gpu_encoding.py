"""DNGaussian's gridencoder / shencoder on the GPU (csrc/gs_encoding.hip) against the float64 torch oracle
(tests/encoding_reference.py): outputs, embedding and input gradients within 1e-4 of each tensor's largest entry,
the embedding gradient the same bits run after run, and DNGaussian's neural-renderer chain into dgr_dng."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import encoding_reference as ref
import gridencoder
import shencoder
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda")


def points(B, D, seed, edges=True, outside=True):
    """Uniform points in [0,1]^D, with exact 0 / 1 coordinates and points outside the cube mixed in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, D), generator=g)
    if edges and B >= 8:
        x[0::7, 0] = 0.0
        x[1::7, D - 1] = 1.0
        x[2] = 1.0
        x[3] = 0.0
    if outside and B >= 8:
        x[4::11, 0] = 1.0 + torch.rand((len(range(4, B, 11)),), generator=g) * 0.1
        x[5::13, D - 1] = -torch.rand((len(range(5, B, 13)),), generator=g) * 0.1
    return x


def run_grid(enc, x01, g_out):
    """HIP: forward + backward of the raw autograd function (inputs already in [0,1])."""
    xi = x01.to(DEV).requires_grad_(True)
    enc.embeddings.grad = None
    y = gridencoder.grid_encode(xi, enc.embeddings, enc.offsets, enc.per_level_scale, enc.base_resolution, True,
                                enc.gridtype_id, enc.align_corners, enc.interp_id)
    y.backward(g_out.to(DEV))
    return y.detach(), enc.embeddings.grad.detach().clone(), xi.grad.detach().clone()


def run_oracle(enc, x01, g_out, device=DEV):
    xi = x01.to(device).requires_grad_(True)
    emb = enc.embeddings.detach().to(device).double().requires_grad_(True)
    y = ref.grid_encode_ref(xi, emb, enc.offsets.tolist(), enc.per_level_scale, enc.base_resolution, enc.gridtype_id,
                            enc.align_corners, enc.interp_id)
    y.backward(g_out.to(device).double())
    return y.detach(), emb.grad.detach(), xi.grad.detach()


def assert_close(h, o, what):
    for name, a, b in zip(("outputs", "grad_embeddings", "grad_inputs"), h, o):
        e = rel_err(a, b)
        assert e < TOL, "%s: %s rel err %.2e" % (what, name, e)


CONFIGS = list(itertools.product((2, 3), (1, 2, 4, 8), ("hash", "tiled"), ("linear", "smoothstep"), (False, True)))


@pytest.mark.parametrize("D,C,gridtype,interp,align", CONFIGS,
                         ids=["D%dC%d-%s-%s-%s" % (D, C, g, i, "ac" if a else "noac") for D, C, g, i, a in CONFIGS])
def test_grid_matches_oracle(D, C, gridtype, interp, align):
    torch.manual_seed(D * 100 + C)
    enc = gridencoder.GridEncoder(input_dim=D, num_levels=6, level_dim=C, base_resolution=4, per_level_scale=1.7,
                                  log2_hashmap_size=9, gridtype=gridtype, align_corners=align, interpolation=interp).to(DEV)
    with torch.no_grad():
        enc.embeddings.normal_()
    x = points(3000, D, seed=D * 10 + C)
    g = torch.randn((3000, enc.output_dim), generator=torch.Generator().manual_seed(7))
    assert_close(run_grid(enc, x, g), run_oracle(enc, x, g), "D%d C%d %s %s ac%d" % (D, C, gridtype, interp, align))


@pytest.mark.parametrize("B", [1, 7, 1000, 100_000, 1_000_000])
def test_grid_dngaussian_configuration(B):
    """L=16, C=2, H=16, 2^19-slot tables, desired_resolution 512: every table size from one point to 1 M."""
    torch.manual_seed(B)
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                  desired_resolution=512).to(DEV)
    x = points(B, 3, seed=B) if B >= 8 else torch.rand((B, 3), generator=torch.Generator().manual_seed(B))
    g = torch.randn((B, 32), generator=torch.Generator().manual_seed(B + 1))
    h = run_grid(enc, x, g)
    o = run_oracle(enc, x, g)
    assert_close(h, o, "DNGaussian B=%d" % B)
    # every slot is written: the ones no point reached are exactly zero
    assert torch.equal(h[1][o[1] == 0], torch.zeros_like(h[1][o[1] == 0]))


def test_grid_module_forward_maps_bound_like_the_reference():
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=8, level_dim=2, log2_hashmap_size=12, desired_resolution=128).to(DEV)
    xyz = (torch.rand((500, 3), generator=torch.Generator().manual_seed(4)) * 7.0 - 3.5).to(DEV)
    y = enc(xyz.view(5, 100, 3), bound=4)
    assert y.shape == (5, 100, 16)
    o = ref.grid_encode_ref((xyz + 4) / 8, enc.embeddings.detach().double(), enc.offsets.tolist(), enc.per_level_scale, 16)
    assert rel_err(y.view(500, 16), o) < TOL
    # inputs without grad: no input gradient, embedding gradient only
    y.sum().backward()
    assert enc.embeddings.grad is not None


def test_grid_backward_is_bitwise_reproducible():
    """P = 200k at DNGaussian's configuration, half the points in one coarse cell (thousands of contributions per slot)."""
    P = 200_000
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                  desired_resolution=512).to(DEV)
    gen = torch.Generator().manual_seed(11)
    x = torch.rand((P, 3), generator=gen)
    x[: P // 2] = 0.5 + torch.rand((P // 2, 3), generator=gen) * (1.0 / 16)
    g = torch.randn((P, 32), generator=gen)
    a = run_grid(enc, x, g)
    b = run_grid(enc, x, g)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    o = run_oracle(enc, x, g)
    assert_close(a, o, "skewed P=200k")


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_matches_oracle(degree):
    g = torch.Generator().manual_seed(degree)
    v = torch.randn((4000, 3), generator=g)
    v[: 2000] = v[: 2000] / v[: 2000].norm(dim=1, keepdim=True)  # unit directions, and non-unit inputs after them
    v[-1] = 0.0
    gout = torch.randn((4000, degree * degree), generator=g)
    xi = v.to(DEV).requires_grad_(True)
    y = shencoder.sh_encode(xi, degree, True)
    y.backward(gout.to(DEV))
    xo = v.double().requires_grad_(True)
    yo = ref.sh_encode_ref(xo, degree)
    yo.backward(gout.double())
    assert rel_err(y.detach(), yo.detach()) < TOL
    assert rel_err(xi.grad, xo.grad) < TOL
    enc = shencoder.SHEncoder(degree=degree)
    y2 = enc(v.to(DEV).view(40, 100, 3) * 2.0, size=2.0)
    assert y2.shape == (40, 100, degree * degree) and rel_err(y2.reshape(4000, -1), yo.detach()) < TOL


class _MLP(torch.nn.Module):
    """scene/neural_renderer.py MLP: bias-free linear layers, ReLU between."""

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


def test_dngaussian_neural_chain_matches_the_oracle_encoders():
    """GridRenderer restated: hash encoder -> 3-layer sigma MLP; SH(dir) + geo_feat -> colour MLP; opacities and
    colors_precomp into dgr_dng, L1 loss, backward.  Gradients on xyz, the embeddings and the MLP weights match the
    same chain with the oracle encoders, within the tolerance of the FSGS / DNG generation (2e-4)."""
    import dgr_dng
    from gsplat_amd import synthetic
    P, W, H = 4000, 256, 192
    sc = synthetic.trained_like(P, seed=3, sh_degree=0)
    cam = synthetic.orbit_cameras(W, H)[2]
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(5)).to(DEV)
    xyz0 = sc["means3D"].to(DEV)
    center = xyz0.mean(0)
    bound = float((xyz0.max(0).values - xyz0.min(0).values).max()) / 2 * 1.2
    torch.manual_seed(0)
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                  desired_resolution=512 * bound).to(DEV)
    with torch.no_grad():
        enc.embeddings.uniform_(-0.1, 0.1)
    sigma_net = _MLP(32, 65, 64, 3).to(DEV)
    color_net = _MLP(16 + 64, 3, 64, 2).to(DEV)
    sh = shencoder.SHEncoder(degree=4)

    def chain(encode_x, encode_d):
        xyz = xyz0.clone().requires_grad_(True)
        emb = enc.embeddings.detach().clone().requires_grad_(True)
        for p in list(sigma_net.parameters()) + list(color_net.parameters()):
            p.grad = None
        h = sigma_net(encode_x(xyz - center, emb))
        sigma, geo = h[:, 0], h[:, 1:]
        d = xyz - cam.camera_center.to(DEV)
        d = d / d.norm(dim=1, keepdim=True)
        color = torch.sigmoid(color_net(torch.cat([encode_d(d), geo], dim=-1))) * (1 + 2 * 0.001) - 0.001
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
        out = {"xyz": xyz.grad, "embeddings": emb.grad}
        for name, net in (("sigma", sigma_net), ("color", color_net)):
            for i, layer in enumerate(net.net):
                out["%s%d" % (name, i)] = layer.weight.grad.clone()
        return float(loss), out

    def hip_x(x, emb):
        return gridencoder.grid_encode((x + bound) / (2 * bound), emb, enc.offsets, enc.per_level_scale, 16, True, 0,
                                       False, 0)

    def ref_x(x, emb):
        return ref.grid_encode_ref((x + bound) / (2 * bound), emb, enc.offsets.tolist(), enc.per_level_scale, 16).float()

    lh, gh = chain(hip_x, lambda d: sh(d))
    lo, go = chain(ref_x, lambda d: ref.sh_encode_ref(d, 4).float())
    assert abs(lh - lo) <= 1e-5 * max(1.0, abs(lo))
    for k in go:
        assert float(go[k].abs().max()) > 0, k
        assert rel_err(gh[k], go[k]) < 2e-4, "%s rel err %.2e" % (k, rel_err(gh[k], go[k]))

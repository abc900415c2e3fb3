"""DNGaussian's gridencoder / shencoder drop-ins without a GPU: package surface, DNGaussian's table geometry, the
reference's error messages, the float64 oracle (tests/encoding_reference.py) and the no-CPU-path rule."""
import math

import numpy as np
import pytest
import torch

import encoding_reference as ref


def dng_encoder(bound):
    """DNGaussian's GridRenderer.create_encoder (scene/neural_renderer.py) at a scene bound."""
    from gridencoder import GridEncoder
    return GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                       desired_resolution=512 * bound, gridtype='hash', align_corners=False)


def test_packages_import():
    import gridencoder
    import shencoder
    assert callable(gridencoder.GridEncoder) and callable(gridencoder.grid_encode)
    assert hasattr(gridencoder._grid_encode, "apply")
    assert callable(shencoder.SHEncoder) and callable(shencoder.sh_encode)


@pytest.mark.parametrize("bound,slots,hashed", [(1, 5291984, 9), (4, 6119864, 11)])
def test_dngaussian_grid_geometry(bound, slots, hashed):
    enc = dng_encoder(bound)
    offs = enc.offsets.tolist()
    pls = ref.per_level_scale_of(16, 16, desired_resolution=512 * bound)
    assert offs == ref.grid_offsets(3, 16, pls, 16, 19, False)
    assert offs[-1] == slots and enc.embeddings.shape == (slots, 2)
    assert enc.offsets.dtype == torch.int32
    assert int(enc.n_params) == 2 * slots
    assert enc.output_dim == 32 and enc.max_params == 2 ** 19
    assert sum(1 for a, b in zip(offs, offs[1:]) if b - a == 2 ** 19) == hashed
    assert float(enc.embeddings.detach().abs().max()) <= 1e-4
    assert repr(enc) == ("GridEncoder: input_dim=3 num_levels=16 level_dim=2 resolution=16 -> %d per_level_scale=%.4f "
                         "params=(%d, 2) gridtype=hash align_corners=False interpolation=linear" % (512 * bound, pls, slots))


def test_sh_encoder_surface():
    from shencoder import SHEncoder
    e = SHEncoder()
    assert e.output_dim == 16 and repr(e) == "SHEncoder: input_dim=3 degree=4"
    with pytest.raises(AssertionError, match="SH encoder only support input dim == 3"):
        SHEncoder(input_dim=2)
    for deg in (0, 9):
        with pytest.raises(AssertionError, match=r"SH encoder only supports degree in \[1, 8\]"):
            SHEncoder(degree=deg)


@pytest.mark.parametrize("D,C", [(3, 3), (3, 16), (6, 2), (1, 2)])
def test_grid_rejects_what_the_reference_rejects(D, C):
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=D, num_levels=2, level_dim=C, log2_hashmap_size=8)
    with pytest.raises(RuntimeError, match=r"GridEncoding: C must be 1, 2, 4, or 8\."):
        enc(torch.zeros((4, D)))


def test_grid_total_variation_is_a_named_divergence():
    with pytest.raises(NotImplementedError, match="grad_total_variation"):
        dng_encoder(1).grad_total_variation()


def test_cpu_inputs_raise():
    from gridencoder import GridEncoder
    from shencoder import SHEncoder
    with pytest.raises(RuntimeError, match="no CPU path"):
        GridEncoder(num_levels=4, log2_hashmap_size=10)(torch.rand((8, 3)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        SHEncoder()(torch.rand((8, 3)))


@pytest.mark.parametrize("gridtype,interp,align", [(0, 0, False), (1, 1, True), (0, 1, False)])
def test_grid_oracle_gradcheck(gridtype, interp, align):
    g = torch.Generator().manual_seed(3)
    D, L, C = 3, 3, 2
    pls, H = 1.5, 4
    offs = ref.grid_offsets(D, L, pls, H, 5, align)
    x = (torch.rand((6, D), generator=g) * 0.9 + 0.05).double().requires_grad_(True)
    emb = torch.randn((offs[-1], C), generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.grid_encode_ref(a, b, offs, pls, H, gridtype, align, interp,
                                                                     fp32_cells=False), (x, emb))


def test_grid_oracle_outside_points_are_zero():
    offs = ref.grid_offsets(2, 3, 2.0, 4, 8, False)
    emb = torch.randn((offs[-1], 2), dtype=torch.float64, requires_grad=True)
    x = torch.tensor([[0.5, 1.01], [-0.1, 0.3], [0.0, 1.0]], requires_grad=True)
    y = ref.grid_encode_ref(x, emb, offs, 2.0, 4)
    assert torch.equal(y[:2], torch.zeros_like(y[:2])) and bool((y[2] != 0).any())
    y[:2].sum().backward()
    assert float(emb.grad.abs().max()) == 0.0 and float(x.grad.abs().max()) == 0.0


def test_grid_oracle_dense_level_is_trilinear():
    """A dense level (no hash): the value at a grid vertex is that vertex's embedding."""
    offs = ref.grid_offsets(2, 1, 2.0, 4, 10, True)
    emb = torch.randn((offs[-1], 1), dtype=torch.float64)
    sc, res = ref.level_geometry(1, 2.0, 4)[0]
    assert sc == 3.0 and res == 4
    i, j = 2, 1
    x = torch.tensor([[i / 3.0, j / 3.0]], dtype=torch.float32)
    y = ref.grid_encode_ref(x, emb, offs, 2.0, 4, gridtype=1, align_corners=True)
    assert abs(float(y[0, 0]) - float(emb[i + j * 4, 0])) < 1e-6


def _legendre_sh(v, degree):
    """Associated-Legendre evaluation on unit vectors: (-1)^m sqrt(2) K P_l^m(cos t) {cos, sin}(m phi), scipy's lpmv
    carries the Condon-Shortley phase itself."""
    from scipy.special import lpmv
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    phi = np.arctan2(y, x)
    out = np.zeros((v.shape[0], degree * degree))
    for l in range(degree):
        for m in range(l + 1):
            K = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            P = lpmv(m, l, z)
            if m == 0:
                out[:, l * l + l] = K * P
            else:
                out[:, l * l + l + m] = math.sqrt(2) * K * P * np.cos(m * phi)
                out[:, l * l + l - m] = math.sqrt(2) * K * P * np.sin(m * phi)
    return out


def test_sh_oracle_matches_associated_legendre_on_unit_vectors():
    g = torch.Generator().manual_seed(5)
    v = torch.randn((500, 3), generator=g, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    got = ref.sh_encode_ref(v, 8).numpy()
    want = _legendre_sh(v.numpy(), 8)
    assert np.abs(got - want).max() < 1e-10
    # band 1 is (-C1 y, C1 z, -C1 x)
    c1 = math.sqrt(3 / (4 * math.pi))
    assert np.allclose(got[:, 1:4], torch.stack([-c1 * v[:, 1], c1 * v[:, 2], -c1 * v[:, 0]], 1).numpy())


def test_sh_oracle_gradcheck():
    v = torch.randn((3, 3), dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: ref.sh_encode_ref(a, 8), (v,))

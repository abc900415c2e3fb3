"""DNGaussian's neural heads without a GPU: the header's constants and the ABI table, dng_neural's modules (state_dict,
parameter groups, checkpoint recovery, encoders), the node's argument errors, and the margin of the GPU tests' tolerance:
on the GPU tests' own inputs the fp32 torch chain is within 1e-5 of the float64 restatement, a tenth of what the kernels
are held to."""
import os
import re

import pytest
import torch

import neural_reference as ref
from helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


def test_header_constants_equal_the_python_mirrors():
    from gsplat_amd import neural
    import test_gpu_dng_neural as gpu
    assert header_constant("GS_DNG_ENC_X") == neural.ENC_X == 32
    assert header_constant("GS_DNG_ENC_D") == neural.ENC_D == 16
    assert header_constant("GS_DNG_HIDDEN") == neural.HIDDEN == 64
    assert header_constant("GS_DNG_GEO") == neural.GEO == 64
    assert header_constant("GS_DNG_HEADS_TILE_ROWS") == neural.TILE_ROWS == gpu.TILE_ROWS
    assert header_constant("GS_DNG_HEADS_MAX_BLOCKS") == neural.MAX_BLOCKS == gpu.MAX_BLOCKS
    assert neural.WEIGHT_SHAPES == ref.SHAPES and neural.WEIGHT_NAMES == ref.NAMES
    assert sum(o * i for o, i in ref.SHAPES) == 15616
    assert gpu.MULTI_PASS_B == neural.TILE_ROWS * neural.MAX_BLOCKS + 37
    assert set(gpu.PARITY_B) >= {1, 31, 32, 33, 63, 64, 65, 255, 4000, gpu.MULTI_PASS_B}


def test_abi_table_has_the_three_entries_and_host_side_answers():
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    from gsplat_amd._lib import hip_api
    for n in ("dng_heads_tmp_bytes", "dng_heads_fwd", "dng_heads_bwd"):
        assert n in PROTOTYPES and n in DEVICE_ONLY
    api = hip_api()
    tmp = api.raw("dng_heads_tmp_bytes")
    assert tmp(0) == 0 and tmp(-1) == 0
    assert tmp(1) >= 15616 * 4 and tmp(128) == tmp(1) and tmp(129) >= 2 * 15616 * 4
    assert tmp(128 * 256) == tmp(10 ** 7) >= 256 * 15616 * 4       # the grid is capped: so is the scratch
    # argument errors are decided before anything touches a device
    assert api.raw("dng_heads_fwd")(None, None, -1, None, None, None, None, None, None, None, 0, None) == -2   # GS_E_SHAPE
    assert api.raw("dng_heads_fwd")(None, None, 5, None, None, None, None, None, None, None, 0, None) == -1    # GS_E_NULL
    assert api.raw("dng_heads_fwd")(None, None, 0, None, None, None, None, None, None, None, 0, None) == 0
    assert api.raw("dng_heads_fwd")(None, None, 5, None, None, None, None, None, None, None, -1, None) == -2  # max_blocks < 0
    nul = [None] * 14
    assert api.raw("dng_heads_bwd")(None, None, -1, *nul[:14], None, 0, 0, None) == -2
    assert api.raw("dng_heads_bwd")(None, None, 5, *nul[:14], None, 0, 0, None) == -1
    assert api.raw("dng_heads_bwd")(None, None, 5, *nul[:14], None, 0, -1, None) == -2


KEYS = {"bound": (), "coord_center": (3,), "encoder_x.offsets": (17,), "sigma_net.net.0.weight": (64, 32),
        "sigma_net.net.1.weight": (64, 64), "sigma_net.net.2.weight": (65, 64), "color_net.net.0.weight": (64, 80),
        "color_net.net.1.weight": (3, 64)}


def test_grid_renderer_state_dict_groups_and_attributes():
    import dng_neural
    assert set(dng_neural.__all__) == {"MLP", "GridRenderer", "get_encoder"}
    r = dng_neural.GridRenderer()
    sd = r.state_dict()
    assert set(sd) == set(KEYS) | {"encoder_x.embeddings"}
    for k, shape in KEYS.items():
        assert tuple(sd[k].shape) == shape, k
    assert sd["encoder_x.embeddings"].shape == (int(r.encoder_x.offsets[-1]), 2)
    assert (r.in_dim_x, r.in_dim_dir, r.hidden_dim, r.geo_feat_dim, r.num_layers, r.num_layers_color) == (32, 16, 64, 64, 3, 2)
    assert r.keep_sigma is False and r.sigma_results_static is None
    for name in ("forward", "density", "color", "encode_x", "create_encoder", "recover_from_ckpt", "get_params"):
        assert callable(getattr(r, name))
    groups = r.get_params(0.01, 0.001, wd=0.5)
    assert [g["name"] for g in groups] == ["neural_encoder", "neural_sigma", "neural_color"]
    assert "weight_decay" not in groups[0] and groups[1]["weight_decay"] == groups[2]["weight_decay"] == 0.5
    assert (groups[0]["lr"], groups[1]["lr"], groups[2]["lr"]) == (0.01, 0.001, 0.001)
    assert [tuple(p.shape) for p in groups[1]["params"]] == [(64, 32), (64, 64), (65, 64)]
    assert [tuple(p.shape) for p in groups[2]["params"]] == [(64, 80), (3, 64)]
    assert r.get_params(1, 1)[1]["weight_decay"] == 0
    opt = torch.optim.Adam(r.get_params(0.01, 0.001))  # the groups are what an optimizer takes
    assert len(opt.param_groups) == 3


def test_recover_from_ckpt_rebuilds_the_encoder_for_another_bound():
    import dng_neural
    src = dng_neural.GridRenderer(bound=2.5, coord_center=[1., 2., 3.])
    with torch.no_grad():
        src.encoder_x.embeddings.normal_()
    dst = dng_neural.GridRenderer()
    assert dst.encoder_x.per_level_scale != src.encoder_x.per_level_scale
    dst.recover_from_ckpt(src.state_dict())
    assert float(dst.bound) == 2.5 and dst.encoder_x.per_level_scale == src.encoder_x.per_level_scale
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k


def test_mlp_is_plain_torch_and_get_encoder_serves_the_references_names():
    import dng_neural
    import gridencoder
    import shencoder
    m = dng_neural.MLP(5, 2, 7, 3)
    assert [tuple(l.weight.shape) for l in m.net] == [(7, 5), (7, 7), (2, 7)] and all(l.bias is None for l in m.net)
    x = torch.randn((4, 5))
    want = torch.relu(torch.relu(x @ m.net[0].weight.t()) @ m.net[1].weight.t()) @ m.net[2].weight.t()
    assert torch.allclose(m(x.clone()), want)
    e, dim = dng_neural.get_encoder("hashgrid", desired_resolution=512, log2_hashmap_size=12)
    assert isinstance(e, gridencoder.GridEncoder) and e.gridtype == "hash" and dim == 32
    e, dim = dng_neural.get_encoder("tiledgrid", num_levels=4, log2_hashmap_size=10)
    assert e.gridtype == "tiled" and dim == 8
    e, dim = dng_neural.get_encoder("sphere_harmonics")
    assert isinstance(e, shencoder.SHEncoder) and dim == 16
    e, dim = dng_neural.get_encoder("None", input_dim=5)
    assert dim == 5 and e(x, bound=1) is x
    for name in ("frequency", "ash", "other"):
        with pytest.raises(NotImplementedError, match="Unknown encoding mode, choose from"):
            dng_neural.get_encoder(name)


def test_density_result_behaves_like_the_full_dict(monkeypatch):
    """'sigma' alone never evaluates geo_feat; every other dict operation sees both entries (the sigma kernel is replaced by
    the torch chain here: this is about the container)."""
    import dng_neural
    from gsplat_amd import neural
    monkeypatch.setattr(neural, "dng_heads_sigma", lambda x, a, b, c, max_blocks=0: ref.torch_chain(x, None, [a, b, c])[0])
    r = dng_neural.GridRenderer()
    enc = torch.randn((9, 32))

    def fresh():
        return r.density(None, enc_x=enc)

    res = fresh()
    assert res["sigma"].shape == (9,) and res.get("sigma") is res["sigma"] and not res.has_geo_feat()
    assert len(res) == 2 and res.has_geo_feat()
    want = r.sigma_net(enc)[:, 1:]
    for geo in (fresh()["geo_feat"], fresh().get("geo_feat"), dict(fresh())["geo_feat"], dict(fresh().items())["geo_feat"],
                list(fresh().values())[1], fresh().copy()["geo_feat"], {**fresh()}["geo_feat"]):
        assert torch.equal(geo, want)
    assert list(fresh()) == list(fresh().keys()) == ["sigma", "geo_feat"]
    assert "geo_feat" in fresh() and "other" not in fresh() and fresh().get("other", 5) == 5
    with pytest.raises(KeyError):
        fresh()["other"]


def test_node_argument_errors():
    from gsplat_amd import neural
    t = ref.make_inputs(8, seed=0)
    w = [t[n] for n in ref.NAMES]
    with pytest.raises(RuntimeError, match="no CPU path"):
        neural.dng_heads(t["enc_x"], t["enc_d"], *w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        neural.dng_heads_sigma(t["enc_x"], *w[:3])
    with pytest.raises(ValueError, match=r"enc_x must be \[B,32\]"):
        neural.dng_heads(t["enc_x"][:, :31], t["enc_d"], *w)
    with pytest.raises(ValueError, match="enc_d must be"):
        neural.dng_heads(t["enc_x"], t["enc_d"][:7], *w)
    with pytest.raises(ValueError, match=r"w_s2 must be \[65, 64\]"):
        neural.dng_heads(t["enc_x"], t["enc_d"], w[0], w[1], w[2][:64], w[3], w[4])
    # shapes before devices, devices before dtypes
    with pytest.raises(ValueError, match="w_c1 must be"):
        neural.dng_heads(t["enc_x"].double(), t["enc_d"], *w[:4], w[4].t())
    with pytest.raises(RuntimeError, match="no CPU path"):
        neural.dng_heads(t["enc_x"].double(), t["enc_d"], *w)
    if torch.cuda.is_available():
        dev = torch.device("cuda")
        with pytest.raises(RuntimeError, match="fp32 only"):
            neural.dng_heads(t["enc_x"].to(dev).double(), t["enc_d"].to(dev), *[x.to(dev) for x in w])
    import dng_neural
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_neural.GridRenderer().density(torch.zeros((4, 3)))


def test_fp32_torch_chain_is_ten_times_inside_the_gpu_tolerance():
    """Reference-alone margin: arithmetic of the kernels' own width meets a tenth of the GPU tests' 1e-4 on their inputs, so a
    GPU failure is the kernel's."""
    import test_gpu_dng_neural as gpu
    assert gpu.TOL == 1e-4
    worst = 0.0
    for B in gpu.PARITY_B:
        t, o = gpu.reference(B)
        f = ref.run(ref.torch_chain, t, torch.float32)
        for k in gpu.ALL:
            e = rel_err(f[k], o[k])
            worst = max(worst, e)
            assert e < 1e-5, "B=%d %s: fp32 chain rel err %.2e" % (B, k, e)
    print("fp32 torch chain vs float64 restatement: worst rel err %.2e" % worst)

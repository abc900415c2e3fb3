"""DNGaussian's neural renderer on the MI355X kernels: MLP, GridRenderer and get_encoder under the names DNGaussian's
scene/gaussian_model.py and scene/neural_renderer.py use.  Change `from scene.neural_renderer import GridRenderer` to
`from dng_neural import GridRenderer`; a DNGaussian checkpoint's neural_renderer_state loads unchanged, because the module
tree (encoder_x, sigma_net.net.N, color_net.net.N) and the two buffers (bound, coord_center) carry DNGaussian's names.

Written from that interface, not from DNGaussian's module: the computation is this project's.  GridRenderer.forward is three
launches - hash grid, SH (csrc/gs_encoding.hip) and ONE fused MFMA kernel for both MLPs (csrc/gs_mlp.hip through
gsplat_amd/neural.py).  density() returns a dict whose 'sigma' comes from the sigma-only form of that kernel; 'geo_feat' is
evaluated through the torch MLP the first time anything but 'sigma' is asked of the dict, since the fused kernels never write
it to memory.  color(sigma_result, d) of a result whose geo_feat was never read is the fused node again.

fp32 and CUDA(HIP) tensors only for forward / density / color (MLP itself is plain torch and runs anywhere); the
'frequency' and 'ash' encoders have no counterpart here."""
import torch
from torch import nn

from gsplat_amd import neural as _n

__all__ = ["MLP", "GridRenderer", "get_encoder"]

_COLOR_SCALE, _COLOR_SHIFT = 1.002, 0.001  # colour = sigmoid(.) * 1.002 - 0.001: the ends reach slightly past [0, 1]


def _grid(gridtype):
    def make(input_dim, degree, grid):
        from gridencoder import GridEncoder
        return GridEncoder(input_dim=input_dim, gridtype=gridtype, **grid)
    return make


def _sh(input_dim, degree, grid):
    from shencoder import SHEncoder
    return SHEncoder(input_dim=input_dim, degree=degree)


_ENCODERS = {"hashgrid": _grid("hash"), "tiledgrid": _grid("tiled"), "sphere_harmonics": _sh}


def get_encoder(encoding, input_dim=3, multires=6, degree=4, num_levels=16, level_dim=2, base_resolution=16,
                log2_hashmap_size=19, desired_resolution=2048, align_corners=False, **kwargs):
    """-> (encoder, output width).  'None' is the identity; 'hashgrid' / 'tiledgrid' / 'sphere_harmonics' are the HIP
    encoders; anything else ('frequency' and 'ash' too) raises NotImplementedError with DNGaussian's message."""
    if encoding == "None":
        return (lambda x, **_: x), input_dim
    make = _ENCODERS.get(encoding)
    if make is None:
        raise NotImplementedError("Unknown encoding mode, choose from [None, frequency, sphere_harmonics, hashgrid, tiledgrid]")
    grid = dict(num_levels=num_levels, level_dim=level_dim, base_resolution=base_resolution,
                log2_hashmap_size=log2_hashmap_size, desired_resolution=desired_resolution, align_corners=align_corners)
    enc = make(input_dim, degree, grid)
    return enc, enc.output_dim


class MLP(nn.Module):
    """num_layers bias-free Linear layers (self.net) with ReLU after all but the last.  It owns the parameters the fused
    kernels read, and evaluates any shape through torch."""

    def __init__(self, dim_in, dim_out, dim_hidden, num_layers):
        super().__init__()
        self.dim_in, self.dim_out, self.dim_hidden, self.num_layers = dim_in, dim_out, dim_hidden, num_layers
        widths = [dim_in] + [dim_hidden] * (num_layers - 1) + [dim_out]
        self.net = nn.ModuleList(nn.Linear(a, b, bias=False) for a, b in zip(widths[:-1], widths[1:]))

    def forward(self, x):
        for layer in self.net[:-1]:
            x = torch.relu(layer(x))
        return self.net[-1](x)

    def weights(self):
        return [layer.weight for layer in self.net]


class _SigmaResult(dict):
    """density()'s {'sigma', 'geo_feat'}.  'sigma' is there from the start; 'geo_feat' is computed by the torch MLP the first
    time the dict is asked for anything else - a key test, a length, an iteration, a copy - so that every dict operation sees
    both entries, while `result['sigma']` alone (get_opacity) never evaluates it."""

    def __init__(self, sigma_net, enc_x):
        super().__init__()
        self.enc_x = enc_x
        self._sigma_net = sigma_net
        sigma = _n.dng_heads_sigma(enc_x.reshape(-1, enc_x.shape[-1]), *sigma_net.weights())
        super().__setitem__("sigma", sigma.view(enc_x.shape[:-1]))

    def has_geo_feat(self):
        return super().__contains__("geo_feat")

    def _fill(self):
        if not self.has_geo_feat():
            super().__setitem__("geo_feat", self._sigma_net(self.enc_x)[..., 1:])
        return self

    def __getitem__(self, key):
        if key != "sigma":
            self._fill()
        return super().__getitem__(key)

    def get(self, key, default=None):
        if key != "sigma":
            self._fill()
        return super().get(key, default)

    def __contains__(self, key):
        return self._fill() is self and super().__contains__(key)

    def __iter__(self):
        return super(_SigmaResult, self._fill()).__iter__()

    def __len__(self):
        return super(_SigmaResult, self._fill()).__len__()

    def keys(self):
        return super(_SigmaResult, self._fill()).keys()

    def values(self):
        return super(_SigmaResult, self._fill()).values()

    def items(self):
        return super(_SigmaResult, self._fill()).items()

    def copy(self):
        return dict(self.items())

    def __eq__(self, other):
        return dict(self.items()) == other

    __hash__ = None

    def __repr__(self):
        return repr(dict(self.items()))


class GridRenderer(nn.Module):
    """Per-Gaussian opacity logit and view-dependent colour from a hash-grid encoding of the position and an SH encoding of the
    view direction.  forward(x [N,3] in [-bound, bound], d [N,3] unit) -> (sigma [N], color [N,3])."""

    # DNGaussian's fixed configuration (csrc/gs_mlp.hip is compiled for these widths)
    num_levels, level_dim, base_resolution, table_size, desired_resolution = 16, 2, 16, 19, 512
    num_layers, hidden_dim, geo_feat_dim = 3, 64, 64
    num_layers_color, hidden_dim_color = 2, 64

    def __init__(self, bound=1., coord_center=[0., 0., 0.], keep_sigma=False):
        super().__init__()
        for name, value in (("bound", bound), ("coord_center", coord_center)):
            self.register_buffer(name, torch.as_tensor(value, dtype=torch.float32).detach())
        self.keep_sigma = keep_sigma
        self.sigma_results_static = None  # with keep_sigma: the first density() result, returned from then on
        self.create_encoder()
        self.encoder_dir, self.in_dim_dir = get_encoder("sphere_harmonics")
        self.sigma_net = MLP(self.in_dim_x, 1 + self.geo_feat_dim, self.hidden_dim, self.num_layers)
        self.color_net = MLP(self.in_dim_dir + self.geo_feat_dim, 3, self.hidden_dim_color, self.num_layers_color)

    def create_encoder(self):
        """(Re)build the hash grid for the current bound: its finest level resolves desired_resolution cells per unit."""
        finest = self.desired_resolution * float(self.bound)
        self.encoder_x, self.in_dim_x = get_encoder("hashgrid", input_dim=3, num_levels=self.num_levels, level_dim=self.level_dim,
                                                    base_resolution=self.base_resolution, log2_hashmap_size=self.table_size,
                                                    desired_resolution=finest)
        return self.encoder_x, self.in_dim_x

    def recover_from_ckpt(self, state_dict):
        """Load a state_dict saved under another bound: the grid's geometry follows the bound, so it is rebuilt first."""
        self.bound = state_dict["bound"]
        self.create_encoder()
        self.load_state_dict(state_dict)

    def encode_x(self, x):
        return self.encoder_x(x - self.coord_center, bound=self.bound)

    def _fused(self, enc_x, d):
        enc_d = self.encoder_dir(d)
        lead = tuple(enc_x.shape[:-1])
        sigma, color = _n.dng_heads(enc_x.reshape(-1, self.in_dim_x), enc_d.reshape(-1, self.in_dim_dir),
                                    *self.sigma_net.weights(), *self.color_net.weights())
        return sigma.view(lead), color.view(lead + (3,))

    def forward(self, x, d):
        if self.keep_sigma:  # sigma is frozen after the first call: go through the cached density() result
            result = self.density(x)
            return result["sigma"], self.color(result, d)
        return self._fused(self.encode_x(x), d)

    def density(self, x, enc_x=None):
        """-> {'sigma': [N], 'geo_feat': [N,64]} (geo_feat evaluated on demand, see _SigmaResult)."""
        if self.keep_sigma and self.sigma_results_static is not None:
            return self.sigma_results_static
        result = _SigmaResult(self.sigma_net, self.encode_x(x) if enc_x is None else enc_x)
        if self.keep_sigma:
            self.sigma_results_static = result
        return result

    def color(self, sigma_result, d):
        """Colour [N,3] of a density() result seen from d."""
        if isinstance(sigma_result, _SigmaResult) and not sigma_result.has_geo_feat():
            return self._fused(sigma_result.enc_x, d)[1]
        # any other mapping with a geo_feat (or a result whose geo_feat a caller has read): the colour net through torch
        features = torch.cat([self.encoder_dir(d), sigma_result["geo_feat"]], dim=-1)
        return torch.sigmoid(self.color_net(features)) * _COLOR_SCALE - _COLOR_SHIFT

    def get_params(self, lr, lr_net, wd=0):
        """Optimizer groups under DNGaussian's names: the grid at lr, the two nets at lr_net with weight decay wd."""
        groups = [{"params": self.encoder_x.parameters(), "name": "neural_encoder", "lr": lr}]
        for name, net in (("neural_sigma", self.sigma_net), ("neural_color", self.color_net)):
            groups.append({"params": net.parameters(), "name": name, "lr": lr_net, "weight_decay": wd})
        return groups

"""FSGS's depth-correlation term and proximity unpooling restated in plain torch - the yardstick of tests/test_fsgs_loss_cpu.py
and tests/test_gpu_fsgs_loss.py.  Dtype-generic: the same functions run in float32 and float64.

  pearson(x, y)                      r = Sxy / sqrt(Sxx Syy) clamped to [-1, 1], two-pass centred sums (what
                                     torchmetrics.functional.pearson_corrcoef returns for one output)
  form(t, name)                      "ID": t, "NEG": -t, "RECIP200": 1 / (t + 200)
  depth_pearson_loss(depth, midas)   FSGS/train.py:105-108 with Python's min on the two scalars
  pseudo_depth_pearson_loss          FSGS/train.py:127
  pearson_grad(x, y)                 the closed form the backward kernel evaluates
  scene(H, W, kind, seed)            inputs of the kinds the term meets
  proximity(...)                     FSGS/scene/gaussian_model.py:405-420 on plain tensors"""
import torch

FORMS = ("ID", "NEG", "RECIP200")


def form(t, name):
    if name == "ID":
        return t
    if name == "NEG":
        return -t
    if name == "RECIP200":
        return 1 / (t + 200.)
    raise ValueError(name)


def sums(x, y):
    x, y = x.reshape(-1), y.reshape(-1)
    xc, yc = x - x.mean(), y - y.mean()
    return xc, yc, (xc * xc).sum(), (yc * yc).sum(), (xc * yc).sum()


def pearson(x, y, clamp=True):
    _, _, sxx, syy, sxy = sums(x, y)
    r = sxy / torch.sqrt(sxx * syy)
    # (a clamp written with where: torch.clamp would zero the gradient outside [-1, 1], and the clamp does not gate it)
    if clamp:
        r = r + (torch.clamp(r.detach(), -1.0, 1.0) - r.detach())
    return r


def pearson_grad(x, y):
    """(dr/dx, dr/dy) in closed form: dr/dx_i = (y_i - mean y) / sqrt(Sxx Syy) - r (x_i - mean x) / Sxx, and symmetrically."""
    xc, yc, sxx, syy, sxy = sums(x, y)
    d = torch.sqrt(sxx * syy)
    r = sxy / d
    return (yc / d - r * xc / sxx).reshape(x.shape), (xc / d - r * yc / syy).reshape(y.shape)


def py_min(a, b):
    """Python's min(a, b) on two scalars: b only if b < a (a tie or a NaN keeps a) -> (value, branch)."""
    return (b, 1) if bool(b < a) else (a, 0)


def depth_pearson_loss(depth, midas, return_branch=False):
    a = 1 - pearson(form(midas, "NEG"), depth)
    b = 1 - pearson(form(midas, "RECIP200"), depth)
    loss, branch = py_min(a, b)
    return (loss, branch) if return_branch else loss


def pseudo_depth_pearson_loss(depth, midas):
    return 1 - pearson(depth, form(midas, "NEG"))


def scene(H, W, kind, seed, dtype=torch.float64):
    """(x = a rendered depth, m = a MiDaS-like target), [H, W] each, drawn in float64 and passed through float32 so that the
    fp32 and fp64 runs start from the same numbers.
      "A"        z = 2 + 6 U, m = 1000 - 100 z + 40 N(0,1): affine in z - the NEG form wins
      "B"        m = 3000 / z - 200 + 30 N(0,1): a disparity - the RECIP200 form wins
      "offset"   x = 1000 + 0.01 N(0,1), m affine in x plus noise: where raw fp32 moments cancel to nothing
      "exact+" / "exact-"   m affine in z, no noise, falling / rising: r(z, -m) = +1 / -1
      "constant" constant x"""
    g = torch.Generator().manual_seed(seed)
    n = H * W
    z = 2.0 + 6.0 * torch.rand((n,), generator=g, dtype=torch.float64)
    noise = torch.randn((n,), generator=g, dtype=torch.float64)
    if kind == "A":
        x, m = z, 1000.0 - 100.0 * z + 40.0 * noise
    elif kind == "B":
        x, m = z, 3000.0 / z - 200.0 + 30.0 * noise
    elif kind == "offset":
        x = 1000.0 + 0.01 * torch.randn((n,), generator=g, dtype=torch.float64)
        m = 500.0 - 2000.0 * (x - 1000.0) + 10.0 * noise
    elif kind == "exact+":
        x, m = z, 1000.0 - 100.0 * z
    elif kind == "exact-":
        x, m = z, 100.0 + 100.0 * z
    elif kind == "constant":
        x, m = torch.full((n,), 3.25, dtype=torch.float64), 1000.0 - 100.0 * z
    else:
        raise ValueError(kind)
    return x.float().to(dtype).reshape(H, W), m.float().to(dtype).reshape(H, W)


def proximity(xyz, scaling_raw, opacity_raw, rotation, features, dist, nearest, extent, N=3):
    """The reference's unpooling step (FSGS/scene/gaussian_model.py:405-420) restated on plain tensors, operation for
    operation; features = [P,16,3] (its f_dc and f_rest together).  -> (dict of the NEW rows, the selection mask).
    Note the sources: the reference writes _xyz[mask].repeat(1, N, 1).reshape(-1, 3), which lays the S selected rows out N
    times one after the other (s0 .. sS-1, s0 .. sS-1, ...), while the neighbour lists run s0k0, s0k1, s0k2, s1k0, ...: new row
    j pairs selected row j % S with neighbour entry j."""
    sel = torch.logical_and(dist > (5. * extent), torch.max(torch.exp(scaling_raw), dim=1).values > (extent))
    idx = nearest[sel].reshape(-1).long()
    S = int(sel.sum())
    tiled = xyz[sel].repeat(1, N, 1).reshape(-1, 3)
    assert torch.equal(tiled, xyz[sel][torch.arange(S * N) % max(S, 1)])  # what that expression does, spelled out
    rot = torch.zeros_like(rotation[idx])
    rot[:, 0] = 1
    return dict(xyz=(tiled + xyz[idx]) / 2, scaling=scaling_raw[idx], rotation=rot, features=torch.zeros_like(features[idx]),
                opacity=opacity_raw[idx]), sel

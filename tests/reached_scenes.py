"""Constructed scenes for the reached split (tests/test_gpu_reached_split.py) and the list arithmetic that says, from a
forward's exported lists, which Gaussians the backward blend can reach.  Host-side torch only.

wall   two opaque spherical shells around a ball: from the orbit cameras the shells cover the whole image and saturate every
       pixel, so every Gaussian of the ball (and of the shells' far side) is accepted by tiles, listed, and never reached.
       Rows: the shells' Gaussians first, in random order, then the ball's - the last blocks of 256 rows hold nothing else.
haze   trained_like with opacities of a few percent: no pixel saturates, every list is walked to its end.
"""
import numpy as np
import torch

from gsplat_amd import synthetic

W, H = 256, 160
P = 2503              # not a multiple of 4 or of 256
N_SHELL = 1500        # rows [0, N_SHELL): the two opaque shells; rows [N_SHELL, P): the ball behind them


def _sh(n, g):
    sh = torch.zeros((n, 16, 3), dtype=torch.float32)
    sh[:, 0, :] = torch.randn((n, 3), generator=g)
    sh[:, 1:, :] = 0.15 * torch.randn((n, 15, 3), generator=g)
    return sh


def wall(seed=0):
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    n_back = P - N_SHELL
    d = rng.standard_normal((N_SHELL, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.where(rng.random_sample(N_SHELL) < 0.5, 1.8, 1.7)   # (both shells in every block of rows)
    front = torch.from_numpy((d * r[:, None]).astype(np.float32))
    b = rng.standard_normal((n_back, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    back = torch.from_numpy((b * (0.9 * rng.random_sample(n_back) ** (1.0 / 3.0))[:, None]).astype(np.float32))
    scales = torch.cat([torch.full((N_SHELL, 3), 0.22), 0.08 * torch.exp(0.3 * torch.randn((n_back, 3), generator=g))])
    q = torch.randn((P, 4), generator=g)
    opac = torch.cat([torch.full((N_SHELL, 1), 0.9), 0.5 + 0.4 * torch.rand((n_back, 1), generator=g)])
    return dict(means3D=torch.cat([front, back]), scales=scales.float(), rotations=(q / q.norm(dim=1, keepdim=True)).float(),
                opacities=opac.float(), shs=_sh(P, g), sh_degree=3)


def haze(seed=1):
    sc = synthetic.trained_like(P, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    sc["opacities"] = (0.02 + 0.02 * torch.rand((P, 1), generator=g)).float()
    return sc


def cameras():
    return synthetic.orbit_cameras(W, H)[:3]


def list_sets(st, n_gauss, width=W, height=H):
    """From a forward's exported state (ranges [T, 2], point_list [R], n_contrib [H, W]; host tensors) ->
    (must, may, listed), bool [P] each.  A pixel's n_contrib is the 1-based list position of its last contributor and the
    backward blend of a tile visits the 0-based positions below the tile's largest n_contrib (`bound`).
      must    Gaussians with an entry at a position < bound in some tile: the ones the backward blend adds sums to
      may     ... at a position <= bound: `must` and the one entry per tile at which its last pixel saturated
      listed  Gaussians with any list entry"""
    ranges, pl, nc = st["ranges"].long(), st["point_list"].long(), st["n_contrib"].long()
    gx, gy = (width + 15) // 16, (height + 15) // 16
    must = torch.zeros((n_gauss,), dtype=torch.bool)
    may = torch.zeros((n_gauss,), dtype=torch.bool)
    listed = torch.zeros((n_gauss,), dtype=torch.bool)
    for t in range(gx * gy):
        lo, hi = int(ranges[t, 0]), int(ranges[t, 1])
        tx, ty = t % gx, t // gx
        bound = int(nc[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16].max())
        assert bound <= hi - lo
        listed[pl[lo:hi]] = True
        must[pl[lo:lo + bound]] = True
        may[pl[lo:min(lo + bound + 1, hi)]] = True
    return must, may, listed

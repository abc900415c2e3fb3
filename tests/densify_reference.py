"""A pure-torch restatement of the device form of densify / split / prune (csrc/gs_densify.hip), and the inputs its tests share.

The device form takes every discrete decision PER SOURCE ROW (one flag byte) from five fp32 thresholds and then places the
rows in the reference order [survivors | clones | sample block 0 | ... | sample block N-1].  `plan_flags` and
`destination_table` restate that; `apply_table` builds the model they describe.  tests/test_densify_device_cpu.py holds the
result to GaussianModelLite.densify_and_prune's host path (the arbiter), which proves the two facts the plan rests on: a
clone's prune decision is its source survivor's, and the N samples of a split row share one decision.

`build_model` makes the inputs of both the CPU and the GPU tests from CPU generators only, so that the CPU test can assert
the margin condition - every row decisive by more than 1e-5 relative, about 100 fp32 ulps - on exactly what the GPU sees.
"""
import functools

import numpy as np
import torch

from gsplat_amd import synthetic
from gsplat_amd.trainer import GaussianModelLite

CLONE, SPLIT, PRUNE_SELF, PRUNE_SAMPLE = 1, 2, 4, 8
SURVIVOR, CLONED, SAMPLE = 0, 1, 2
EXTENT, MAX_GRAD, MIN_OPACITY = 4.4, 2e-4, 0.005
SIZES, SEEDS, NS, SCREENS = (1, 70, 257, 1031), (7, 5, 3), (2, 3), (None, 20)
EMPTY_BLOCK = 2   # with four blocks or more: no selected row in this one
# rows with constructed statistics (models of 70 rows or more)
ROW_INF, ROW_NAN, ROW_NEG_SMALL, ROW_NEG_LARGE, ROW_EXACT, ROW_BELOW = 11, 12, 13, 14, 16, 17


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def thresholds(max_grad, min_opacity, extent, percent_dense, N):
    """The five fp32 values torch compares fp32 tensors with: products formed in double (Python), rounded to fp32 once."""
    return dict(max_grad=f32(max_grad), scale_bound=f32(percent_dense * extent), min_opacity=f32(min_opacity),
                world_bound=f32(0.1 * extent), sample_div=f32(0.8 * N))


def plan_flags(scaling, opacity, accum, denom, thr, size_test):
    """One flag byte per source row (include/gsplat.h: GS_DENSIFY_*), every comparison fp32 against fp32."""
    g = accum.reshape(-1) / denom.reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    e = torch.exp(scaling)
    max_scale = e.max(dim=1).values
    small = max_scale <= thr["scale_bound"]
    faint = torch.sigmoid(opacity.reshape(-1)) < thr["min_opacity"]
    max_sample = torch.exp(torch.log(e / thr["sample_div"])).max(dim=1).values
    clone = (g.abs() >= thr["max_grad"]) & small
    split = (g >= thr["max_grad"]) & ~small
    prune_self, prune_sample = faint.clone(), faint.clone()
    if size_test:
        prune_self |= max_scale > thr["world_bound"]
        prune_sample |= max_sample > thr["world_bound"]
    return (clone.to(torch.uint8) * CLONE + split.to(torch.uint8) * SPLIT + prune_self.to(torch.uint8) * PRUNE_SELF +
            prune_sample.to(torch.uint8) * PRUNE_SAMPLE)


def destination_table(flags, N):
    """(src [P2], kind [P2], noise_row [P2] (-1: none), counts): the output rows in reference order, each group by ascending
    source row.  counts = the five totals of gs_densify_plan."""
    f = flags.to(torch.int64)
    split = (f & SPLIT) != 0
    kept = ~split & ((f & PRUNE_SELF) == 0)
    cloned = kept & ((f & CLONE) != 0)
    split_kept = split & ((f & PRUNE_SAMPLE) == 0)
    si = split.nonzero().squeeze(1)
    ns = int(si.numel())
    rank = torch.cumsum(split.to(torch.int64), 0) - 1          # rank among ALL split rows
    ki, ci, ski = kept.nonzero().squeeze(1), cloned.nonzero().squeeze(1), split_kept.nonzero().squeeze(1)
    src = [ki, ci] + [ski] * N
    kind = [torch.full_like(ki, SURVIVOR), torch.full_like(ci, CLONED)] + [torch.full_like(ski, SAMPLE)] * N
    noise_row = [torch.full_like(ki, -1), torch.full_like(ci, -1)] + [k * ns + rank[ski] for k in range(N)]
    counts = [int(ki.numel()), int(ci.numel()), ns, int(ski.numel()), int(((f & CLONE) != 0).sum())]
    return torch.cat(src), torch.cat(kind), torch.cat(noise_row), counts


def returned_counts(counts, P, N):
    """(n_clone, n_split, n_pruned) as densify_and_prune returns them."""
    nk, nck, ns, nsk, ncl = counts
    return ncl, ns, (P - ns - nk) + (ncl - nck) + N * (ns - nsk)


def apply_table(model, src, kind, noise_row, noise, N):
    """(params, exp_avg, exp_avg_sq) as dicts field -> [P2, w] of the model the table describes."""
    opt = model.optimizer
    raw = {n: model.params[n].detach().reshape(model.P, w) for n, w in model.fields}
    m1, m2 = opt.field_views(opt.exp_avg), opt.field_views(opt.exp_avg_sq)
    surv = (kind == SURVIVOR)[:, None]
    sam = kind == SAMPLE
    p = {n: raw[n][src].clone() for n, _ in model.fields}
    a = {n: torch.where(surv, m1[n][src], torch.zeros_like(m1[n][src])) for n, _ in model.fields}
    b = {n: torch.where(surv, m2[n][src], torch.zeros_like(m2[n][src])) for n, _ in model.fields}
    if bool(sam.any()):
        s = src[sam]
        stds = torch.exp(raw["scaling"][s])
        samples = noise[noise_row[sam]] * stds
        rots = GaussianModelLite.build_rotation(raw["rotation"][s])
        p["xyz"][sam] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + raw["xyz"][s]
        p["scaling"][sam] = torch.log(stds / (0.8 * N))
    return p, a, b


# ---- shared inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(P, seed):
    knn = (lambda x: torch.full((x.shape[0],), 0.01)) if P < 4 else None   # (fewer than 3 neighbours)
    return synthetic.trained_like(P, seed=seed, scale_mult=1.5, knn=knn)


def build_model(api, device, P, seed, with_nir=False, spatial_order=False, overrides=True, percent_dense=None):
    """trained_like(P, seed, scale_mult=1.5) with the overrides of tests/test_densify_cpu.py, Adam moments and statistics from
    CPU generators (signed zeros among the moments), rows with constructed statistics, and selected rows on the first and
    last row of every 256-row block but one."""
    sc = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in _scene(P, seed).items()}
    m = GaussianModelLite(sc, torch.device(device), api=api, with_nir=with_nir, spatial_order=spatial_order)
    if percent_dense is not None:
        m.percent_dense = percent_dense
    g = torch.Generator().manual_seed(1000 + seed)
    n = m.flat.numel()
    ea = torch.randn(n, generator=g) * 1e-3
    ev = torch.rand(n, generator=g) * 1e-6
    ea[::7] = -0.0
    ev[::11] = 0.0
    accum = torch.rand((P, 1), generator=g) * 6e-4
    denom = torch.randint(0, 3, (P, 1), generator=g).float()   # zeros -> inf / NaN statistics
    with torch.no_grad():
        opac, scal = m.params["opacity"].detach().cpu().clone(), m.params["scaling"].detach().cpu().clone()
        if overrides:
            opac[::9] = -6.0
            scal[::31] = 0.2
            scal[::5] = -4.6
        nb = (P + 255) // 256
        for b in range(nb):
            lo, hi = b * 256, min(b * 256 + 255, P - 1)
            if nb >= 4 and b == EMPTY_BLOCK:
                accum[lo:hi + 1] = 0.0
            elif P > 1:
                accum[lo], denom[lo], accum[hi], denom[hi] = 1e-3, 1.0, 1e-3, 1.0
        if P >= 70:
            thr = float(f32(MAX_GRAD))
            accum[ROW_INF], denom[ROW_INF] = 3e-4, 0.0
            accum[ROW_NAN], denom[ROW_NAN] = 0.0, 0.0
            accum[ROW_NEG_SMALL], denom[ROW_NEG_SMALL], scal[ROW_NEG_SMALL] = -5e-4, 1.0, -4.6
            accum[ROW_NEG_LARGE], denom[ROW_NEG_LARGE], scal[ROW_NEG_LARGE] = -5e-4, 1.0, -1.0
            accum[ROW_EXACT], denom[ROW_EXACT], scal[ROW_EXACT] = thr, 1.0, -4.6
            accum[ROW_BELOW], denom[ROW_BELOW], scal[ROW_BELOW] = float(np.nextafter(np.float32(thr), np.float32(0))), 1.0, -4.6
            opac[ROW_INF:ROW_BELOW + 1] = 2.0
        m.params["opacity"].copy_(opac)
        m.params["scaling"].copy_(scal)
        m.optimizer.exp_avg.copy_(ea)
        m.optimizer.exp_avg_sq.copy_(ev)
        m.optimizer.invalidate_dormant()
    m.xyz_gradient_accum = accum.to(m.device)
    m.denom = denom.to(m.device)
    m.max_radii2D = (torch.rand((P,), generator=g) * 50).to(m.device)
    return m


def smallest_margin(m, extent, N, min_opacity=MIN_OPACITY):
    """The smallest relative distance (float64) of any row's decision value from its threshold: max scale against both scale
    bounds, the sample's scale against the world bound, sigmoid(opacity) against min_opacity."""
    s = torch.exp(m.params["scaling"].detach().cpu().double()).max(dim=1).values
    o = torch.sigmoid(m.params["opacity"].detach().cpu().double()).reshape(-1)
    rel = lambda v, t: float(((v - t).abs() / t).min())   # noqa: E731
    return min(rel(s, m.percent_dense * extent), rel(s, 0.1 * extent), rel(s / (0.8 * N), 0.1 * extent), rel(o, min_opacity))


def snapshot(m):
    """The model's rows as CPU tensors: (params, exp_avg, exp_avg_sq) dicts field -> [P, w]."""
    opt = m.optimizer
    p = {n: m.params[n].detach().reshape(m.P, w).cpu().clone() for n, w in m.fields}
    a = {n: v.cpu().clone() for n, v in opt.field_views(opt.exp_avg).items()}
    b = {n: v.cpu().clone() for n, v in opt.field_views(opt.exp_avg_sq).items()}
    return p, a, b


def bits(t):
    return t.contiguous().view(torch.int32)

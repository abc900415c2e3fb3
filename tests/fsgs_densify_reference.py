"""FSGS's densify_and_prune (FSGS/scene/gaussian_model.py:424-491) restated on plain tensors, and the inputs its tests share.

`densify_and_prune` goes through the reference's statements stage by stage - densify_and_clone, densify_and_split,
proximity, the final prune - with torch.cat and boolean indexing, and does to the two Adam moments what
cat_tensors_to_optimizer (zeros for the new rows) and _prune_optimizer (the same boolean index) do.  The kNN is the
caller's (`knn(xyz) -> (dist, nearest)`), the split noise comes from a CPU generator as in the host path of
GaussianModelLite.densify_and_prune_fsgs, which tests/test_fsgs_densify_cpu.py holds to this file bit for bit.

`build_model` makes the inputs of the CPU and the GPU tests from CPU generators only, so the CPU test can assert the input
conditions (decisive rows, separated neighbours, every rule selecting something) on exactly what the GPU tests use.
"""
import numpy as np
import torch

from gsplat_amd.trainer import GaussianModelLite

FIELDS = (("xyz", 3), ("features", 48), ("opacity", 1), ("scaling", 3), ("rotation", 4))
EXTENT, MAX_GRAD, MIN_OPACITY, DIST_THRES, PRUNE_FROM, PROX_UNTIL = 0.02, 2e-4, 0.005, 10.0, 500, 2000
PERCENT_DENSE = 0.01
SIZES, NS, SCREENS, ITERATIONS = (4, 70, 257, 1031), (2, 3), (None, 20), (400, 600, 2000)
SEED = 9     # (tuned until the restatement alone meets the input conditions of tests/test_fsgs_densify_cpu.py)
EMPTY_BLOCK = 2   # with four blocks or more: no row of this one is selected by any rule
ROW_INF, ROW_NAN, ROW_NEG_SMALL, ROW_NEG_LARGE, ROW_EXACT, ROW_BELOW = 11, 12, 13, 14, 16, 17
# the mean spacing of the centres: mean squared 3-NN distances straddle both 10 * EXTENT and 5 * EXTENT
SPACING = 0.62


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _cat(state, new):
    """cat_tensors_to_optimizer + densification_postfix: the new rows behind the old ones, their moments zero."""
    p, a, b = state
    return ({k: torch.cat((p[k], new[k]), dim=0) for k in p},
            {k: torch.cat((a[k], torch.zeros_like(new[k])), dim=0) for k in a},
            {k: torch.cat((b[k], torch.zeros_like(new[k])), dim=0) for k in b})


def _prune(state, mask, iteration, prune_from_iter):
    """prune_points: gated by the iteration; _prune_optimizer indexes parameters and both moments with ~mask."""
    if not iteration > prune_from_iter:
        return state, 0
    valid = ~mask
    return tuple({k: v[valid] for k, v in part.items()} for part in state), int(mask.sum())


def build_rotation(r):
    """FSGS/utils/general_utils.py: build_rotation."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3))
    rr, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - rr * z)
    R[:, 0, 2] = 2 * (x * z + rr * y)
    R[:, 1, 0] = 2 * (x * y + rr * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - rr * x)
    R[:, 2, 0] = 2 * (x * z - rr * y)
    R[:, 2, 1] = 2 * (y * z + rr * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def densify_and_prune(state, accum, denom, knn, max_grad, min_opacity, extent, max_screen_size, iteration, generator,
                      N=2, dist_thres=DIST_THRES, prune_from_iter=PRUNE_FROM, proximity_until_iter=PROX_UNTIL,
                      percent_dense=PERCENT_DENSE):
    """state = (params, exp_avg, exp_avg_sq), dicts field -> [P, w] CPU tensors.  -> (new state, (n_clone, n_split,
    n_proximity, n_pruned), info): info records every stage's mask and the two kNN point sets with what the kNN said, and
    info["computed"] = per final row, whether its xyz / its scaling goes back to a split sample's COMPUTED value (the sample
    itself, or a proximity row that took a sample as neighbour or partner) - everything else is a copy, or the midpoint of two
    copies, which any IEEE arithmetic forms alike."""
    info = {}
    n0 = state[0]["xyz"].shape[0]
    tag = dict(xyz=torch.zeros(n0, dtype=torch.bool), scaling=torch.zeros(n0, dtype=torch.bool))
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    # densify_and_clone
    scale = torch.exp(state[0]["scaling"])
    clone = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    clone = torch.logical_and(clone, torch.max(scale, dim=1).values <= percent_dense * extent)
    state = _cat(state, {k: v[clone] for k, v in state[0].items()})
    tag = {k: torch.cat((v, v[clone])) for k, v in tag.items()}
    info["clone"] = clone
    # densify_and_split
    p = state[0]
    n_init = p["xyz"].shape[0]
    padded = torch.zeros((n_init,))
    padded[:grads.shape[0]] = grads.squeeze(1)
    scale = torch.exp(p["scaling"])
    sel = torch.where(padded >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(scale, dim=1).values > percent_dense * extent)
    dist, nearest = knn(p["xyz"])
    sel2 = torch.logical_and(dist > (dist_thres * extent), torch.max(scale, dim=1).values > (extent))
    info.update(grad_split=sel, dist_split=sel2, knn1=dict(xyz=p["xyz"], scaling=p["scaling"], opacity=p["opacity"], dist=dist))
    sel = torch.logical_or(sel, sel2)
    ns = int(sel.sum())
    n_pruned = 0
    if ns:   # (the reference goes through the same statements with empty tensors)
        stds = scale[sel].repeat(N, 1)
        noise = torch.randn((ns * N, 3), generator=generator, dtype=torch.float32)
        samples = noise * stds
        rots = build_rotation(p["rotation"][sel]).repeat(N, 1, 1)
        new = {k: v[sel].repeat(N, 1) for k, v in p.items()}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p["xyz"][sel].repeat(N, 1)
        new["scaling"] = torch.log(scale[sel].repeat(N, 1) / (0.8 * N))
        state = _cat(state, new)
        tag = {k: torch.cat((v, torch.ones(N * ns, dtype=torch.bool))) for k, v in tag.items()}
        prune_filter = torch.cat((sel, torch.zeros(N * ns, dtype=bool)))
        state, n = _prune(state, prune_filter, iteration, prune_from_iter)
        if n:
            tag = {k: v[~prune_filter] for k, v in tag.items()}
        n_pruned += n
    # proximity
    n_prox = 0
    if iteration < proximity_until_iter:
        p = state[0]
        dist, nearest = knn(p["xyz"])
        psel = torch.logical_and(dist > (5. * extent), torch.max(torch.exp(p["scaling"]), dim=1).values > (extent))
        new_indices = nearest[psel].reshape(-1).long()
        source_xyz = p["xyz"][psel].repeat(1, 3, 1).reshape(-1, 3)
        target_xyz = p["xyz"][new_indices]
        new = dict(xyz=(source_xyz + target_xyz) / 2, scaling=p["scaling"][new_indices], opacity=p["opacity"][new_indices],
                   features=torch.zeros_like(p["features"][new_indices]), rotation=torch.zeros_like(p["rotation"][new_indices]))
        new["rotation"][:, 0] = 1
        info.update(proximity=psel, new_indices=new_indices,
                    knn2=dict(xyz=p["xyz"], scaling=p["scaling"], opacity=p["opacity"], dist=dist, nearest=nearest))
        n_prox = int(new_indices.numel())
        state = _cat(state, new)
        S = int(psel.sum())
        partner = psel.nonzero().squeeze(1)[torch.arange(3 * S) % max(S, 1)]
        tag = dict(xyz=torch.cat((tag["xyz"], tag["xyz"][new_indices] | tag["xyz"][partner])),
                   scaling=torch.cat((tag["scaling"], tag["scaling"][new_indices])))
    # the final prune
    p = state[0]
    prune_mask = (torch.sigmoid(p["opacity"]) < min_opacity).squeeze(1)
    info["faint"] = prune_mask.clone()
    if max_screen_size:
        big_points_vs = torch.zeros_like(prune_mask)   # max_radii2D was zeroed by every densification_postfix above
        big_points_ws = torch.exp(p["scaling"]).max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
    info["final"] = dict(scaling=p["scaling"], opacity=p["opacity"])
    state, n = _prune(state, prune_mask, iteration, prune_from_iter)
    if iteration > prune_from_iter:
        tag = {k: v[~prune_mask] for k, v in tag.items()}
    n_pruned += n
    info["computed"] = tag
    return state, (int(clone.sum()), ns, n_prox, n_pruned), info


# ---- shared inputs ------------------------------------------------------------------------------------------------------
def _scene(P, seed):
    g = torch.Generator().manual_seed(seed * 7919 + P)
    xyz = torch.rand((P, 3), generator=g) * (SPACING * P ** (1.0 / 3.0))
    # three classes of size against the bounds percent_dense * EXTENT = 2e-4 and EXTENT = 0.02: below both, between, above both
    cls = torch.randint(0, 3, (P,), generator=g)
    if P < 70:      # the smallest sizes hold both ends: rows a size test leaves behind, rows the distance rules can select
        cls[::2] = 0
        cls[1::2] = 2
    base = torch.tensor([1e-4, 1e-2, 1e-1])[cls]
    scales = base[:, None] * (0.3 + 0.6 * torch.rand((P, 3), generator=g))
    rots = torch.randn((P, 4), generator=g)
    opac = 0.05 + 0.9 * torch.rand((P, 1), generator=g)
    shs = torch.randn((P, 16, 3), generator=g) * 0.1
    return dict(means3D=xyz, scales=scales, rotations=rots, opacities=opac, shs=shs, sh_degree=3)


def build_model(api, device, P, seed=SEED, spatial_order=False):
    """P Gaussians whose spacing, sizes, statistics and opacities make every rule of the FSGS densification select some rows
    and not all; Adam moments with signed zeros; rows with constructed statistics (inf, NaN, negative, the threshold itself
    and the fp32 below it); selected rows on the first and last row of every 256-row block but one, which has none."""
    m = GaussianModelLite(_scene(P, seed), torch.device(device), api=api, spatial_order=spatial_order)
    g = torch.Generator().manual_seed(1000 + seed)
    n = m.flat.numel()
    ea = torch.randn(n, generator=g) * 1e-3
    ev = torch.rand(n, generator=g) * 1e-6
    ea[::7] = -0.0
    ev[::11] = 0.0
    accum = torch.rand((P, 1), generator=g) * 6e-4
    denom = torch.randint(0, 3, (P, 1), generator=g).float()
    with torch.no_grad():
        opac, scal = m.params["opacity"].detach().cpu().clone(), m.params["scaling"].detach().cpu().clone()
        opac[::9] = -6.0
        nb = (P + 255) // 256
        for b in range(nb):
            lo, hi = b * 256, min(b * 256 + 255, P - 1)
            if nb >= 4 and b == EMPTY_BLOCK:
                accum[lo:hi + 1] = 0.0
                scal[lo:hi + 1] = scal[lo:hi + 1].clamp(-8.0, -4.5)   # above 2e-4 (no clone), below EXTENT (no distance rule)
            else:
                accum[lo], denom[lo], accum[hi], denom[hi] = 1e-3, 1.0, 1e-3, 1.0
        if P >= 70:
            thr = float(f32(MAX_GRAD))
            accum[ROW_INF], denom[ROW_INF] = 3e-4, 0.0
            accum[ROW_NAN], denom[ROW_NAN] = 0.0, 0.0
            accum[ROW_NEG_SMALL], denom[ROW_NEG_SMALL], scal[ROW_NEG_SMALL] = -5e-4, 1.0, -9.5
            accum[ROW_NEG_LARGE], denom[ROW_NEG_LARGE], scal[ROW_NEG_LARGE] = -5e-4, 1.0, -5.0
            accum[ROW_EXACT], denom[ROW_EXACT], scal[ROW_EXACT] = thr, 1.0, -9.5
            accum[ROW_BELOW], denom[ROW_BELOW], scal[ROW_BELOW] = float(np.nextafter(np.float32(thr), np.float32(0))), 1.0, -9.5
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


def snapshot(m):
    """The model's rows as CPU tensors: (params, exp_avg, exp_avg_sq) dicts field -> [P, w]."""
    opt = m.optimizer
    p = {n: m.params[n].detach().reshape(m.P, w).cpu().clone() for n, w in m.fields}
    a = {n: v.cpu().clone() for n, v in opt.field_views(opt.exp_avg).items()}
    b = {n: v.cpu().clone() for n, v in opt.field_views(opt.exp_avg_sq).items()}
    return p, a, b


def bits(t):
    return t.contiguous().view(torch.int32)


def run_reference(m, knn, iteration, N, screen, seed=77):
    """The restatement applied to model m (which is left alone): -> (state, counts, info)."""
    return densify_and_prune(snapshot(m), m.xyz_gradient_accum.cpu().clone(), m.denom.cpu().clone(), knn, MAX_GRAD, MIN_OPACITY,
                             EXTENT, screen, iteration, torch.Generator().manual_seed(seed), N=N,
                             percent_dense=m.percent_dense)


def run_model(m, iteration, N, screen, seed=77, **kw):
    gen = torch.Generator().manual_seed(seed)
    out = m.densify_and_prune_fsgs(MAX_GRAD, MIN_OPACITY, EXTENT, screen, iteration, dist_thres=DIST_THRES,
                                   prune_from_iter=PRUNE_FROM, proximity_until_iter=PROX_UNTIL, generator=gen, N=N, **kw)
    return out, gen


def _rel(v, t):
    return float(((v.double() - t).abs() / abs(t)).min()) if v.numel() else float("inf")


def smallest_margin(info, accum, denom, N, screen, percent_dense=PERCENT_DENSE, extent=EXTENT, dist_thres=DIST_THRES,
                    max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, constructed=True):
    """The smallest relative distance (float64) of any decision value from its threshold over the stages `info` records: the
    largest scale against percent_dense * extent, extent (both kNN sets: the distance split and proximity) and 0.1 * extent
    (final set, with a screen size), both mean distances against their bounds, sigmoid(opacity) against min_opacity, and the
    statistic against max_grad.  `constructed` (build_model's inputs): the rows ROW_EXACT / ROW_BELOW are left out of the last -
    they sit ON the threshold and one fp32 below it by construction, and their g = accum / 1 is exact in any IEEE arithmetic."""
    k1 = info["knn1"]
    s1 = torch.exp(k1["scaling"].double()).max(dim=1).values
    out = [_rel(s1, percent_dense * extent), _rel(s1, extent), _rel(k1["dist"], dist_thres * extent)]
    if "knn2" in info:
        k2 = info["knn2"]
        out += [_rel(torch.exp(k2["scaling"].double()).max(dim=1).values, extent), _rel(k2["dist"], 5.0 * extent)]
    fin = info["final"]
    out.append(_rel(torch.sigmoid(fin["opacity"].double()), min_opacity))
    if screen:
        out.append(_rel(torch.exp(fin["scaling"].double()).max(dim=1).values, 0.1 * extent))
    g = (accum.double() / denom.double()).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    rows = torch.ones_like(g, dtype=torch.bool)
    if constructed and g.numel() >= 70:
        rows[ROW_EXACT] = rows[ROW_BELOW] = False
    g = g[rows & g.isfinite()]
    out += [_rel(g, max_grad), _rel(g.abs(), max_grad)]
    return min(out)


def neighbours_are_separated(k, rel=1e-5):
    """For every row of a kNN point set: the squared distances (float64) to its 1st .. 4th neighbour differ by more than `rel`
    relative, OR the two tied points carry identical centre, scaling and opacity (a source and its clone) - so whichever
    of them a kNN implementation reports, the rows built from it are the same."""
    x = k["xyz"].double()
    n = x.shape[0]
    if n < 4:
        return False
    d = torch.cdist(x, x) ** 2
    d.fill_diagonal_(float("inf"))
    kk = min(4, n - 1)   # (four points: the three neighbours are all the others, only their order is at stake)
    val, idx = torch.topk(d, kk, dim=1, largest=False)
    for j in range(kk - 1):
        tied = (val[:, j + 1] - val[:, j]) <= rel * val[:, j + 1]
        a, b = idx[tied, j], idx[tied, j + 1]
        same = ((k["xyz"][a] == k["xyz"][b]).all(dim=1) & (k["scaling"][a] == k["scaling"][b]).all(dim=1) &
                (k["opacity"][a] == k["opacity"][b]).all(dim=1))
        if not bool(same.all()):
            return False
    return True

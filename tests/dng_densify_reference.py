"""DNGaussian's densify_and_prune, prune_points, prune and opacity resets (DNGaussian/scene/gaussian_model.py:296-306, 355-392,
403-524, 536-538) restated on plain tensors with a torch.optim.Adam state per group, a torch restatement of the device form
(csrc/gs_densify.hip: gs_densify_plan_gated, gs_prune_plan, gs_prune_emit), and the inputs the tests share.

`Reference` goes through the reference's statements in the reference's order: every prune_points indexes each group's parameter
and both moments with the same boolean mask and re-registers the state under the new parameter (_prune_optimizer), every
densification_postfix appends rows with zero moments (cat_tensors_to_optimizer) and zeroes the statistics, densify_and_clone and
densify_and_split are gated by get_opacity > opa_thresh, the split originals leave through prune_points, and the final prune is
by opacity alone: its max_screen_size branch reads max_radii2D, which the postfix has just zeroed.  The split noise is CPU randn
from a generator times the stds, as GaussianModelLite draws it (the reference calls torch.normal on the device).
tests/test_dng_densify_cpu.py holds GaussianModelLite's host methods to this file bit for bit.

`gated_flags`, `prune_block_counts` and `prune_table` restate what the kernels decide; `build_model` and `mask_patterns` make the
inputs of the CPU and the GPU tests from CPU generators only, so the CPU test can assert the margin condition on exactly what
the GPU tests use.
"""
import torch

import densify_reference as dr

EXTENT, MAX_GRAD, MIN_OPACITY, OPA_THRESH = dr.EXTENT, dr.MAX_GRAD, dr.MIN_OPACITY, 0.1
SIZES, SEEDS, NS = dr.SIZES, (7, 5), (2, 3)
REL = 1e-4   # how far the placed opacities sit from their thresholds, relative
# rows placed in models of 70 rows or more (beside densify_reference's statistic rows 11 .. 17)
ROW_CLONE_OPEN, ROW_CLONE_SHUT = 20, 21      # clone candidates, sigmoid(opacity) = OPA_THRESH (1 + REL) / (1 - REL)
ROW_SPLIT_OPEN, ROW_SPLIT_SHUT = 22, 23      # split candidates, likewise
ROW_KEPT, ROW_FAINT = 24, 26                 # sigmoid(opacity) = MIN_OPACITY (1 + REL) / (1 - REL)
ROW_GATED_CLONE, ROW_GATED_SPLIT = 28, 29    # pass the gradient and size tests, opacity 0.05: stopped by the gate alone
PLACED = (ROW_CLONE_OPEN, ROW_CLONE_SHUT, ROW_SPLIT_OPEN, ROW_SPLIT_SHUT, ROW_KEPT, ROW_FAINT, ROW_GATED_CLONE, ROW_GATED_SPLIT)
SMALL_SCALE, LARGE_SCALE = -4.6, -1.0        # exp: 0.01 and 0.37 against percent_dense * EXTENT = 0.044


def logit(p):
    p = torch.tensor(p, dtype=torch.float64)
    return float(torch.log(p / (1 - p)))


def build_rotation(r):
    """DNGaussian/utils/general_utils.py: build_rotation (the quaternion normalised first), on r's device."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


# ---- the reference's sequence ------------------------------------------------------------------------------------------------
class Reference:
    """The per-Gaussian part of DNGaussian's GaussianModel on plain tensors: one parameter and one Adam group per field."""

    def __init__(self, params, exp_avg, exp_avg_sq, accum, denom, max_radii2D, percent_dense=0.01):
        self.percent_dense = percent_dense
        self.names = list(params)
        self.p = {k: torch.nn.Parameter(params[k].clone().requires_grad_(True)) for k in self.names}
        self.optimizer = torch.optim.Adam([{"params": [self.p[k]], "lr": 0.0, "name": k} for k in self.names], lr=0.0, eps=1e-15)
        for k in self.names:
            self.optimizer.state[self.p[k]] = {"step": torch.tensor(0.0), "exp_avg": exp_avg[k].clone(),
                                               "exp_avg_sq": exp_avg_sq[k].clone()}
        self.xyz_gradient_accum, self.denom, self.max_radii2D = accum.clone(), denom.clone(), max_radii2D.clone()

    @classmethod
    def of(cls, m):
        """The restatement's copy of a GaussianModelLite (which is left alone), on the model's device."""
        opt = m.optimizer
        p = {n: m.params[n].detach().reshape(m.P, w) for n, w in m.fields}
        return cls(p, opt.field_views(opt.exp_avg), opt.field_views(opt.exp_avg_sq), m.xyz_gradient_accum, m.denom, m.max_radii2D,
                   m.percent_dense)

    @property
    def P(self):
        return self.p["xyz"].shape[0]

    @property
    def get_scaling(self):
        return torch.exp(self.p["scaling"])

    @property
    def get_opacity(self):
        return torch.sigmoid(self.p["opacity"])

    def state(self):
        """(params, exp_avg, exp_avg_sq) as dicts field -> [P, w] CPU tensors."""
        st = {k: self.optimizer.state[self.p[k]] for k in self.names}
        return ({k: self.p[k].detach().cpu() for k in self.names}, {k: st[k]["exp_avg"].cpu() for k in self.names},
                {k: st[k]["exp_avg_sq"].cpu() for k in self.names})

    def _reregister(self, group, tensor, stored):
        del self.optimizer.state[group["params"][0]]
        group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
        self.optimizer.state[group["params"][0]] = stored
        self.p[group["name"]] = group["params"][0]

    def _prune_optimizer(self, valid):
        for group in self.optimizer.param_groups:
            stored = self.optimizer.state[group["params"][0]]
            stored["exp_avg"] = stored["exp_avg"][valid]
            stored["exp_avg_sq"] = stored["exp_avg_sq"][valid]
            self._reregister(group, group["params"][0].detach()[valid], stored)

    def prune_points(self, mask):
        valid = ~mask
        self._prune_optimizer(valid)
        self.xyz_gradient_accum = self.xyz_gradient_accum[valid]
        self.denom = self.denom[valid]
        self.max_radii2D = self.max_radii2D[valid]

    def densification_postfix(self, new):
        for group in self.optimizer.param_groups:
            ext = new[group["name"]]
            stored = self.optimizer.state[group["params"][0]]
            stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(ext)), dim=0)
            stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            self._reregister(group, torch.cat((group["params"][0].detach(), ext), dim=0), stored)
        dev = self.p["xyz"].device
        self.xyz_gradient_accum = torch.zeros((self.P, 1), device=dev)
        self.denom = torch.zeros((self.P, 1), device=dev)
        self.max_radii2D = torch.zeros((self.P,), device=dev)

    def densify_and_clone(self, grads, grad_threshold, scene_extent, opa_thresh):
        sel = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
        sel = torch.logical_and(sel, torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        sel = torch.logical_and(sel, self.get_opacity.squeeze(1) > opa_thresh)
        self.densification_postfix({k: self.p[k].detach()[sel] for k in self.names})
        return int(sel.sum())

    def densify_and_split(self, grads, grad_threshold, scene_extent, opa_thresh, generator, N=2):
        n_init = self.P
        dev = self.p["xyz"].device
        padded = torch.zeros((n_init,), device=dev)
        padded[:grads.shape[0]] = grads.squeeze(1)
        base = torch.where(padded >= grad_threshold, True, False)
        base = torch.logical_and(base, torch.max(self.get_scaling, dim=1).values > self.percent_dense * scene_extent)
        sel = torch.logical_and(base, self.get_opacity.squeeze(1) > opa_thresh)
        ns = int(sel.sum())
        raw = {k: self.p[k].detach() for k in self.names}
        stds = self.get_scaling.detach()[sel].repeat(N, 1)
        noise = torch.randn((ns * N, 3), generator=generator, dtype=torch.float32).to(dev) if ns else torch.zeros((0, 3), device=dev)
        samples = noise * stds
        rots = build_rotation(raw["rotation"][sel]).repeat(N, 1, 1)
        new = {k: raw[k][sel].repeat(N, 1) for k in self.names}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + raw["xyz"][sel].repeat(N, 1)
        new["scaling"] = torch.log(self.get_scaling.detach()[sel].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new)
        self.prune_points(torch.cat((sel, torch.zeros(N * ns, device=dev, dtype=torch.bool))))
        return ns

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, opa_thresh, max_dist, knn=None, generator=None,
                          N=2):
        """-> (n_outliers, n_clone, n_split, n_pruned).  knn(xyz) -> mean squared 3-NN distances [P] (distCUDA2)."""
        n_out = 0
        if max_dist is not None:
            d = torch.sqrt(knn(self.p["xyz"].detach()))
            outliers = (d.view(max_dist.shape) > max_dist) if torch.is_tensor(max_dist) else (d > max_dist)
            outliers = outliers.reshape(-1)
            n_out = int(outliers.sum())
            self.prune_points(outliers)
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        n_clone = self.densify_and_clone(grads, max_grad, extent, opa_thresh)
        n_split = self.densify_and_split(grads, max_grad, extent, opa_thresh, generator, N)
        prune_mask = (self.get_opacity < min_opacity).squeeze(1)
        if max_screen_size:
            prune_mask = prune_mask | (self.max_radii2D > max_screen_size)   # all False: the postfix has just zeroed it
        self.prune_points(prune_mask)
        return n_out, n_clone, n_split, int(prune_mask.sum())

    def prune(self, min_opacity):
        mask = (self.get_opacity < min_opacity).squeeze(1)
        self.prune_points(mask)
        return int(mask.sum())

    def _replace_opacity(self, tensor):
        for group in self.optimizer.param_groups:
            if group["name"] == "opacity":
                stored = self.optimizer.state[group["params"][0]]
                stored["exp_avg"] = torch.zeros_like(tensor)
                stored["exp_avg_sq"] = torch.zeros_like(tensor)
                self._reregister(group, tensor, stored)

    def reset_opacity(self, value=0.01):
        x = torch.min(self.get_opacity.detach(), torch.ones_like(self.get_opacity) * value)
        self._replace_opacity(torch.log(x / (1 - x)))

    def reset_opacity_max(self, value=0.8):
        x = torch.max(self.get_opacity.detach(), torch.ones_like(self.get_opacity) * value)
        self._replace_opacity(torch.log(x / (1 - x)))


# ---- the device form ---------------------------------------------------------------------------------------------------------
def thresholds(N, percent_dense=0.01, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT):
    return dr.thresholds(max_grad, min_opacity, extent, percent_dense, N)


def gated_flags(scaling, opacity, accum, denom, thr, gate_opacity, size_test=False):
    """gs_densify_plan_gated's flag bytes: gs_densify_plan's, with CLONE and SPLIT only where sigmoid(opacity) > the fp32 gate."""
    flags = dr.plan_flags(scaling, opacity, accum, denom, thr, size_test)
    shut = ~(torch.sigmoid(opacity.reshape(-1)) > dr.f32(gate_opacity))
    return torch.where(shut, flags & ~torch.tensor(dr.CLONE | dr.SPLIT, dtype=torch.uint8), flags)


def prune_block_counts(mask):
    """gs_prune_plan: rows kept per 256-row block."""
    keep = (mask.reshape(-1) == 0).to(torch.int64)
    nb = (keep.numel() + 255) // 256
    return torch.nn.functional.pad(keep, (0, nb * 256 - keep.numel())).view(nb, 256).sum(dim=1)


def prune_table(mask):
    """gs_prune_emit's table: destination row = exclusive block prefix + rank inside the block -> the source row of every
    destination row (every kind a survivor), built the way the kernel places them."""
    keep = mask.reshape(-1) == 0
    counts = prune_block_counts(mask)
    prefix = torch.cumsum(counts, 0) - counts
    src = torch.full((int(counts.sum()),), -1, dtype=torch.int64)
    for b in range(counts.numel()):
        rows = keep[b * 256:(b + 1) * 256].nonzero().squeeze(1) + b * 256
        src[int(prefix[b]) + torch.arange(rows.numel())] = rows
    return src


# ---- shared inputs -----------------------------------------------------------------------------------------------------------
def build_model(api, device, P, seed, with_nir=False, spatial_order=False):
    """densify_reference.build_model (statistic rows inf, NaN, negative, exact, just below; selected rows at block edges; signed
    zeros among the moments) plus, from 70 rows, the rows DNGaussian's rule turns on: opacities REL above and below opa_thresh on
    clone and on split candidates, REL above and below min_opacity, and a clone and a split candidate that fail the gate alone."""
    m = dr.build_model(api, device, P, seed, with_nir=with_nir, spatial_order=spatial_order)
    if P >= 70:
        with torch.no_grad():
            opac, scal = m.params["opacity"].detach().cpu().clone(), m.params["scaling"].detach().cpu().clone()
            accum, denom = m.xyz_gradient_accum.cpu().clone(), m.denom.cpu().clone()
            for r in PLACED:
                accum[r], denom[r] = 1e-3, 1.0
            for r, s, o in ((ROW_CLONE_OPEN, SMALL_SCALE, OPA_THRESH * (1 + REL)), (ROW_CLONE_SHUT, SMALL_SCALE, OPA_THRESH * (1 - REL)),
                            (ROW_SPLIT_OPEN, LARGE_SCALE, OPA_THRESH * (1 + REL)), (ROW_SPLIT_SHUT, LARGE_SCALE, OPA_THRESH * (1 - REL)),
                            (ROW_KEPT, SMALL_SCALE, MIN_OPACITY * (1 + REL)), (ROW_FAINT, SMALL_SCALE, MIN_OPACITY * (1 - REL)),
                            (ROW_GATED_CLONE, SMALL_SCALE, 0.05), (ROW_GATED_SPLIT, LARGE_SCALE, 0.05)):
                scal[r], opac[r] = s, logit(o)
            m.params["opacity"].copy_(opac)
            m.params["scaling"].copy_(scal)
        m.xyz_gradient_accum, m.denom = accum.to(m.device), denom.to(m.device)
    return m


def mask_patterns(P, seed=0):
    """name -> bool [P], True = the row goes."""
    g = torch.Generator().manual_seed(4000 + 17 * seed + P)
    rows = torch.arange(P)
    block = 1 if P >= 512 else 0            # a whole 256-row block (the model's only, cut short, below 512 rows)
    in_block = (rows // 256) == block
    out = {"all_false": torch.zeros(P, dtype=torch.bool), "all_true": torch.ones(P, dtype=torch.bool),
           "only_first_kept": rows != 0, "only_last_kept": rows != P - 1,
           "rows_255_256": (rows == 255) | (rows == 256), "block_removed": in_block, "block_kept_alone": ~in_block,
           "alternating": rows % 2 == 0, "random_1pct": torch.rand(P, generator=g) < 0.01,
           "random_50pct": torch.rand(P, generator=g) < 0.5}
    return out


def smallest_margin(m, N, opa_thresh=OPA_THRESH, min_opacity=MIN_OPACITY, max_grad=MAX_GRAD, extent=EXTENT, constructed=True):
    """The smallest relative distance (float64) of any row's decision value from its threshold: densify_reference's (largest
    scale against the scale bounds, sigmoid(opacity) against min_opacity), sigmoid(opacity) against the gate, and the statistic
    g and |g| against max_grad.  Left out of the last (`constructed`: build_model's inputs): ROW_EXACT and ROW_BELOW, which sit ON
    the threshold and one fp32 below it by construction - their g = accum / 1 is exact in any IEEE arithmetic -, and the
    non-finite statistics, which no rounding moves."""
    o = torch.sigmoid(m.params["opacity"].detach().cpu().double()).reshape(-1)
    g = (m.xyz_gradient_accum.cpu().double() / m.denom.cpu().double()).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    rows = g.isfinite()
    if constructed and m.P >= 70:
        rows[dr.ROW_EXACT] = rows[dr.ROW_BELOW] = False
    g = g[rows]
    rel = lambda v, t: float(((v - t).abs() / t).min()) if v.numel() else float("inf")   # noqa: E731
    return min(dr.smallest_margin(m, extent, N, min_opacity), rel(o, opa_thresh), rel(g, max_grad), rel(g.abs(), max_grad))


def snapshot(m):
    return dr.snapshot(m)


def statistics(m):
    return m.xyz_gradient_accum.cpu().clone(), m.denom.cpu().clone(), m.max_radii2D.cpu().clone()


bits = dr.bits

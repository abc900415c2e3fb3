"""Build-owned counterpart of the reference's training step (the reference's Python never travels).

  GaussianModel.get_*            LGDWT-GS/scene/gaussian_model.py:40-60,102-135  (activations)
  training_setup / Adam groups   LGDWT-GS/scene/gaussian_model.py:178-201        (per-group LRs, eps 1e-15)
  render()                       LGDWT-GS/gaussian_renderer/__init__.py:18-128   (argument / return contract)
  one iteration                  LGDWT-GS/train.py:97-218,279-288                 (render, losses, backward, Adam)
  densify / prune / reset        LGDWT-GS/scene/gaussian_model.py:258-261,316-473 (clone, split, prune, moments)
  schedule                       LGDWT-GS/train.py:99-111,262-288, arguments/__init__.py:78-100

MI355X-first differences:
  * the six parameter tensors are views into ONE flat fp32 buffer and their gradients views into one
    flat gradient buffer, so that the data-parallel exchange is a single RCCL all-reduce of 59 floats per
    Gaussian with no packing copies;
  * cameras are sharded over ranks (one camera per GPU per step); every rank holds a full replica and
    applies the identical Adam step after the all-reduce, so replicas stay bit-identical;
  * densification statistics (xyz_gradient_accum, denom: sum; max_radii2D: max) are reduced too
    (gaussian_model.py:471-473, train.py:266-268).
"""
import math

import torch
import torch.distributed as dist

# flat layout: one segment per field; the SH block keeps DC and rest interleaved [P,16,3] exactly as the
# rasterizer reads it, so get_features is a view (the reference concatenates _features_dc/_features_rest
# every step: gaussian_model.py:119-123).  The two learning rates of that block alternate with period 48.
FIELDS = (("xyz", 3), ("features", 48), ("opacity", 1), ("scaling", 3), ("rotation", 4))
FLOATS_PER_GAUSSIAN = sum(n for _, n in FIELDS)  # 59
# LGDWT-GS/arguments/__init__.py:79-86 (position_lr_init, feature_lr, opacity_lr, scaling_lr, rotation_lr)
LRS = {"xyz": 0.00016, "f_dc": 0.0025, "f_rest": 0.0025 / 20.0, "opacity": 0.025, "scaling": 0.005, "rotation": 0.001,
       # multispectral variant (mult-dwtgs/scene/gaussian_model.py:266-280): albedo at position_lr_init (unscaled,
       # no schedule), the global gain at feature_lr
       "nir_albedo": 0.00016, "nir_gain": 0.0025}
NIR_FIELD = ("nir_albedo", 1)
SHARD_UNIT = 4 * 840  # float4 x lcm(1..8)


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """get_expon_lr_func of LGDWT-GS/utils/general_utils.py:29-62 (pinned by tests/golden/schedule.npz)."""
    import numpy as np
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    else:
        delay_rate = 1.0
    t = np.clip(step / max_steps, 0, 1)
    log_lerp = np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
    return float(delay_rate * log_lerp)


class FlatAdam:
    """torch.optim.Adam(lr=0.0, eps=1e-15) with the reference's per-group learning rates
    (gaussian_model.py:183-193), as ONE fused pass over the flat buffers through gs_adam_step."""

    def __init__(self, api, model, betas=(0.9, 0.999), eps=1e-15):
        from .capi import GsAdamSeg
        self.api, self.model, self.betas, self.eps = api, model, betas, eps
        self.alloc_moments()
        self.t = 0
        # torch keeps Adam's step count per parameter; a group that is skipped (no gradient after its tensor
        # was replaced) falls behind the others
        self.seg_steps = {name: 0 for name, _ in model.fields}
        if getattr(model, "with_nir", False):
            self.seg_steps["nir_gain"] = 0   # the global gain (not a per-Gaussian field): stepped with every optimizer step
        self.lr = dict(LRS)
        self.lr["xyz"] = LRS["xyz"] * model.spatial_lr_scale
        self._Seg = GsAdamSeg
        # optimizer_type = "sparse_adam" (arguments/__init__.py:101, train.py:282-284: `visible = radii > 0;
        # optimizer.step(visible, N)`): only the Gaussians visible in the step's view(s) are stepped; parameters and moments of
        # the others keep their bits.  (The optimizer class the reference would use, SparseGaussianAdam, lives in the 3dgs_accel
        # branch of the rasterizer, which the reference does not vendor - its pinned branch is dr_aa; the update applied to a
        # visible row here is torch.optim.Adam's, bias correction by the group's step count included.)
        self.sparse = False

    def alloc_moments(self):
        """Zeroed moment buffers for the model's current size, padded like the parameters (the sharded optimizer
        all-gathers them in place before a re-layout or a checkpoint)."""
        m = self.model
        self.exp_avg_padded = torch.zeros_like(m.flat_padded)
        self.exp_avg_sq_padded = torch.zeros_like(m.flat_padded)
        self.exp_avg = self.exp_avg_padded[:m.flat.numel()]
        self.exp_avg_sq = self.exp_avg_sq_padded[:m.flat.numel()]
        self._dormant, self._dormant_valid = None, False

    # Dormant blocks (GsStepState.dormant, include/gsplat.h): one byte per 256 consecutive Gaussians, 1 = every Adam moment
    # of every row of the block is +0, so the zero-gradient update is a no-op and gs_backward_step / gs_step_uninstanced
    # skip the block's parameter and moment traffic.  DERIVED from the moments (never assumed), kept current by the fused
    # kernels (a block that receives a gradient is cleared on the device) and recomputed after anything else wrote the
    # moments (invalidate_dormant).  Pays when the rows are in spatial order (GaussianModelLite(spatial_order=True)): the
    # Gaussians no camera reaches - more than half of bench.py's scene - then fill whole blocks.  GS_DORMANT_BLOCKS=0: off.
    USE_DORMANT = __import__("os").environ.get("GS_DORMANT_BLOCKS", "1") != "0"
    DORMANT_BLOCK = 256

    def invalidate_dormant(self):
        self._dormant_valid = False

    def dormant_flags(self):
        """The current flags (uint8 [ceil(P / 256)], same tensor until the model is re-laid out), recomputed from the moment
        buffers when something other than the fused step may have written them."""
        m = self.model
        B = self.DORMANT_BLOCK
        nb = (m.P + B - 1) // B
        if getattr(self, "_dormant", None) is None or self._dormant.numel() != nb or self._dormant.device != m.flat.device:
            self._dormant = torch.zeros((nb,), dtype=torch.uint8, device=m.flat.device)
            self._dormant_valid = False
        if not self._dormant_valid:
            with torch.no_grad():
                live = torch.zeros((nb * B,), dtype=torch.bool, device=m.flat.device)
                for buf in (self.exp_avg, self.exp_avg_sq):
                    for name, view in self.field_views(buf).items():
                        live[:m.P] |= (view.view(torch.int32) != 0).any(dim=1)   # (bit patterns: -0.0 is not +0)
                self._dormant.copy_((~live.view(nb, B).any(dim=1)).to(torch.uint8))
            self._dormant_valid = True
        return self._dormant

    def segments(self, skip=()):
        P = self.model.P
        names = [(name, n) for name, n in self.model.fields]
        segs = (self._Seg * len(names))()
        off, k = 0, 0
        for name, n in names:
            if name not in skip:
                segs[k].begin, segs[k].end = off, off + P * n
                if name == "features":
                    segs[k].lr_a, segs[k].lr_b, segs[k].period, segs[k].split = self.lr["f_dc"], self.lr["f_rest"], 48, 3
                else:
                    segs[k].lr_a, segs[k].lr_b, segs[k].period, segs[k].split = self.lr[name], 0.0, 0, 0
                segs[k].step = self.seg_steps[name]
                segs[k].row_width = n
                k += 1
            off += P * n
        return segs, k

    def step(self, skip=(), row_mask=None):
        """skip: fields without a gradient this iteration (their tensor was replaced after backward: torch's
        optimizer.step() leaves such a parameter, its moments and its step count alone).
        row_mask (sparse_adam): float [P], > 0 = the Gaussian is stepped."""
        self.begin_step(skip)
        self.step_range(0, self.model.flat.numel(), skip, row_mask=row_mask)

    def begin_step(self, skip=()):
        self.t += 1
        for name, _ in self.model.fields:
            if name not in skip:
                self.seg_steps[name] += 1
        if "nir_gain" in self.seg_steps:
            self.seg_steps["nir_gain"] += 1

    def _nir_into(self, st, grads_out):
        """The 4th channel's part of a GsStepState (multispectral model): raw albedo row, global gain, moments, rates."""
        m = self.model
        if not m.with_nir:
            return
        st.extra = m.params["nir_albedo"].data_ptr()
        st.gain = m.nir_gain.data_ptr()
        st.lr_extra, st.lr_gain = self.lr["nir_albedo"], self.lr["nir_gain"]
        if grads_out:
            st.grad_out_extra = m.grad_views()["nir_albedo"].data_ptr()
            st.grad_out_gain = m.gain_grad_word.data_ptr()
            st.step_extra = st.step_gain = 1
            return
        ea, eas = self.field_views(self.exp_avg), self.field_views(self.exp_avg_sq)
        st.extra_m, st.extra_v = ea["nir_albedo"].data_ptr(), eas["nir_albedo"].data_ptr()
        gs = m.nir_gain_optimizer.state[m.nir_gain]
        st.gain_m, st.gain_v = gs["exp_avg"].data_ptr(), gs["exp_avg_sq"].data_ptr()
        st.step_extra = self.seg_steps["nir_albedo"] if self.seg_steps["nir_albedo"] > 0 else self.t
        st.step_gain = self.seg_steps["nir_gain"]

    def grads_out_request(self):
        """The GsStepState of the data-parallel form of gs_backward_step: raw rows in, gradients OUT into the flat gradient
        buffer (nothing to pack before the exchange), this view's statistic increments into `stat_delta`, the validity
        flag into the exchange buffer's tail.  Counters are not touched (exchange_and_step advances them)."""
        from .capi import GsStepState
        m = self.model
        st = GsStepState()
        p, gv = self.field_views(m.flat), m.grad_views()
        for k, name in enumerate(self.ROWS):
            setattr(st, name, p[name].data_ptr())
            st.grad_out[k] = gv[name].data_ptr()
            st.step[k] = 1
        st.beta1, st.beta2, st.eps = self.betas[0], self.betas[1], self.eps
        st.max_radii2D = m.max_radii2D.data_ptr()
        st.xyz_gradient_accum, st.denom = m.stat_delta[0].data_ptr(), m.stat_delta[1].data_ptr()
        st.fail_flag = m.fail_flag.data_ptr()
        st.grad_mask = m.grad_mask.data_ptr()
        self._nir_into(st, True)
        return st

    def step_range(self, lo, hi, skip=(), grads=None, gate=None, row_mask=None):
        """The update of elements [lo, hi) of the flat buffers (lo a multiple of 4): the data-parallel step applies
        Adam chunk by chunk as the chunks of the gradient all-reduce arrive.  The segment table is shifted by -lo so
        that the kernel's element index i stands for element lo + i (a negative `begin` keeps the phase of the
        interleaved SH learning rates)."""
        import ctypes as C
        m = self.model
        segs, nseg = self.segments(skip)
        if nseg == 0 or hi <= lo:
            return
        self._dormant_valid = False   # (gs_adam_step writes moments without keeping the dormant-block flags)
        for k in range(nseg):
            segs[k].begin -= lo
            segs[k].end -= lo
        stream = C.c_void_p(torch.cuda.current_stream(m.flat.device).cuda_stream) if m.flat.is_cuda else None
        # grads: a tensor holding the gradients of elements [lo, hi) (default: that slice of the flat gradient buffer)
        gptr = m.flat_grad.data_ptr() + 4 * lo if grads is None else grads.data_ptr()
        if self.sparse and row_mask is None:
            raise RuntimeError("sparse_adam: the step needs the view's visibility (row_mask)")
        if row_mask is not None:   # (sparse_adam, or one part of a step that is applied in two parts: the sparse exchange)
            self.api.call("adam_step_masked", m.flat.data_ptr() + 4 * lo, gptr,
                          self.exp_avg.data_ptr() + 4 * lo, self.exp_avg_sq.data_ptr() + 4 * lo, hi - lo, segs, nseg,
                          self.betas[0], self.betas[1], self.eps, self.t, None if gate is None else gate.data_ptr(),
                          row_mask.data_ptr(), stream)
            return
        if gate is not None:  # a device float: the update is a no-op on the device when it is non-zero (gs_adam_step_gated)
            self.api.call("adam_step_gated", m.flat.data_ptr() + 4 * lo, gptr,
                          self.exp_avg.data_ptr() + 4 * lo, self.exp_avg_sq.data_ptr() + 4 * lo, hi - lo, segs, nseg,
                          self.betas[0], self.betas[1], self.eps, self.t, gate.data_ptr(), stream)
            return
        self.api.call("adam_step", m.flat.data_ptr() + 4 * lo, gptr,
                      self.exp_avg.data_ptr() + 4 * lo, self.exp_avg_sq.data_ptr() + 4 * lo, hi - lo, segs, nseg,
                      self.betas[0], self.betas[1], self.eps, self.t, stream)

    ROWS = ("xyz", "features", "opacity", "scaling", "rotation")
    LR_CLASSES = (("xyz", 0), ("f_dc", 1), ("f_rest", 1), ("opacity", 2), ("scaling", 3), ("rotation", 4))

    def step_coefficients(self, skip=()):
        """The 11 step-dependent constants of gs_backward_step for the CURRENT counters (call after begin_step):
        lr / (1 - beta1^t) per learning-rate class, 1 / sqrt(1 - beta2^t) per row - in the float arithmetic of
        gs_adam_step (double, rounded once; the product lr * 1/(1 - beta1^t) in float).  Always 15 floats: words 11..14 are
        the same two constants of the multispectral model's 4th-channel row and of its gain (zero without them)."""
        import numpy as np
        t = [self.seg_steps[name] if self.seg_steps[name] > 0 else self.t for name in self.ROWS]
        t = [max(x, 1) for x in t]
        b1, b2 = (float(np.float32(b)) for b in self.betas)  # the C ABI takes the betas as float
        out = np.zeros(15, dtype=np.float32)
        for c, (name, row) in enumerate(self.LR_CLASSES):
            out[c] = np.float32(self.lr[name]) * np.float32(1.0 / (1.0 - b1 ** t[row]))
        for k in range(5):
            out[6 + k] = np.float32(1.0 / math.sqrt(1.0 - b2 ** t[k]))
        if getattr(self.model, "with_nir", False):
            for k, name in enumerate(("nir_albedo", "nir_gain")):
                tk = max(self.seg_steps[name] if self.seg_steps[name] > 0 else self.t, 1)
                out[11 + 2 * k] = np.float32(self.lr[name]) * np.float32(1.0 / (1.0 - b1 ** tk))
                out[12 + 2 * k] = np.float32(1.0 / math.sqrt(1.0 - b2 ** tk))
        return out

    def fused_request(self, skip=(), coef_dev=None):
        """The GsStepState of ONE optimizer step (counters advanced as step() would) for gs_backward_step: raw parameter
        rows, both moment buffers, per-row step counts (0 = skipped), learning rates, view statistics.
        coef_dev: device tensor of 11 floats to read the step-dependent constants from (graph replay)."""
        from .capi import GsStepState
        m = self.model
        self.begin_step(skip)
        st = GsStepState()
        if coef_dev is not None:
            st.coef_dev = coef_dev.data_ptr()
        names = ("xyz", "features", "opacity", "scaling", "rotation")
        # (the eighteen row addresses only change when the buffers do: a re-layout, a restore - not every step)
        key = (m.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), m.P)
        ptrs = getattr(self, "_row_ptrs", None)
        if ptrs is None or ptrs[0] != key:
            p, ea, eas = self.field_views(m.flat), self.field_views(self.exp_avg), self.field_views(self.exp_avg_sq)
            ptrs = self._row_ptrs = (key, [(p[n].data_ptr(), ea[n].data_ptr(), eas[n].data_ptr()) for n in names])
        for k, name in enumerate(names):
            pp, pm, pv = ptrs[1][k]
            setattr(st, name, pp)
            st.m[k], st.v[k] = pm, pv
            st.step[k] = 0 if name in skip else (self.seg_steps[name] if self.seg_steps[name] > 0 else self.t)
        for k, name in enumerate(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
            st.lr[k] = self.lr[name]
        st.beta1, st.beta2, st.eps = self.betas[0], self.betas[1], self.eps
        st.max_radii2D, st.xyz_gradient_accum, st.denom = (m.max_radii2D.data_ptr(), m.xyz_gradient_accum.data_ptr(),
                                                           m.denom.data_ptr())
        self._nir_into(st, False)
        if m.with_nir and "nir_albedo" in skip:
            st.step_extra = 0
        if self.USE_DORMANT and m.flat.is_cuda:
            st.dormant = self.dormant_flags().data_ptr()
        st.sparse = 1 if self.sparse else 0
        return st

    def field_views(self, buf):
        P, off, out = self.model.P, 0, {}
        for name, n in self.model.fields:
            out[name] = buf[off:off + P * n].view(P, n)
            off += P * n
        return out


def _stream_of(t):
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _f32(v):
    """A Python float as the kernels' thresholds take it: torch compares fp32 tensors with Python floats by rounding the scalar
    to fp32 ONCE, so the products are formed in double as the host paths form them, then rounded."""
    import ctypes as C
    return C.c_float(v).value


def _split_noise(ns, N, generator, device):
    """The [N ns, 3] normal draws of ns split rows, None without any: ONE draw from `generator` (default: seed 0), on the CPU so
    every rank and every backend sees the same numbers, then moved to `device`."""
    if not ns:
        return None
    if generator is None:
        generator = torch.Generator().manual_seed(0)
    return torch.randn((ns * N, 3), generator=generator, dtype=torch.float32).to(device)


class _FusedActivations(torch.autograd.Function):
    """scales, rotations, opacities = exp(_scaling), normalize(_rotation), sigmoid(_opacity) in one kernel each way
    (gs_activations_fwd / gs_activations_bwd); the backward writes straight into the model's flat gradient buffer
    and hands those views to autograd, so nothing is copied afterwards."""

    @staticmethod
    def forward(ctx, scaling, rotation, opacity, model):
        api = model.optimizer.api
        P = scaling.shape[0]
        scales, rots, opac = torch.empty_like(scaling), torch.empty_like(rotation), torch.empty_like(opacity)
        api.call("activations_fwd", scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(), P, scales.data_ptr(),
                 rots.data_ptr(), opac.data_ptr(), _stream_of(scaling))
        ctx.model = model
        ctx.save_for_backward(scaling, rotation, opacity)
        ctx.set_materialize_grads(False)
        return scales, rots, opac

    @staticmethod
    def backward(ctx, g_s, g_r, g_o):
        if g_s is None and g_r is None and g_o is None:
            # nothing flowed back (the fused train step has already consumed the gradients inside gs_backward_step)
            return None, None, None, None
        scaling, rotation, opacity = ctx.saved_tensors
        model = ctx.model
        P = scaling.shape[0]
        v = model.grad_views()
        g_s = torch.zeros_like(scaling) if g_s is None else g_s.contiguous()
        g_r = torch.zeros_like(rotation) if g_r is None else g_r.contiguous()
        g_o = torch.zeros_like(opacity) if g_o is None else g_o.contiguous()
        model.optimizer.api.call("activations_bwd", scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(), P,
                                 g_s.data_ptr(), g_r.data_ptr(), g_o.data_ptr(), v["scaling"].data_ptr(),
                                 v["rotation"].data_ptr(), v["opacity"].data_ptr(), _stream_of(scaling))
        return v["scaling"], v["rotation"], v["opacity"], None


class GaussianModelLite:
    """Raw (pre-activation) parameters of P Gaussians at max SH degree 3."""

    SPATIAL_ORDER_MIN_P = 100_000

    def __init__(self, scene, device, spatial_lr_scale=1.0, api=None, with_nir=False, spatial_order=None):
        """scene: dict of ACTIVATED tensors as produced by gsplat_amd.synthetic (means3D, scales,
        rotations, opacities, shs[P,16,3]) - converted back to raw form as create_from_pcd would hold them.
        api: C-ABI implementation that provides adam_step (None: torch.optim.Adam on the same flat buffers).
        spatial_order: keep the rows in Morton order of the centres (here, and again after every densification): rows that
        are neighbours in memory are neighbours in space, so whole wavefronts / 256-row blocks are culled, depth-limited
        away, stepped or skipped (FlatAdam.dormant_flags) together.  The model is the same set of Gaussians; only which row
        holds which one differs from the reference's [survivors, clones, split samples] order.  Default (None): on from
        SPATIAL_ORDER_MIN_P = 100 000 Gaussians - below, a step is launch-bound and the row order buys nothing -;
        GS_SPATIAL_ORDER=0 / 1 forces it off / on for models that do not say."""
        if spatial_order is None:
            env = __import__("os").environ.get("GS_SPATIAL_ORDER", "")
            spatial_order = (env == "1") if env in ("0", "1") else int(scene["means3D"].shape[0]) >= self.SPATIAL_ORDER_MIN_P
        self.spatial_order = bool(spatial_order)
        if self.spatial_order:
            from . import synthetic
            scene = synthetic.spatially_ordered(scene)
        P = scene["means3D"].shape[0]
        self.P = P
        self.device = device
        self.spatial_lr_scale = spatial_lr_scale
        self.max_sh_degree = 3
        self.active_sh_degree = scene.get("sh_degree", 3)
        self.percent_dense = 0.01  # arguments/__init__.py:91
        # multispectral variant: one more per-Gaussian parameter (raw NIR albedo, sigmoid-activated) and a global gain
        # (mult-dwtgs/scene/gaussian_model.py:183-186,266-280,408-423).  The reference only creates them in load_ply
        # (SURVEY Q5): here they exist from the start, initialised as its load_ply does - albedo = the DC coefficient
        # it would broadcast (channel 0 is the one its render keeps), gain = 1.
        self.with_nir = bool(with_nir)
        self.fields = FIELDS + ((NIR_FIELD,) if self.with_nir else ())
        self.width = sum(n for _, n in self.fields)
        self.nir_gain = None
        self.exposure = None
        self.exposure_optimizer = None
        self._allocate(P)
        with torch.no_grad():
            self.params["xyz"].copy_(scene["means3D"])
            self.params["features"].copy_(scene["shs"])
            op = scene["opacities"].clamp(1e-6, 1 - 1e-6)
            self.params["opacity"].copy_(torch.log(op / (1 - op)))
            self.params["scaling"].copy_(torch.log(scene["scales"]))
            self.params["rotation"].copy_(scene["rotations"])
            if self.with_nir:
                self.params["nir_albedo"].copy_(scene["shs"][:, 0, 0:1])
        if self.with_nir:
            self.nir_gain = torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float32, device=device))
            self.nir_gain_optimizer = torch.optim.Adam([self.nir_gain], lr=LRS["nir_gain"], eps=1e-15)
            # the moments exist from the start: the fused multispectral step (gs_backward_step_x) updates them in place, the
            # un-fused one goes through torch's optimizer - ONE state for both.  The step count lives with the main
            # optimizer's (FlatAdam.seg_steps["nir_gain"]): the gain steps whenever that one does.
            self.nir_gain_optimizer.state[self.nir_gain] = {
                "step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": torch.zeros_like(self.nir_gain.data),
                "exp_avg_sq": torch.zeros_like(self.nir_gain.data)}
        if api is not None:
            self.optimizer = FlatAdam(api, self)
        else:
            # plain torch Adam on the same storage (used to pin FlatAdam): f_dc / f_rest as strided views
            f = self.params["features"]
            groups = [{"params": [self.params["xyz"]], "lr": LRS["xyz"] * spatial_lr_scale, "name": "xyz"},
                      {"params": [self.params["opacity"]], "lr": LRS["opacity"], "name": "opacity"},
                      {"params": [self.params["scaling"]], "lr": LRS["scaling"], "name": "scaling"},
                      {"params": [self.params["rotation"]], "lr": LRS["rotation"], "name": "rotation"}]
            self.optimizer = _TorchAdamWithFeatureSplit(groups, f, LRS["f_dc"], LRS["f_rest"])
        self.xyz_gradient_accum = torch.zeros((P, 1), device=device)
        self.denom = torch.zeros((P, 1), device=device)
        self.max_radii2D = torch.zeros((P,), device=device)

    def enable_exposure(self, n_cameras):
        """Per-camera exposure (LGDWT-GS/scene/gaussian_model.py:173-176,201: a [n_cams, 3, 4] parameter starting at
        [I | 0] with its own Adam; rate from get_expon_lr_func(0.01, 0.001, delay_steps 0, delay_mult 0) over the
        run, arguments/__init__.py:87-90, set by update_learning_rate).  Used by render(..., use_trained_exp=True).
        A GPU model built with an api gets the device optimizer (optim.ExposureAdam: one launch per step, gated like the
        model's own step, so the fast train step keeps its shape); otherwise torch's."""
        eye = torch.eye(3, 4, device=self.device)[None].repeat(int(n_cameras), 1, 1)
        self.exposure = torch.nn.Parameter(eye.requires_grad_(True))
        if isinstance(self.optimizer, FlatAdam) and self.exposure.is_cuda:
            from .optim import ExposureAdam
            self.exposure_optimizer = ExposureAdam(self.exposure)
        else:
            self.exposure_optimizer = torch.optim.Adam([self.exposure])

    def get_exposure(self, camera_index):
        return self.exposure[camera_index]

    @staticmethod
    def _shapes(P):
        return {"xyz": (P, 3), "features": (P, 16, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4),
                "nir_albedo": (P, 1)}

    def _allocate(self, P):
        """(Re)create the flat parameter / gradient buffers for P Gaussians and the views into them."""
        # every re-allocation (densification, restore, load_ply) gives the model new buffers: whoever froze addresses of the
        # old ones (GraphedStep) compares this counter
        self.generation = getattr(self, "generation", 0) + 1
        self.P = P
        W = self.width
        # parameters and gradients are padded to a multiple of SHARD_UNIT floats so that the flat buffers split into
        # equal, float4-aligned shards for any world size up to 8 (sharded optimizer: reduce-scatter / all-gather
        # run in place on the padded buffers); `flat` / `flat_grad` are the un-padded views everything else uses
        n = P * W
        n_pad = (n + SHARD_UNIT - 1) // SHARD_UNIT * SHARD_UNIT
        self.flat_padded = torch.zeros((n_pad,), dtype=torch.float32, device=self.device)
        self.flat = self.flat_padded[:n]
        # gradient buffer + a [2, P] tail for this step's densification-statistic increments: the data-parallel
        # exchange is then ONE all-reduce (SUM) over gradients and increments together
        # ... and four more floats: word 0 = "some rank's view was invalid" (GsStepState.fail_flag: lists that proved too
        # short under depth limits, or a binning overflow), summed with everything else
        self.exchange = torch.zeros((n_pad + 2 * P + 4,), dtype=torch.float32, device=self.device)
        self.flat_grad = self.exchange[:n]
        self.grad_padded = self.exchange[:n_pad]
        self.stat_delta = self.exchange[n_pad:n_pad + 2 * P].view(2, P)
        self.stat_tail = self.exchange[n_pad:]            # statistics + flag: what travels beside the gradients
        self.fail_flag = self.exchange[n_pad + 2 * P:n_pad + 2 * P + 1]
        self.gain_grad_word = self.exchange[n_pad + 2 * P + 1:n_pad + 2 * P + 2]   # multispectral model: dL/dgain of this view
        # data-parallel step: 1 where this view's gradient row of the Gaussian may be non-zero (sparse exchange)
        self.grad_mask = torch.zeros((P,), dtype=torch.uint8, device=self.device)
        # ... and the union of the ranks' masks, exchanged EARLY (as soon as the forward knows which Gaussians have instances,
        # Trainer._begin_union), with its inclusive prefix - 1 (the packed row of every union member)
        self.union_mask = torch.zeros((P,), dtype=torch.uint8, device=self.device)
        self.union_pos = torch.zeros((P,), dtype=torch.int32, device=self.device)
        # the union as the row masks of gs_adam_step_masked (float, > 0 = stepped): members / everybody else
        self.union_rows_f = torch.zeros((2, P), dtype=torch.float32, device=self.device)
        self.params = {}
        off = 0
        shapes = self._shapes(P)
        for name, n in self.fields:
            view = self.flat[off:off + P * n].view(shapes[name])
            p = torch.nn.Parameter(view, requires_grad=True)
            p.grad = self.flat_grad[off:off + P * n].view(shapes[name])
            self.params[name] = p
            off += P * n

    # ------------------------------------------------------------------ files (formats: gsplat_amd/io.py)
    @classmethod
    def create_from_pcd(cls, points, colors, device, spatial_lr_scale=1.0, api=None, knn=None, spatial_order=None):
        """create_from_pcd (gaussian_model.py:149-176): DC = RGB2SH(colour), rest 0, scale = sqrt of the mean squared
        distance to the 3 nearest neighbours (clamped at 1e-7) on all axes, identity rotation, opacity 0.1, active
        SH degree 0.  knn: callable [P,3] -> [P] (simple_knn's distCUDA2); default = the float64 brute force."""
        from . import synthetic
        pts = torch.as_tensor(points, dtype=torch.float32)
        col = torch.as_tensor(colors, dtype=torch.float32)
        P = pts.shape[0]
        dist2 = (knn(pts) if knn is not None else synthetic.brute_force_knn_dist2(pts)).clamp_min(1e-7).cpu()
        shs = torch.zeros((P, 16, 3))
        shs[:, 0, :] = synthetic.rgb2sh(col)
        scene = dict(means3D=pts, shs=shs, scales=torch.sqrt(dist2)[:, None].repeat(1, 3),
                     rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1), opacities=torch.full((P, 1), 0.1),
                     sh_degree=0)
        return cls(scene, device, spatial_lr_scale=spatial_lr_scale, api=api, spatial_order=spatial_order)

    def save_ply(self, path):
        """save_ply (gaussian_model.py:240-256): raw parameters, the reference's 62-property layout."""
        from . import io as gio
        p = {k: v.detach().cpu().numpy() for k, v in self.params.items()}
        extra = {"nir_albedo": p["nir_albedo"]} if self.with_nir else None
        gio.save_gaussians_ply(path, p["xyz"], p["features"], p["opacity"], p["scaling"], p["rotation"], extra=extra)

    def load_ply(self, path):
        """load_ply (gaussian_model.py:263-314): replaces the parameters (fresh Adam state), active degree = max."""
        from . import io as gio
        d = gio.load_gaussians_ply(path, self.max_sh_degree)
        api = getattr(self.optimizer, "api", None)
        self._allocate(d["xyz"].shape[0])
        if self.with_nir and "nir_albedo" not in d:
            # mult-dwtgs/scene/gaussian_model.py:417-421: no NIR property in the file -> start from the DC coefficient
            d["nir_albedo"] = d["features"][:, 0, 0:1].copy()
        with torch.no_grad():
            for name in self.params:
                self.params[name].copy_(torch.from_numpy(d[name]).reshape(self.params[name].shape))
        if api is not None:
            self.optimizer = FlatAdam(api, self)
        self.xyz_gradient_accum = torch.zeros((self.P, 1), device=self.device)
        self.denom = torch.zeros((self.P, 1), device=self.device)
        self.max_radii2D = torch.zeros((self.P,), device=self.device)
        self.active_sh_degree = self.max_sh_degree

    def capture(self):
        """Checkpoint payload (the role of GaussianModel.capture, gaussian_model.py:62-76): flat parameters, Adam
        moments and step counts, densification statistics.  A model that is being trained is checkpointed through
        Trainer.checkpoint(), which first settles a pending depth-limit verdict and gathers sharded Adam moments."""
        opt = self.optimizer
        return dict(P=self.P, active_sh_degree=self.active_sh_degree, flat=self.flat.detach().cpu().clone(),
                    exp_avg=opt.exp_avg.cpu().clone(), exp_avg_sq=opt.exp_avg_sq.cpu().clone(), t=opt.t,
                    seg_steps=dict(opt.seg_steps), lr=dict(opt.lr), xyz_gradient_accum=self.xyz_gradient_accum.cpu().clone(),
                    denom=self.denom.cpu().clone(), max_radii2D=self.max_radii2D.cpu().clone(),
                    spatial_lr_scale=self.spatial_lr_scale,
                    nir_gain=None if self.nir_gain is None else self.nir_gain.detach().cpu().clone(),
                    nir_gain_optimizer=None if self.nir_gain is None else self.nir_gain_optimizer.state_dict())

    def restore(self, state):
        opt = self.optimizer
        self._allocate(int(state["P"]))
        with torch.no_grad():
            self.flat.copy_(state["flat"])
        opt.alloc_moments()
        opt.exp_avg.copy_(state["exp_avg"])
        opt.exp_avg_sq.copy_(state["exp_avg_sq"])
        opt.t, opt.seg_steps, opt.lr = int(state["t"]), dict(state["seg_steps"]), dict(state["lr"])
        self.active_sh_degree = int(state["active_sh_degree"])
        self.xyz_gradient_accum = state["xyz_gradient_accum"].to(self.device).clone()
        self.denom = state["denom"].to(self.device).clone()
        self.max_radii2D = state["max_radii2D"].to(self.device).clone()
        self.spatial_lr_scale = state["spatial_lr_scale"]
        if self.nir_gain is not None and state.get("nir_gain") is not None:
            with torch.no_grad():
                self.nir_gain.copy_(state["nir_gain"])
            self.nir_gain_optimizer.load_state_dict(state["nir_gain_optimizer"])
        if self.with_nir and "nir_gain" not in opt.seg_steps:
            # a checkpoint from before the gain's step count moved into seg_steps: it lived in the gain optimizer's own state
            try:
                opt.seg_steps["nir_gain"] = int(state["nir_gain_optimizer"]["state"][0]["step"])
            except (KeyError, IndexError, TypeError):
                opt.seg_steps["nir_gain"] = int(state["t"])

    def oneupSHdegree(self):
        """gaussian_model.py:145-147"""
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ------------------------------------------------------------------ densification
    def _relayout(self, src_idx, new_rows):
        """New model = rows `src_idx` of the current one (parameters AND Adam moments kept) followed by
        `new_rows` (dict field -> [n_new, width], moments zero): the flat-buffer form of _prune_optimizer +
        cat_tensors_to_optimizer (gaussian_model.py:331-393)."""
        opt = self.optimizer
        if not isinstance(opt, FlatAdam):
            raise NotImplementedError("densification needs the flat Adam state")
        old_p = {name: self.params[name].detach().reshape(self.P, n) for name, n in self.fields}
        old_m, old_v = opt.field_views(opt.exp_avg), opt.field_views(opt.exp_avg_sq)
        n_new = next(iter(new_rows.values())).shape[0] if new_rows else 0
        P2 = int(src_idx.numel()) + n_new
        cat_p, cat_m, cat_v = {}, {}, {}
        for name, n in self.fields:
            add = new_rows[name].reshape(n_new, n) if n_new else old_p[name][:0]
            cat_p[name] = torch.cat((old_p[name][src_idx], add), dim=0)
            z = torch.zeros_like(add)
            cat_m[name] = torch.cat((old_m[name][src_idx], z), dim=0)
            cat_v[name] = torch.cat((old_v[name][src_idx], z), dim=0)
        self._allocate(P2)
        opt.alloc_moments()
        new_m, new_v = opt.field_views(opt.exp_avg), opt.field_views(opt.exp_avg_sq)
        with torch.no_grad():
            for name, n in self.fields:
                self.params[name].reshape(P2, n).copy_(cat_p[name])
                new_m[name].copy_(cat_m[name])
                new_v[name].copy_(cat_v[name])
        for p in self.params.values():  # replaced tensors have no gradient until the next backward
            p.grad = None

    @staticmethod
    def build_rotation(r):
        """general_utils.py:78-99 (quaternion normalised here, unlike the rasterizer)."""
        q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=1)
        return R.view(-1, 3, 3)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, radii=None, generator=None, N=2,
                          decisions=None, on_device=False):
        """gaussian_model.py:395-467 in one re-layout: clone small Gaussians with a large view-space gradient,
        split large ones into N samples of their own distribution (scale / (0.8 N)), drop the split originals,
        then prune by opacity / world size.  Row order = the reference's: [survivors, clones, split samples].
        `generator`: CPU generator for the split samples (drawn on the CPU so every rank and every backend
        sees the same numbers).  Returns (n_clone, n_split, n_pruned).
        Note: the reference zeroes max_radii2D inside densification_postfix (:383) BEFORE the screen-size test of
        :458 reads it, so that test never fires; reproduced by construction.
        `decisions` (parity instrument, normally None): a dict.  Without the key "replay" the three DISCRETE decisions of this
        call - the clone mask, the split mask (both [P]) and the prune mask (over [survivors, clones, samples]) - are
        recorded into it (CPU bool tensors, plus the statistic `g` and the threshold they were taken with).  With
        decisions["replay"] = such a record, the recorded masks are USED instead of this model's own, and what this model
        would have decided is reported beside them (decisions["own"], decisions["disagree"]): two implementations whose
        statistics differ in the last bits take the same discrete trajectory, which separates threshold chaos from
        arithmetic differences (tests/test_gpu_psnr_parity.py).
        `on_device` (default off): the same result from HIP kernels (csrc/gs_densify.hip, _densify_on_device) - the decisions
        taken per row on the device, ONE host read-back (the counts that size the new buffers and the noise; the upload of the
        CPU-drawn noise is the only other host wait), one gather pass
        that writes parameters and moments in their final order, Morton order included.  Needs a GPU model with the flat Adam
        state; copied values are the host path's bit for bit, the split samples' centres and scales agree to the last bits
        (tests/test_gpu_densify_device.py).  With `decisions`, or when every row is pruned, the host path runs."""
        if on_device:
            self._require_device_form("densify_and_prune", "densify_plan")
            if decisions is None:
                out = self._densify_on_device(max_grad, min_opacity, extent, max_screen_size, generator, N)
                if out is not None:
                    return out
        return self._clone_split_prune(max_grad, min_opacity, extent, bool(max_screen_size), None, generator, N, decisions)

    def _clone_split_prune(self, max_grad, min_opacity, extent, world_size_prune, gate_opacity, generator, N, decisions=None):
        """The host body of densify_and_prune and, with its two parameters, of densify_and_prune_dng: world_size_prune - the
        final prune's max scale > 0.1 * extent term (DNGaussian has none); gate_opacity - not None: clone and split also need
        sigmoid(opacity) > gate_opacity (DNGaussian's opa_thresh).  Returns (n_clone, n_split, n_pruned)."""
        with torch.no_grad():
            P0 = self.P
            grads = self.xyz_gradient_accum / self.denom
            grads[grads.isnan()] = 0.0
            g = grads.reshape(P0)
            scaling = self.get_scaling
            max_scale = scaling.max(dim=1).values
            small = max_scale <= self.percent_dense * extent
            clone = (g.abs() >= max_grad) & small        # torch.norm over the single column (:435)
            split = (g >= max_grad) & ~small             # padded_grad of the clones is 0: never selected (:399-402)
            if gate_opacity is not None:
                gate = self.get_opacity.squeeze(1) > gate_opacity
                clone, split = clone & gate, split & gate
            replay = decisions.get("replay") if decisions is not None else None
            if decisions is not None:
                own = dict(clone=clone.cpu(), split=split.cpu(), g=g.detach().cpu().clone(), max_grad=float(max_grad),
                           max_scale=max_scale.detach().cpu().clone(), scale_bound=float(self.percent_dense * extent))
                if replay is None:
                    decisions.update(own)
                else:
                    decisions["own"] = own
                    clone, split = replay["clone"].to(clone.device), replay["split"].to(split.device)
            ci = clone.nonzero().squeeze(1)
            si = split.nonzero().squeeze(1)
            ns = int(si.numel())
            raw = {name: self.params[name].detach().reshape(P0, n) for name, n in self.fields}
            new = {name: [raw[name][ci]] for name, _ in self.fields}
            if ns:
                new_xyz, new_scaling = self._split_samples(raw["xyz"][si], scaling[si], raw["rotation"][si], N, generator)
                new["xyz"].append(new_xyz)
                new["scaling"].append(new_scaling)
                for name, _ in self.fields:
                    if name not in ("xyz", "scaling"):
                        new[name].append(raw[name][si].repeat(N, 1))
            new = {name: torch.cat(v, dim=0) for name, v in new.items()}
            # final prune (:455-462) evaluated on [survivors, clones, samples]
            keep_old = ~split
            op_all = torch.cat((torch.sigmoid(raw["opacity"][keep_old]), torch.sigmoid(new["opacity"])), dim=0).squeeze(1)
            prune = op_all < min_opacity
            if world_size_prune:
                sc_all = torch.cat((max_scale[keep_old], torch.exp(new["scaling"]).max(dim=1).values), dim=0)
                prune = prune | (sc_all > 0.1 * extent)  # big_points_vs is all-False (max_radii2D was just zeroed)
            if decisions is not None:
                if replay is None:
                    decisions["prune"] = prune.cpu()
                    decisions["opacity"] = op_all.cpu()
                else:
                    decisions["own"]["prune"], decisions["own"]["opacity"] = prune.cpu(), op_all.cpu()
                    prune = replay["prune"].to(prune.device)
                    o = decisions["own"]
                    decisions["disagree"] = dict(clone=int((o["clone"] != replay["clone"]).sum()),
                                                 split=int((o["split"] != replay["split"]).sum()),
                                                 prune=int((o["prune"] != replay["prune"]).sum()))
            n_keep_old = int(keep_old.sum())
            src = keep_old.nonzero().squeeze(1)[~prune[:n_keep_old]]
            keep_new = ~prune[n_keep_old:]
            self._relayout(src, {name: v[keep_new] for name, v in new.items()})
            self._restore_order_and_zero_statistics()
            return int(ci.numel()), ns, int(prune.sum())

    def _split_samples(self, xyz, scales, rotation, N, generator):
        """The N samples of each of the ns selected rows (their centres, ACTIVATED scales and raw rotations), drawn from the
        row's own distribution (gaussian_model.py:404-412): centres R (noise * scale) + xyz and raw scaling log(scale / (0.8 N)),
        both [N ns, 3] in the reference's repeat(N, 1) order.  One draw from the generator (_split_noise); ns > 0."""
        stds = scales.repeat(N, 1)
        samples = _split_noise(scales.shape[0], N, generator, stds.device) * stds
        rots = self.build_rotation(rotation).repeat(N, 1, 1)
        return torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + xyz.repeat(N, 1), torch.log(stds / (0.8 * N))

    def _zero_statistics(self):
        self.xyz_gradient_accum = torch.zeros((self.P, 1), device=self.device)
        self.denom = torch.zeros((self.P, 1), device=self.device)
        self.max_radii2D = torch.zeros((self.P,), device=self.device)

    def _restore_order_and_zero_statistics(self):
        """The tail of every host rule: under spatial_order the new rows go where their neighbours are (an empty model has no
        order to restore), then the statistics are zeroed at the new size (densification_postfix)."""
        if getattr(self, "spatial_order", False) and self.P > 0:
            from . import synthetic
            self._relayout(synthetic.morton_order(self.params["xyz"]), {})
        self._zero_statistics()

    def _densify_on_device(self, max_grad, min_opacity, extent, max_screen_size, generator, N, gate_opacity=None):
        """densify_and_prune from the kernels of csrc/gs_densify.hip (include/gsplat.h: gs_densify_plan / emit / gather,
        gs_morton_codes).  Returns (n_clone, n_split, n_pruned), or None - nothing written, the generator untouched - when every
        row would be pruned (the caller then takes the host path).  gate_opacity (DNGaussian's rule, _densify_dng_on_device):
        the plan is gs_densify_plan_gated's; everything behind it is unchanged."""
        opt = self.optimizer
        api, dev, P0 = opt.api, self.flat.device, self.P
        stream = _stream_of(self.flat)
        with torch.no_grad():
            raw = {name: self.params[name].detach() for name, _ in self.fields}
            accum, denom = self._statistics_for_device()
            sample_div = _f32(0.8 * N)
            nbytes = api.raw("densify_tmp_bytes")(P0)
            tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            plan = [raw["scaling"].data_ptr(), raw["opacity"].data_ptr(), accum.data_ptr(), denom.data_ptr(), P0, N, _f32(max_grad),
                    _f32(self.percent_dense * extent), _f32(min_opacity), _f32(0.1 * extent), sample_div,
                    1 if max_screen_size else 0]
            if gate_opacity is None:
                api.call("densify_plan", *plan, tmp.data_ptr(), nbytes, stream)
            else:
                api.call("densify_plan_gated", *plan, _f32(gate_opacity), tmp.data_ptr(), nbytes, stream)
            # the ONE read-back: the counts size the new buffers and the noise (whose upload below blocks too, when rows split)
            n_keep, n_clone_keep, ns, ns_keep, n_clone = tmp[:20].view(torch.int32).cpu().tolist()
            P2 = n_keep + n_clone_keep + N * ns_keep
            if P2 == 0:
                return None
            noise = _split_noise(ns, N, generator, dev)
            table = torch.empty((P2,), dtype=torch.int32, device=dev)
            new_xyz = torch.empty((P2, 3), dtype=torch.float32, device=dev)
            api.call("densify_emit", tmp.data_ptr(), nbytes, raw["xyz"].data_ptr(), raw["scaling"].data_ptr(),
                     raw["rotation"].data_ptr(), None if noise is None else noise.data_ptr(), P0, N, n_keep, n_clone_keep, ns,
                     ns_keep, P2, table.data_ptr(), new_xyz.data_ptr(), stream)
            perm = self._morton_perm_on_device(new_xyz, stream)
            self._gather_on_device("densify_gather", (perm, table, new_xyz), P2, sample_div, stream)
            self._zero_statistics()
            return n_clone, ns, (P0 - ns - n_keep) + (n_clone - n_clone_keep) + N * (ns - ns_keep)

    # ---- what the three device forms (_densify_on_device, _prune_on_device, _densify_fsgs_on_device) share
    def _statistics_for_device(self, with_radii=False):
        """xyz_gradient_accum and denom (and max_radii2D) as the kernels read them: contiguous fp32 of P elements on the model's
        device."""
        stats = [self.xyz_gradient_accum.contiguous(), self.denom.contiguous()]
        if with_radii:
            stats.append(self.max_radii2D.contiguous())
        if any(t.numel() != self.P or t.dtype != torch.float32 or t.device != self.flat.device for t in stats):
            raise RuntimeError("densification statistics do not match the model")
        return stats

    def _morton_perm_on_device(self, new_xyz, stream):
        """synthetic.morton_order of the new centres (gs_morton_codes, a stable sort), no read-back; None without spatial_order."""
        if not getattr(self, "spatial_order", False):
            return None
        P2 = new_xyz.shape[0]
        lo, hi = torch.aminmax(new_xyz, dim=0)
        codes = torch.empty((P2,), dtype=torch.int32, device=new_xyz.device)
        self.optimizer.api.call("morton_codes", new_xyz.data_ptr(), P2, lo.data_ptr(), hi.data_ptr(), codes.data_ptr(), stream)
        return torch.sort(codes, stable=True).indices

    def _gather_on_device(self, entry, lead, P2, sample_div, stream, extra_fields=()):
        """The one HBM pass of a device re-layout: new buffers of P2 rows, filled by the gather `entry` ("densify_gather" or
        "densify_fsgs_gather") from the old ones.  lead: the entry's leading tensors (perm or None, table, [nb_kind,] new_xyz);
        extra_fields: the fields the entry is told of behind xyz and scaling.  Every p.grad is None afterwards."""
        import ctypes as C
        opt, P0 = self.optimizer, self.P
        old_flat, old_m, old_v = self.flat, opt.exp_avg, opt.exp_avg_sq   # (alive until the gather has been enqueued)
        names = [name for name, _ in self.fields]
        widths = (C.c_int32 * len(names))(*[n for _, n in self.fields])
        self._allocate(P2)
        opt.alloc_moments()
        opt.api.call(entry, *[None if t is None else t.data_ptr() for t in lead], P2, old_flat.data_ptr(), old_m.data_ptr(),
                     old_v.data_ptr(), P0, self.flat.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), len(names), widths,
                     *[names.index(n) for n in ("xyz", "scaling") + tuple(extra_fields)], sample_div, stream)
        for p in self.params.values():  # replaced tensors have no gradient until the next backward
            p.grad = None

    # ------------------------------------------------------------------ DNGaussian: mask prunes and its densification rule
    def _require_device_form(self, what, entry):
        api = getattr(self.optimizer, "api", None)
        if not (self.flat.is_cuda and isinstance(self.optimizer, FlatAdam) and hasattr(api, "_" + entry)):
            raise RuntimeError("%s(on_device=True) needs a GPU model built with the HIP api (flat Adam state); "
                               "there is no fallback" % what)

    def prune_points(self, mask, on_device=False):
        """DNGaussian/scene/gaussian_model.py:374-392: remove the rows whose mask entry is nonzero (bool or uint8, [P] or
        [P,1]).  The new model is the rows that stay, in their old relative order (a subsequence of spatially ordered rows is
        ordered: nothing is re-sorted); parameters and both Adam moments are copied bit for bit (_prune_optimizer), and
        xyz_gradient_accum, denom and max_radii2D are INDEXED, not zeroed (:387-392) - a prune between two densifications keeps
        what the views since the last one have accumulated.  Step counts stay, every p.grad is None afterwards, the dormant
        flags are recomputed.  The multispectral model's NIR field is one more copied field.  Returns the number of rows removed;
        an all-false mask returns 0 and touches nothing (`generation` does not move).
        `on_device`: the same model from gs_prune_plan / gs_prune_emit and the gather of the densification
        (csrc/gs_densify.hip), ONE host read-back (the number of rows kept, which sizes the new buffers) where the host path
        has the nonzero() of its boolean index.  Needs a GPU model with the flat Adam state (RuntimeError otherwise); when every
        row goes, the host path runs."""
        if on_device:
            self._require_device_form("prune_points", "prune_plan")
        P0 = self.P
        mask = torch.as_tensor(mask)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("prune_points: the mask must be bool or uint8, got %s" % mask.dtype)
        if tuple(mask.shape) not in ((P0,), (P0, 1)):
            raise ValueError("prune_points: the mask must be [P] or [P,1] with P = %d, got shape %s" % (P0, tuple(mask.shape)))
        if not isinstance(self.optimizer, FlatAdam):
            raise NotImplementedError("prune_points needs the flat Adam state")
        with torch.no_grad():
            mask = mask.reshape(P0).to(self.flat.device)
            remove = mask if mask.dtype == torch.bool else mask != 0
            if on_device and P0 > 0:
                out = self._prune_on_device(remove)
                if out is not None:
                    return out
            src = (~remove).nonzero().squeeze(1)
            n_removed = P0 - int(src.numel())
            if n_removed == 0:
                return 0
            accum, denom, radii = self.xyz_gradient_accum[src], self.denom[src], self.max_radii2D[src]
            self._relayout(src, {})
            self.xyz_gradient_accum, self.denom, self.max_radii2D = accum, denom, radii
            return n_removed

    def _prune_on_device(self, remove):
        """prune_points from gs_prune_plan / gs_prune_emit / gs_densify_gather.  `remove`: bool [P] on the model's device.
        Returns the number of rows removed, or None - nothing written - when every row would go."""
        api, dev, P0 = self.optimizer.api, self.flat.device, self.P
        stream = _stream_of(self.flat)
        remove = remove.contiguous()
        stats = self._statistics_for_device(with_radii=True)
        nbytes = api.raw("prune_tmp_bytes")(P0)
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        api.call("prune_plan", remove.data_ptr(), P0, tmp.data_ptr(), nbytes, stream)
        P2 = int(tmp[:4].view(torch.int32).cpu())   # the ONE read-back: the number of rows kept sizes the new buffers
        if P2 == 0:
            return None
        if P2 == P0:
            return 0
        table = torch.empty((P2,), dtype=torch.int32, device=dev)
        new_xyz = torch.empty((P2, 3), dtype=torch.float32, device=dev)
        new_stats = [torch.empty((P2, 1), device=dev), torch.empty((P2, 1), device=dev), torch.empty((P2,), device=dev)]
        api.call("prune_emit", tmp.data_ptr(), nbytes, remove.data_ptr(), self.params["xyz"].detach().data_ptr(), P0, P2,
                 table.data_ptr(), new_xyz.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                 new_stats[0].data_ptr(), new_stats[1].data_ptr(), new_stats[2].data_ptr(), stream)
        # every row is a survivor, in its old order: no permutation, and no sample, so the gather's sample_div is never read
        self._gather_on_device("densify_gather", (None, table, new_xyz), P2, 1.0, stream)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = new_stats
        return P0 - P2

    def prune(self, min_opacity, on_device=False):
        """DNGaussian/scene/gaussian_model.py:536-538: prune_points(sigmoid(opacity) < min_opacity).  The mask is formed on the
        model's device with no read-back; the prune's count is the only one.  Returns the number of rows removed."""
        with torch.no_grad():
            mask = (self.get_opacity < min_opacity).squeeze(1)
        return self.prune_points(mask, on_device=on_device)

    def densify_and_prune_dng(self, max_grad, min_opacity, extent, max_screen_size, opa_thresh, max_dist=None, generator=None,
                              N=2, on_device=False):
        """DNGaussian's densify_and_prune (DNGaussian/scene/gaussian_model.py:454-524), the reference's statements in the
        reference's order - the 3DGS rule of densify_and_prune with three differences:
          outliers  if max_dist is not None (a float, or a tensor of P elements): rows with sqrt(distCUDA2(xyz)) > max_dist are
                    removed FIRST, through prune_points - so the statistics the selection reads are those of the rows that stay;
          gate      clone (|g| >= max_grad, max scale <= percent_dense * extent) and split (g >= max_grad, larger) both ALSO
                    need sigmoid(opacity) > opa_thresh; a clone is never split; samples use scale / (0.8 N);
          prune     sigmoid(opacity) < min_opacity ONLY: the reference's max_screen_size branch reads max_radii2D, which
                    densification_postfix has just zeroed, so it never fires (as in densify_and_prune) and there is no world-size
                    rule beside it.  Reproduced by construction: max_screen_size is accepted and not read.
        Then the statistics are zeroed at the new size.  Selection, split and final prune are ONE re-layout
        ([survivors | clones | sample blocks], then the Morton order under spatial_order) where the reference re-creates the
        optimizer state four times; the outlier prune in front is a second one.  Noise: CPU randn from `generator` times the stds,
        as densify_and_prune draws it.  Returns (n_outliers, n_clone, n_split, n_pruned); n_pruned counts the final prune.
        `on_device`: the same model from HIP kernels - gs_densify_plan_gated, then gs_densify_emit / gs_morton_codes /
        gs_densify_gather unchanged: one count read-back, the noise upload the only other wait.  max_dist composes
        gs_knn_mean_dist2, torch's sqrt and compare on the device and prune_points(on_device=True) (one more read-back).  Needs a
        GPU model with the flat Adam state (RuntimeError otherwise); when every row would be pruned the host path runs."""
        if on_device:
            self._require_device_form("densify_and_prune_dng", "densify_plan_gated")
        n_outliers = 0
        if max_dist is not None:
            from .knn import dist2
            with torch.no_grad():
                dist = torch.sqrt(dist2(self.optimizer.api, self.params["xyz"].detach()))
                if torch.is_tensor(max_dist):
                    if max_dist.numel() != self.P:
                        raise ValueError("densify_and_prune_dng: max_dist must be a number or hold P = %d elements" % self.P)
                    max_dist = max_dist.reshape(self.P).to(dist.device)
                outliers = dist > max_dist
            n_outliers = self.prune_points(outliers, on_device=on_device)
        if on_device and self.P > 0:
            out = self._densify_dng_on_device(max_grad, min_opacity, extent, opa_thresh, generator, N)
            if out is not None:
                return (n_outliers,) + out
        # the final prune (:518-523) is opacity only: no world-size term, whatever max_screen_size is
        return (n_outliers,) + self._clone_split_prune(max_grad, min_opacity, extent, False, opa_thresh, generator, N)

    def _densify_dng_on_device(self, max_grad, min_opacity, extent, opa_thresh, generator, N):
        """Steps 2-6 of densify_and_prune_dng from the kernels: _densify_on_device with the gated plan and no size test.
        Returns (n_clone, n_split, n_pruned), or None when every row would be pruned."""
        return self._densify_on_device(max_grad, min_opacity, extent, None, generator, N, gate_opacity=opa_thresh)

    def proximity(self, extent, api=None):
        """FSGS's proximity-guided unpooling (FSGS/scene/gaussian_model.py:405-420, N = 3), the reference's tensor
        expressions one for one: a Gaussian is selected if its mean SQUARED distance to its three nearest neighbours
        exceeds 5 * extent (a length - the reference compares the two as they are) and its largest activated scale exceeds
        extent; every selected Gaussian adds three: raw scaling and raw opacity of the neighbour, rotation (1, 0, 0, 0), zero
        SH.  New row j takes neighbour j of the flattened [S, 3] neighbour lists (selected Gaussian j // 3, nearest first) and
        lies midway between that neighbour and selected Gaussian j % S: the reference's `_xyz[mask].repeat(1, N, 1)` TILES the
        S selected rows, it does not repeat each three times, so only with S = 1 is every new Gaussian between a Gaussian
        and its own neighbour.  Reproduced as written.
        The new rows follow the existing ones (whose parameters and Adam moments stay, new moments are zero), the statistics
        are zeroed at the new size (densification_postfix) and the spatial order is restored as densify_and_prune does.
        api: whose kNN to use (default: the optimizer's).  Returns the number of new rows."""
        if self.with_nir:
            raise NotImplementedError("proximity: the multispectral model has no rule for the new rows' NIR albedo")
        with torch.no_grad():
            P0 = self.P
            raw = {name: self.params[name].detach().reshape(P0, n) for name, n in self.fields}
            new = self._proximity_rows(raw, extent, api or self.optimizer.api)
            self._relayout(torch.arange(P0, device=raw["xyz"].device), new)
            self._restore_order_and_zero_statistics()
            return int(new["xyz"].shape[0])

    @staticmethod
    def _proximity_rows(rows, extent, knn_api):
        """The rows proximity()'s rule adds to the set `rows` (field -> [n, w], raw values), as proximity()'s docstring states it,
        the tiled repeat(1, 3, 1) of the selected centres as the reference writes it: field -> [3 S, w]."""
        from .knn import dist2_with_indices
        dist, nearest = dist2_with_indices(knn_api, rows["xyz"])
        sel = torch.logical_and(dist > (5. * extent), torch.max(torch.exp(rows["scaling"]), dim=1).values > extent)
        new_idx = nearest[sel].reshape(-1).long()
        source_xyz = rows["xyz"][sel].repeat(1, 3, 1).reshape(-1, 3)
        new = {"xyz": (source_xyz + rows["xyz"][new_idx]) / 2, "scaling": rows["scaling"][new_idx],
               "opacity": rows["opacity"][new_idx], "features": torch.zeros_like(rows["features"][new_idx])}
        new["rotation"] = torch.zeros_like(rows["rotation"][new_idx])
        new["rotation"][:, 0] = 1
        return new

    def densify_and_prune_fsgs(self, max_grad, min_opacity, extent, max_screen_size, iteration, dist_thres=10.0,
                               prune_from_iter=500, proximity_until_iter=2000, generator=None, N=2, api=None, on_device=False):
        """FSGS's own densify_and_prune (FSGS/scene/gaussian_model.py:424-491), the reference's statements in the reference's
        order - it is NOT the 3DGS rule of densify_and_prune:
          clone     |g| >= max_grad and max scale <= percent_dense * extent; the clones are appended (moments zero);
          split     over the P0 + n_clone rows: (padded g >= max_grad and max scale > percent_dense * extent) OR
                    (dist > dist_thres * extent and max scale > extent), dist = mean squared 3-NN distance of THAT point set;
                    N samples per selected row are appended (noise from the CPU `generator`, build_rotation, scale / (0.8 N));
                    the selected originals are removed only if iteration > prune_from_iter;
          proximity if iteration < proximity_until_iter: the rule of proximity() on the set as it then stands (its kNN sees
                    the split samples), tiling quirk included (see proximity's docstring);
          prune     sigmoid(opacity) < min_opacity, with a truthy max_screen_size also max scale > 0.1 * extent (the screen
                    rule never fires: max_radii2D has just been zeroed, as in densify_and_prune) - applied only if
                    iteration > prune_from_iter.  FSGS/train.py:166 always passes max_screen_size = None, and its
                    opacity threshold is prune_threshold.
        Afterwards the Morton order is restored when spatial_order is set and the statistics are zeroed at the new size.
        kNN: gsplat_amd.knn.dist2_with_indices(api or self.optimizer.api, ...).  The reference's `confidence` tensor (ones
        for every new row, pruned with the rest, never read by the densification) has no counterpart on this model.
        The whole call is ONE re-layout of parameters and moments (plus the Morton one).
        Returns (n_clone, n_split, n_proximity, n_pruned); n_pruned counts the split originals removed and the final prune.
        `on_device`: the same model from HIP kernels (csrc/gs_densify.hip: gs_densify_fsgs_*, _densify_fsgs_on_device) -
        THREE host read-backs (the clone count in front of kNN #1, the split / keep counts in front of the noise and kNN #2,
        the proximity counts that size the final buffers; two without proximity) plus the upload of the CPU-drawn noise, and one
        gather pass; CPU-drawn noise and no atomics, so every data-parallel rank derives the same model, as with the 3DGS
        form.  Needs a GPU model with the flat Adam state (RuntimeError otherwise).  When a kNN stage would hold
        fewer than 4 points, every row would be pruned or percent_dense > 1, the host path runs."""
        if self.with_nir:
            raise NotImplementedError("densify_and_prune_fsgs: the multispectral model has no rule for the new rows' NIR albedo")
        if on_device:
            self._require_device_form("densify_and_prune_fsgs", "densify_fsgs_plan")
            out = self._densify_fsgs_on_device(max_grad, min_opacity, extent, max_screen_size, iteration, dist_thres,
                                               prune_from_iter, proximity_until_iter, generator, N)
            if out is not None:
                return out
        from .knn import dist2_with_indices
        knn_api = api or self.optimizer.api
        with torch.no_grad():
            P0 = self.P
            grads = self.xyz_gradient_accum / self.denom
            grads[grads.isnan()] = 0.0
            g = grads.reshape(P0)
            dev = self.flat.device
            cur = {name: self.params[name].detach().reshape(P0, n) for name, n in self.fields}
            origin = torch.arange(P0, device=dev)      # the model's row a current row came from, -1 for an appended one
            pruning = iteration > prune_from_iter      # prune_points (:335-336)
            n_pruned = 0

            def append(cur, origin, new):
                n_new = new["xyz"].shape[0]
                cur = {name: torch.cat((cur[name], new[name]), dim=0) for name in cur}
                return cur, torch.cat((origin, torch.full((n_new,), -1, dtype=origin.dtype, device=dev)))

            # densify_and_clone (:457-472)
            max_scale = torch.exp(cur["scaling"]).max(dim=1).values
            clone = (g.abs() >= max_grad) & (max_scale <= self.percent_dense * extent)
            n_clone = int(clone.sum())
            cur, origin = append(cur, origin, {name: v[clone] for name, v in cur.items()})
            # densify_and_split (:424-454) on the P0 + n_clone rows
            n1 = P0 + n_clone
            padded = torch.zeros((n1,), device=dev)
            padded[:P0] = g
            act = torch.exp(cur["scaling"])
            max_scale = act.max(dim=1).values
            split = (padded >= max_grad) & (max_scale > self.percent_dense * extent)
            dist, _ = dist2_with_indices(knn_api, cur["xyz"])
            split = split | ((dist > dist_thres * extent) & (max_scale > extent))
            ns = int(split.sum())
            if ns:
                new = {name: v[split].repeat(N, 1) for name, v in cur.items()}
                new["xyz"], new["scaling"] = self._split_samples(cur["xyz"][split], act[split], cur["rotation"][split], N, generator)
                cur, origin = append(cur, origin, new)
                if pruning:
                    keep = ~torch.cat((split, torch.zeros((N * ns,), dtype=torch.bool, device=dev)))
                    cur, origin = {name: v[keep] for name, v in cur.items()}, origin[keep]
                    n_pruned += ns
            # proximity (:405-420) on the set as it stands
            n_prox = 0
            if iteration < proximity_until_iter:
                new = self._proximity_rows(cur, extent, knn_api)
                n_prox = int(new["xyz"].shape[0])
                cur, origin = append(cur, origin, new)
            # the final prune (:484-490)
            prune = (torch.sigmoid(cur["opacity"]) < min_opacity).squeeze(1)
            if max_screen_size:
                prune = prune | (torch.exp(cur["scaling"]).max(dim=1).values > 0.1 * extent)   # (big_points_vs is all-False)
            if pruning:
                keep = ~prune
                cur, origin = {name: v[keep] for name, v in cur.items()}, origin[keep]
                n_pruned += int(prune.sum())
            old = origin >= 0     # rows of the model come first, in their order: nothing above reorders
            self._relayout(origin[old], {name: v[~old] for name, v in cur.items()})
            self._restore_order_and_zero_statistics()
            return n_clone, ns, n_prox, n_pruned

    def _densify_fsgs_on_device(self, max_grad, min_opacity, extent, max_screen_size, iteration, dist_thres, prune_from_iter,
                                proximity_until_iter, generator, N):
        """densify_and_prune_fsgs from the kernels of csrc/gs_densify.hip (include/gsplat.h: gs_densify_fsgs_*), the two kNN
        searches from gs_knn_mean_dist2_idx.  Three read-backs (two without proximity), each one small copy.  Returns the
        4-tuple, or None - nothing written, the generator untouched - when a kNN stage would hold fewer than 4 points, every row
        would be pruned or percent_dense > 1 (a clone could then be split); the caller takes the host path."""
        if self.percent_dense > 1:
            return None
        api, dev, P0 = self.optimizer.api, self.flat.device, self.P
        if P0 < 1:
            return None
        stream = _stream_of(self.flat)
        with torch.no_grad():
            raw = {name: self.params[name].detach() for name, _ in self.fields}
            accum, denom = self._statistics_for_device()
            sample_div = _f32(0.8 * N)
            prune_on = 1 if iteration > prune_from_iter else 0
            proximity = iteration < proximity_until_iter
            u8 = lambda n: torch.empty((n,), dtype=torch.uint8, device=dev)   # noqa: E731

            def knn(xyz, n, with_idx):
                dist = torch.empty((n,), dtype=torch.float32, device=dev)
                nearest = torch.empty((n, 3), dtype=torch.int32, device=dev) if with_idx else None
                kb = int(api.raw("knn_tmp_bytes")(n))
                ktmp = u8(kb)
                api.call("knn_mean_dist2_idx", xyz.data_ptr(), n, dist.data_ptr(), None if nearest is None else nearest.data_ptr(),
                         ktmp.data_ptr(), kb, stream)
                return dist, nearest

            nbytes = api.raw("densify_fsgs_tmp_bytes")(P0)
            tmp = u8(nbytes)
            xyz1 = torch.empty((2 * P0, 3), dtype=torch.float32, device=dev)
            api.call("densify_fsgs_plan", raw["scaling"].data_ptr(), raw["opacity"].data_ptr(), accum.data_ptr(), denom.data_ptr(),
                     raw["xyz"].data_ptr(), P0, N, _f32(max_grad), _f32(self.percent_dense * extent), _f32(min_opacity),
                     _f32(0.1 * extent), _f32(extent), sample_div, 1 if max_screen_size else 0, tmp.data_ptr(), nbytes,
                     xyz1.data_ptr(), stream)
            n_clone = int(tmp[:4].view(torch.int32).cpu())                                   # read-back 1
            if P0 + n_clone < 4:
                return None
            dist1, _ = knn(xyz1, P0 + n_clone, False)
            api.call("densify_fsgs_merge", tmp.data_ptr(), nbytes, dist1.data_ptr(), P0, _f32(dist_thres * extent), prune_on, stream)
            ns, n_stay, keep_old, keep_clone, keep_split = tmp[32:52].view(torch.int32).cpu().tolist()   # read-back 2
            nQ = n_stay + n_clone + N * ns
            n_keep_q = keep_old + keep_clone + N * keep_split
            # a proximity row is kept exactly when its neighbour, a row of Q, is: nothing kept in Q = nothing kept at all
            if n_keep_q == 0 or (proximity and nQ < 4):
                return None
            noise = _split_noise(ns, N, generator, dev)
            table_q = torch.empty((nQ,), dtype=torch.int32, device=dev)
            xyz_q = torch.empty((nQ, 3), dtype=torch.float32, device=dev)
            api.call("densify_fsgs_emit", tmp.data_ptr(), nbytes, raw["xyz"].data_ptr(), raw["scaling"].data_ptr(),
                     raw["rotation"].data_ptr(), None if noise is None else noise.data_ptr(), P0, N, n_clone, ns, n_stay, nQ,
                     prune_on, table_q.data_ptr(), xyz_q.data_ptr(), stream)
            dist2, nearest = knn(xyz_q, nQ, True) if proximity else (None, None)
            qbytes = api.raw("densify_fsgs_tmp_bytes")(nQ)
            tmp_q = u8(qbytes)
            api.call("densify_fsgs_prox_plan", tmp.data_ptr(), nbytes, P0, table_q.data_ptr(), nQ,
                     None if dist2 is None else dist2.data_ptr(), None if nearest is None else nearest.data_ptr(),
                     _f32(5. * extent), prune_on, tmp_q.data_ptr(), qbytes, stream)
            S, n_keep_prox = 0, 0
            if proximity:
                _, S, k0, k1, k2 = tmp_q[:20].view(torch.int32).cpu().tolist()              # read-back 3
                n_keep_prox = k0 + k1 + k2
            P2 = n_keep_q + n_keep_prox
            table = torch.empty((P2,), dtype=torch.int32, device=dev)
            nb_kind = u8(P2)
            new_xyz = torch.empty((P2, 3), dtype=torch.float32, device=dev)
            sel_rows = torch.empty((2, max(S, 1)), dtype=torch.int32, device=dev)
            api.call("densify_fsgs_final", tmp_q.data_ptr(), qbytes, table_q.data_ptr(), xyz_q.data_ptr(),
                     None if nearest is None else nearest.data_ptr(), nQ, n_keep_q, S, n_keep_prox, P2, table.data_ptr(),
                     nb_kind.data_ptr(), new_xyz.data_ptr(), sel_rows[0].data_ptr(), sel_rows[1].data_ptr(), stream)
            perm = self._morton_perm_on_device(new_xyz, stream)
            self._gather_on_device("densify_fsgs_gather", (perm, table, nb_kind, new_xyz), P2, sample_div, stream,
                                   extra_fields=("opacity", "rotation"))
            self._zero_statistics()
            n_pruned = (ns + (nQ + 3 * S - P2)) if prune_on else 0
            return n_clone, ns, 3 * S, n_pruned

    def reset_opacity(self, value=0.01):
        """gaussian_model.py:258-261: opacity <- min(opacity, 0.01), moments of that group zeroed.  `value`: DNGaussian's
        form (DNGaussian/scene/gaussian_model.py:296-300) takes the ceiling as an argument."""
        self._clamp_opacity(torch.minimum, value)

    def reset_opacity_max(self, value=0.8):
        """DNGaussian/scene/gaussian_model.py:302-306: opacity <- max(opacity, value), moments of that group zeroed."""
        self._clamp_opacity(torch.maximum, value)

    def _clamp_opacity(self, bound, value):
        with torch.no_grad():
            op = torch.sigmoid(self.params["opacity"])
            new = bound(op, torch.full_like(op, value))
            self.params["opacity"].copy_(torch.log(new / (1 - new)))
            opt = self.optimizer
            opt.field_views(opt.exp_avg)["opacity"].zero_()
            opt.field_views(opt.exp_avg_sq)["opacity"].zero_()

    def update_learning_rate(self, iteration, position_lr_final=0.0000016, delay_mult=0.01, max_steps=30000,
                             exposure_max_steps=None):
        """gaussian_model.py:213-223: exponential decay of the xyz learning rate (over position_lr_max_steps) and of the
        exposure rate (over training_args.iterations, gaussian_model.py:208-211: `exposure_max_steps`)."""
        lr = expon_lr(iteration, LRS["xyz"] * self.spatial_lr_scale, position_lr_final * self.spatial_lr_scale,
                      lr_delay_mult=delay_mult, max_steps=max_steps)
        if isinstance(self.optimizer, FlatAdam):
            self.optimizer.lr["xyz"] = lr
        else:
            self.optimizer.set_xyz_lr(lr)
        if self.exposure_optimizer is not None:  # gaussian_model.py:215-217
            elr = expon_lr(iteration, 0.01, 0.001, lr_delay_steps=0, lr_delay_mult=0.0,
                           max_steps=max_steps if exposure_max_steps is None else exposure_max_steps)
            for group in self.exposure_optimizer.param_groups:
                group["lr"] = elr
        return lr

    # activations, gaussian_model.py:102-135
    @property
    def get_xyz(self):
        return self.params["xyz"]

    @property
    def get_scaling(self):
        return torch.exp(self.params["scaling"])

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self.params["rotation"])

    @property
    def get_opacity(self):
        return torch.sigmoid(self.params["opacity"])

    @property
    def get_features(self):
        return self.params["features"]

    def fused_activations(self):
        """(scales, rotations, opacities) through the fused kernels, or None when the model has no C-ABI optimizer
        (then the caller uses the get_* properties)."""
        api = getattr(self.optimizer, "api", None)
        if api is None or not hasattr(api, "_activations_fwd"):
            return None
        return _FusedActivations.apply(self.params["scaling"], self.params["rotation"], self.params["opacity"], self)

    def zero_grad(self):
        """set_to_none, as the reference does (train.py:283-288): autograd then ASSIGNS the new gradients
        instead of adding them to a zeroed buffer (no 236 B/Gaussian memset, no read-modify-write)."""
        for p in self.params.values():
            p.grad = None

    def grad_views(self):
        P, off, out = self.P, 0, {}
        shapes = self._shapes(P)
        for name, n in self.fields:
            out[name] = self.flat_grad[off:off + P * n].view(shapes[name])
            off += P * n
        return out

    def arm_grad_arena(self, backend):
        """Ask the rasterizer backward to write dL_dmeans3D / dL_dsh (51 of the 59 floats per Gaussian) straight
        into the flat gradient buffer: those two parameters reach the rasterizer without an activation in
        between, so autograd hands the very same tensors to the leaves and nothing is copied."""
        v = self.grad_views()
        backend.grad_arena = {"means3D": v["xyz"], "sh": v["features"]}

    def collect_grads(self):
        """After backward: make every .grad a view of the flat buffer (copy only what autograd produced elsewhere:
        the 8 floats per Gaussian behind exp / sigmoid / normalize, or everything when no arena was armed)."""
        for name, view in self.grad_views().items():
            p = self.params[name]
            g = p.grad
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr():
                view.copy_(g)
            p.grad = view

    def update_view_statistics(self, radii, viewspace_grad, into_delta=False):
        """train.py:266-268 + add_densification_stats in one kernel (gs_densify_stats) when available.
        into_delta: write this view's increments of xyz_gradient_accum / denom into `stat_delta` (zeroed first)
        instead of the running totals - the data-parallel step sums the increments over ranks before adding them."""
        api = getattr(self.optimizer, "api", None)
        if into_delta:
            self.stat_delta.zero_()
        acc = self.stat_delta[0] if into_delta else self.xyz_gradient_accum
        den = self.stat_delta[1] if into_delta else self.denom
        if api is not None and hasattr(api, "_densify_stats") and viewspace_grad is not None and viewspace_grad.is_contiguous():
            api.call("densify_stats", radii.data_ptr(), viewspace_grad.data_ptr(), self.P, self.max_radii2D.data_ptr(),
                     acc.data_ptr(), den.data_ptr(), _stream_of(radii))
            return
        if into_delta:
            vm = (radii > 0).to(torch.float32)
            torch.maximum(self.max_radii2D, radii.to(torch.float32), out=self.max_radii2D)
            acc += torch.norm(viewspace_grad[:, :2], dim=-1) * vm
            den += vm
            return
        # train.py:268 (radii are 0 for culled Gaussians, so a plain maximum equals the masked update)
        torch.maximum(self.max_radii2D, radii.to(torch.float32), out=self.max_radii2D)
        self.add_densification_stats(viewspace_grad, radii > 0)

    def add_densification_stats(self, viewspace_grad, visible_mask):
        # gaussian_model.py:471-473, written without boolean indexing (no host sync); rows of culled
        # Gaussians have zero gradient and zero mask, so the result is identical
        vm = visible_mask.to(torch.float32).unsqueeze(-1)
        self.xyz_gradient_accum += torch.norm(viewspace_grad[:, :2], dim=-1, keepdim=True) * vm
        self.denom += vm


class _TorchAdamWithFeatureSplit:
    """Reference optimiser on the flat storage: torch.optim.Adam for the four plain groups and for f_dc / f_rest
    as separate contiguous copies that are written back (the fused torch kernels need dense tensors)."""

    def __init__(self, groups, features, lr_dc, lr_rest):
        self.features = features
        self.f_dc = features.detach()[:, :1, :].clone().requires_grad_(True)
        self.f_rest = features.detach()[:, 1:, :].clone().requires_grad_(True)
        groups = groups + [{"params": [self.f_dc], "lr": lr_dc, "name": "f_dc"},
                           {"params": [self.f_rest], "lr": lr_rest, "name": "f_rest"}]
        self.opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)

    def set_xyz_lr(self, lr):
        for g in self.opt.param_groups:
            if g["name"] == "xyz":
                g["lr"] = lr

    def step(self):
        self.f_dc.grad = self.features.grad[:, :1, :].contiguous()
        self.f_rest.grad = self.features.grad[:, 1:, :].contiguous()
        self.opt.step()
        with torch.no_grad():
            self.features[:, :1, :] = self.f_dc
            self.features[:, 1:, :] = self.f_rest


def render(viewpoint_camera, pc, Rasterizer, Settings, bg_color, scaling_modifier=1.0, antialiasing=False,
           debug=False, filter_as_indices=True, clamp=True, fused=False, use_trained_exp=False, camera_index=None,
           raw_activations=False, camera_key=None):
    """= render() of LGDWT-GS/gaussian_renderer/__init__.py:18-128 (SH evaluated by the rasterizer, scale +
    rotation given, no exposure): returns {render, viewspace_points, visibility_filter, radii, depth}.
    raw_activations: hand the rasterizer the RAW scaling / rotation / opacity rows (the caller has told the backend,
    RasterBackend.raw_activations: the kernels activate them on the fly) - the fused train step's form."""
    act = pc.fused_activations() if fused and not raw_activations else None
    if raw_activations:
        act = (pc.params["scaling"], pc.params["rotation"], pc.params["opacity"])
        screenspace_points = torch.empty_like(pc.get_xyz).requires_grad_(True)
    elif act is None:
        screenspace_points = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True) + 0
        try:
            screenspace_points.retain_grad()
        except Exception:
            pass
        act = (pc.get_scaling, pc.get_rotation, pc.get_opacity)
    else:  # the step loop's lean form: the leaf only carries the view-space gradient - the rasterizer never reads
        # means2D (rasterize_points.cu takes no such argument) - so it is not even filled
        screenspace_points = torch.empty_like(pc.get_xyz).requires_grad_(True)
    scales, rotations, opacities = act
    rs = Settings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=debug, antialiasing=antialiasing)
    rasterizer = Rasterizer(raster_settings=rs)
    if camera_key is not None:  # stable camera identity for the backend's per-camera state (GaussianRasterizer.camera_key)
        rasterizer.camera_key = camera_key
        rasterizer.camera_limits = False   # (the train step asks for depth limits itself: Trainer.depth_limit)
    rendered_image, radii, depth_image = rasterizer(
        means3D=pc.get_xyz, means2D=screenspace_points, shs=pc.get_features, colors_precomp=None,
        opacities=opacities, scales=scales, rotations=rotations, cov3D_precomp=None)
    if use_trained_exp:  # gaussian_renderer/__init__.py:112-115 (training only): 3x3 colour matrix + offset per camera
        exposure = pc.get_exposure(camera_index)
        rendered_image = torch.matmul(rendered_image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + \
            exposure[:3, 3, None, None]
    if clamp:  # gaussian_renderer/__init__.py:119; the fused criterion applies (and differentiates) it itself
        rendered_image = rendered_image.clamp(0, 1)
    return {"render": rendered_image, "viewspace_points": screenspace_points,
            # the reference returns indices ((radii > 0).nonzero(): a host sync); the step loop asks for the
            # equivalent boolean mask instead and stays asynchronous
            # (filter_as_indices=None: not at all - the fused statistics kernel reads radii itself)
            "visibility_filter": None if filter_as_indices is None else
            ((radii > 0).nonzero() if filter_as_indices else (radii > 0)),
            "radii": radii, "depth": depth_image}


def camera_to(cam, device):
    return cam._replace(world_view_transform=cam.world_view_transform.to(device),
                        full_proj_transform=cam.full_proj_transform.to(device),
                        camera_center=cam.camera_center.to(device))


class TrainOptions:
    """The schedule constants of LGDWT-GS/arguments/__init__.py:78-100 (OptimizationParams)."""

    def __init__(self, **kw):
        self.iterations = 30_000
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.min_opacity = 0.005          # train.py:273
        self.size_threshold = 20          # train.py:272
        self.sh_increase_interval = 1000  # train.py:102
        self.depth_l1_weight_init = 1.0   # arguments/__init__.py:98-99; train.py:69: expon schedule over `iterations`
        self.depth_l1_weight_final = 0.01
        self.optimizer_type = "default"   # arguments/__init__.py:101 ("sparse_adam": Trainer(optimizer_type=...))
        self.white_background = False
        self.random_background = False    # arguments/__init__.py: a fresh torch.rand(3) background every iteration (train.py:117)
        self.cameras_extent = 1.0         # scene.cameras_extent = getNerfppNorm radius (dataset_readers.py:48-69)
        self.seed = 0
        self.densify_on_device = False    # densify_and_prune(on_device=True): the HIP form (GPU models only)
        self.densify_rule = "3dgs"        # "fsgs": GaussianModelLite.densify_and_prune_fsgs (FSGS/scene/gaussian_model.py:475-491)
        #                                   "dng": densify_and_prune_dng (DNGaussian/scene/gaussian_model.py:507-524)
        self.dist_thres = 10.0            # FSGS/arguments/__init__.py: the distance split
        self.prune_from_iter = 500        # ... every prune_points is gated by iteration > prune_from_iter
        self.proximity_until_iter = 2000  # FSGS/scene/gaussian_model.py:481
        self.split_opacity_thresh = 0.1   # DNGaussian/arguments/__init__.py:93: densify_rule = "dng" clones / splits above it only
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)


def cameras_extent(camera_centers):
    """getNerfppNorm (dataset_readers.py:48-69): 1.1 x the largest distance of a camera centre from their mean."""
    c = torch.stack([torch.as_tensor(x, dtype=torch.float64).reshape(3) for x in camera_centers])
    return float((c - c.mean(dim=0, keepdim=True)).norm(dim=1).max() * 1.1)


class Trainer:
    """One process per GPU; `step(k)` renders this rank's camera of global step k and updates the model;
    `train_iteration(it, opt)` is one iteration of the reference's loop with its schedule."""

    def __init__(self, model, cameras, gt_images, criterion, Rasterizer, Settings, bg, rank=0, world_size=1,
                 optimizer_step=True, masks=None, sharded_optimizer=None, sparse_exchange=None, optimizer_type="default",
                 alpha_masks=None):
        # sharded_optimizer (default: env GS_SHARDED_ADAM=1): reduce-scatter the gradients, Adam on this rank's 1/N of
        # the rows, all-gather the parameters - instead of all-reduce + the full Adam pass on every replica
        import os
        # Default for N > 1: sharded (GS_SHARDED_ADAM=0: all-reduce).  Byte model: both forms move 2 (N-1)/N x 244 B per
        # Gaussian over each GPU's links (an all-reduce IS a reduce-scatter + all-gather); the sharded form does it in two
        # large collectives instead of four chunks, runs 1/N of the 28 B/element optimizer pass, and owes an all-gather of
        # the moments only before a densification or a checkpoint.
        self.sharded_optimizer = (os.environ.get("GS_SHARDED_ADAM", "1") == "1") if sharded_optimizer is None \
            else bool(sharded_optimizer)
        # N > 1: move only the gradient rows of the Gaussians some rank's view reached (_exchange_and_step_sparse; replaces
        # the sharded / all-reduce forms when on).  GS_SPARSE_EXCHANGE=1 / sparse_exchange=True
        self.sparse_exchange = (os.environ.get("GS_SPARSE_EXCHANGE", "0") == "1") if sparse_exchange is None \
            else bool(sparse_exchange)
        self.last_exchange = None
        # optimizer_type = "sparse_adam" (train.py:68, 282-284): only the Gaussians with radii > 0 in the step's view - on N
        # GPUs: in SOME rank's view - are stepped (FlatAdam.sparse).  The moments then cannot be sharded by element range
        # (a shard would need the visibility of rows it does not own the statistics of): all-reduce or sparse exchange.
        if optimizer_type not in ("default", "sparse_adam"):
            raise ValueError("optimizer_type must be 'default' or 'sparse_adam'")
        self.optimizer_type = optimizer_type
        if optimizer_type == "sparse_adam":
            if not isinstance(model.optimizer, FlatAdam):
                raise RuntimeError("sparse_adam needs the flat Adam state (a model built with an api)")
            model.optimizer.sparse = True
            self.sharded_optimizer = False
        self.model, self.cameras, self.gts, self.criterion = model, cameras, gt_images, criterion
        self.Rasterizer, self.Settings, self.bg = Rasterizer, Settings, bg
        self.rank, self.world_size = rank, world_size
        self.optimizer_step = optimizer_step
        self.masks = masks  # per-camera ELF patch masks (depend on the ground truth only): cached
        # per-camera Camera.alpha_mask (scene/cameras.py:43-54, io.camera_alpha_mask): [1,H,W] / [H,W] on the model's device,
        # or None for the whole list - train.py:121-124 multiplies the render by it before the loss
        self.alpha_masks = alpha_masks
        self._bg_gen = None   # opt.random_background: the device generator and the one buffer GsView.bg points at
        # Depth regularisation (train.py:204-216): per camera None or (mono_invdepth [1,H,W], depth_mask [1,H,W] or None) - the
        # reference's viewpoint_cam.invdepthmap / depth_mask of a camera with depth_reliable (scene/cameras.py:60-80) - and the
        # current weight (train_iteration sets it from the schedule of train.py:69; 0 = term off)
        self.depth_priors = None
        self.depth_l1_weight = 0.0
        self.last = None
        # who this trainer is in the backend's per-camera state (keys ("trainer", uid, camera index)): a counter, not id() -
        # the address of a dead trainer is handed to the next one, which would then inherit its cameras' hints and limits
        Trainer._uids = getattr(Trainer, "_uids", 0) + 1
        self.uid = Trainer._uids
        # the backend keeps per-camera state under ("trainer", uid, camera): it goes when this trainer does
        be = getattr(getattr(getattr(self.Rasterizer, "_fn", None), "_impl", None), "backend", None)
        if be is not None and hasattr(be, "drop_camera_entries"):
            import weakref
            weakref.finalize(self, be.drop_camera_entries, ("trainer", self.uid))
        self._stack = []    # train.py:106-111: cameras are drawn without replacement
        self._rng = None

    def camera_index(self, k):
        return (k * self.world_size + self.rank) % len(self.cameras)

    def step(self, k):
        # (the camera of step k + 1 is known now: the step may start that view's geometry early, _request_early_geometry)
        return self._step_camera(self.camera_index(k), self.optimizer_step, (), next_ci=self.camera_index(k + 1))

    def draw_cameras(self, seed):
        """train.py:106-111 for `world_size` ranks: one global step pops world_size cameras from the shared stack
        (same python RNG on every rank), rank r takes the r-th."""
        import random
        if self._rng is None:
            self._rng = random.Random(seed)
        mine = None
        for r in range(self.world_size):
            if not self._stack:
                self._stack = list(range(len(self.cameras)))
            ci = self._stack.pop(self._rng.randint(0, len(self._stack) - 1))
            if r == self.rank:
                mine = ci
        return mine

    densify_decisions = None
    last_options = None   # the TrainOptions of the last train_iteration (prune_near_cameras / prune_unseen: on_device=None)
    alpha_masks = None
    _bg_gen = None
    _use_stage = False   # (set per step by _step_camera: exposure / alpha mask inside the criterion's node)

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of LGDWT-GS/train.py:97-288: LR schedule, SH ramp, camera draw, render + loss +
        backward, densification statistics, densify / prune / opacity reset on schedule, Adam.
        The reference replaces the parameter tensors when it densifies (their gradients are gone), so
        optimizer.step() of that iteration changes nothing; after reset_opacity only the opacity group is
        skipped.  Returns dict(loss, densified=(n_clone, n_split, n_pruned) or None, reset=bool, P).  With
        opt.densify_rule = "fsgs" the densification is FSGS's (densify_and_prune_fsgs) and `densified` its 4-tuple; with "dng" it
        is DNGaussian's (densify_and_prune_dng) and `densified` is (n_outliers, n_clone, n_split, n_pruned)."""
        # a step whose depth limits failed is repeated HERE, before this iteration's learning rate / SH degree exist: the
        # repeat must see the schedule state of the iteration it belongs to
        self.sync()
        self.last_options = opt
        m = self.model
        m.update_learning_rate(iteration, opt.position_lr_final, opt.position_lr_delay_mult, opt.position_lr_max_steps,
                               exposure_max_steps=opt.iterations)
        if iteration % opt.sh_increase_interval == 0:
            m.oneupSHdegree()
        if self.depth_priors is not None:   # train.py:69
            self.depth_l1_weight = expon_lr(iteration, opt.depth_l1_weight_init, opt.depth_l1_weight_final, max_steps=opt.iterations)
        ci = self.draw_cameras(opt.seed)
        if opt.random_background:   # train.py:117 (after sync: a repeated step has used the previous iteration's colour)
            self._draw_background(opt.seed)
        # What the schedule will do after the backward is known beforehand, so the optimizer step can run inside the
        # step (fused into the backward on one GPU, overlapped with the all-reduce on several).  Its order against
        # reset_opacity is free: the reset replaces the opacity row and its moments, the step skips exactly that row.
        in_densify = iteration < opt.densify_until_iter
        will_densify = in_densify and iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0
        will_reset = in_densify and (iteration % opt.opacity_reset_interval == 0 or
                                     (opt.white_background and iteration == opt.densify_from_iter))
        do_step = iteration < opt.iterations and not will_densify
        # the exposure tensor is never replaced by densification, so its optimizer steps on those iterations too
        # (train.py:279-281: every iteration below opt.iterations)
        loss = self._step_camera(ci, do_step, ("opacity",) if will_reset else (), exposure_step=iteration < opt.iterations)
        if will_densify or will_reset or iteration >= opt.iterations:
            self.sync()  # (depth-limited steps: the model is about to be read / re-laid out)
        densified, reset = None, False
        if will_densify:
            self.gather_optimizer_state()
            thr = opt.size_threshold if iteration > opt.opacity_reset_interval else None
            # (densify_decisions: parity instrument, see GaussianModelLite.densify_and_prune - a callable iteration -> dict)
            dec = self.densify_decisions(iteration) if self.densify_decisions is not None else None
            densified = self._densify(iteration, opt, opt.min_opacity, thr, radii=self.last["radii"], decisions=dec)
        if will_reset:
            m.reset_opacity()
            reset = True
        return dict(loss=loss, densified=densified, reset=reset, P=m.P, camera=ci)

    def _densify(self, iteration, opt, min_opacity, max_screen_size, rule=None, radii=None, decisions=None):
        """The densification of `iteration` by the rule opt.densify_rule names (or `rule`: a trainer of one method uses that
        method's rule whatever the options say), with the iteration's own CPU generator
        (opt.seed, iteration: every rank draws the same noise) -> what the rule returns.  min_opacity and max_screen_size are the
        caller's; FSGS (FSGS/train.py:166) and DNGaussian (DNGaussian/train_llff.py:199-201) take size_threshold = None, and
        DNGaussian max_dist = None."""
        m = self.model
        gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
        on_device = bool(getattr(opt, "densify_on_device", False))
        rule = rule or getattr(opt, "densify_rule", "3dgs")
        if rule == "fsgs":   # -> (n_clone, n_split, n_proximity, n_pruned)
            return m.densify_and_prune_fsgs(opt.densify_grad_threshold, min_opacity, opt.cameras_extent, None, iteration,
                                            dist_thres=opt.dist_thres, prune_from_iter=opt.prune_from_iter,
                                            proximity_until_iter=opt.proximity_until_iter, generator=gen, on_device=on_device)
        if rule == "3dgs":   # -> (n_clone, n_split, n_pruned)
            return m.densify_and_prune(opt.densify_grad_threshold, min_opacity, opt.cameras_extent, max_screen_size, radii,
                                       generator=gen, decisions=decisions, on_device=on_device)
        if rule == "dng":   # -> (n_outliers, n_clone, n_split, n_pruned)
            return m.densify_and_prune_dng(opt.densify_grad_threshold, min_opacity, opt.cameras_extent, None,
                                           opt.split_opacity_thresh, None, generator=gen, on_device=on_device)
        raise ValueError("densify_rule must be '3dgs', 'fsgs' or 'dng'")

    def _draw_background(self, seed):
        """A fresh rand(3) into the one persistent background buffer (allocated, with a generator seeded from seed + rank on
        the buffer's device, the first time): no allocation, no host synchronisation per iteration."""
        if self._bg_gen is None:
            dev = self.bg.device if torch.is_tensor(self.bg) else torch.device(self.model.device)
            self._bg_gen = torch.Generator(device=dev)
            self._bg_gen.manual_seed(int(seed) + self.rank)
            self.bg = torch.empty((3,), dtype=torch.float32, device=dev)
        torch.rand((3,), out=self.bg, generator=self._bg_gen)

    def _alpha(self, ci):
        return None if self.alpha_masks is None else self.alpha_masks[ci]

    def _image_extras(self):
        """Does the step touch the image between rasterizer and loss (trained exposure, alpha mask, random background)?"""
        return self.model.exposure is not None or self.alpha_masks is not None or self._bg_gen is not None

    def _stage_ok(self):
        """Can the fast step (manual backward, deferred depth limits) take this trainer's exposure / alpha masks, through the
        image stage (gs_image_stage_*) and the device exposure optimizer?  TrainerNIR (its own render and criterion) and
        optimizer_type "sparse_adam" are not wired to it: with an exposure, alpha masks or a random background they keep
        the slow form - the torch exposure of render(), the mask multiplied in torch, no deferred verdict."""
        from .optim import ExposureAdam
        m = self.model
        return (self.optimizer_type != "sparse_adam" and type(self)._render_view is Trainer._render_view
                and type(self)._criterion_backward is Trainer._criterion_backward
                and (m.exposure is None or isinstance(m.exposure_optimizer, ExposureAdam)))

    # single-GPU steps run the optimizer inside the rasterizer backward (gs_backward_step); GS_FUSED_STEP=0 keeps the
    # separate activation-backward / statistics / Adam kernels (the path every multi-GPU step takes)
    FUSED_STEP = __import__("os").environ.get("GS_FUSED_STEP", "1") != "0"

    def _fused_step_ok(self, backend, optimizer_step):
        m = self.model
        return (self.FUSED_STEP and optimizer_step and self.world_size == 1 and backend is not None
                and isinstance(m.optimizer, FlatAdam) and (not m.with_nir or self.RENDERS_NIR) and m.flat.is_cuda
                and hasattr(backend.api, "_backward_step") and hasattr(backend, "fused_step"))

    RENDERS_NIR = False   # (TrainerNIR: the step renders and steps the model's 4th channel)

    def _fused_dp_ok(self, backend, optimizer_step):
        """N > 1: the data-parallel form of the fused backward (GsStepState.grad_out): raw rows in, the 59 gradient floats per
        Gaussian written straight into the exchange buffer together with this view's statistic increments and validity
        flag - no activation kernels, no activated copies, no packing; the optimizer then runs gated by the reduced flag."""
        m = self.model
        return (self.FUSED_STEP and optimizer_step and self.world_size > 1 and backend is not None
                and isinstance(m.optimizer, FlatAdam) and (not m.with_nir or self.RENDERS_NIR) and m.flat.is_cuda
                and hasattr(backend.api, "_backward_step") and hasattr(backend.api, "_adam_step_gated")
                and hasattr(backend, "fused_step"))

    # Depth-limited instance lists (RasterBackend.depth_limit_request) for the fused single-GPU step: None = off,
    # "deferred" = on, with the forward's verdict ("were the cut lists long enough?") collected one step later, when it
    # costs no wait.  A step whose limits failed changed nothing on the device (gs_backward_step checks the same flag),
    # so it is simply taken again without limits; until then its loss tensor holds the value of the invalid image - it
    # is overwritten in place.  Anything that reads the model between steps goes through sync() first.
    depth_limit = None
    # the fused step hands the rasterizer the raw scaling / rotation / opacity rows (GsGaussians.raw_activations): the
    # activation kernel and its three output tensors disappear from the step; False keeps them
    RAW_ACTIVATIONS = True

    def sync(self):
        """Settle the verdict of the last depth-limited step (redoing the step if its limits failed), and that of the last
        replay of a GraphedStep bound to this trainer."""
        g = getattr(self, "_graphed", None)
        if g is not None:
            g.settle()
        # (an early geometry pass of the next view may still be reading the rows on the side stream: whatever the caller
        #  enqueues next - a re-layout, a reset, another optimizer - is ordered behind it)
        be = self._backend()
        if be is not None and hasattr(be, "join_early_geometry"):
            be.join_early_geometry()
        p, self._pending = getattr(self, "_pending", None), None
        if p is None:
            return
        if "flag_host" in p:
            # data-parallel step: the verdict is the REDUCED flag - the same number on every rank, so that all ranks repeat
            # the step (its collectives included) or none does; this rank's own verdict only updates its hints and limits
            p["event"].synchronize()
            if p["verdict"] is not None:
                p["verdict"]()
            if float(p["flag_host"][0]) == 0.0:
                return
        elif p["verdict"]():
            return
        if be is not None and hasattr(be, "drop_early_geometry"):
            be.drop_early_geometry()   # (a step that is repeated is not the view an early pass was made for)
        opt = self.model.optimizer
        opt.t, opt.seg_steps = p["counters"][0], dict(p["counters"][1])
        if p.get("exposure_steps") is not None:   # (its gated step changed nothing on the device either)
            self.model.exposure_optimizer.steps = p["exposure_steps"]
        if p["running_mean"] is not None:
            self.criterion.dwt_running_mean.copy_(p["running_mean"])
        p["loss"].copy_(self._step_camera(p["ci"], True, p["skip"], exposure_step=p.get("exposure_step")))  # (the camera's limits are invalid now: full lists)
        self.sync()

    def checkpoint(self):
        """model.capture() of a model in training: the pending depth-limit verdict is settled (so Adam's counters count
        only steps that happened) and, with the sharded optimizer, every rank's moments are gathered first."""
        self.sync()
        self.gather_optimizer_state()
        return self.model.capture()

    def _backend(self):
        be = getattr(getattr(self.Rasterizer, "_fn", None), "_impl", None)
        return getattr(be, "backend", None)

    # what a plain forward leaves on the backend besides its own cameras' entries: put back after an evaluation
    _EVAL_KEEPS = ("_capacity_hint", "_capacity_hint_limited", "_last", "last_workspace", "_pinned", "deferred",
                   "last_deferred_num_rendered")

    def evaluate(self, cameras=None, gts=None, **kw):
        """PSNR / SSIM / L1 of the trainer's model over a test set (default: its own cameras and ground truth) ->
        gsplat_amd.evaluate.evaluate_views' result; kw: names, quantise, clamp, masks, lpips (the LpipsWeights, for "LPIPS").

        Training state is left alone, and this is how: the pending verdict of the last step is settled first (sync);
        every view is rendered through the PLAIN forward under no_grad, named ("trainer", uid, "eval", i) with
        camera_limits off - so the per-camera entries of the training cameras (tile order, depth limits, the buffers a
        captured graph holds) are neither read nor written, and the evaluation's own entries go when the trainer does;
        the backend's capacity hints and last-forward records are restored afterwards.  No fused step is armed, no
        optimizer counter, running mean or random stream is touched."""
        from .evaluate import evaluate_views
        self.sync()
        cameras = self.cameras if cameras is None else cameras
        gts = self.gts if gts is None else gts
        be = self._backend()
        saved = {k: getattr(be, k) for k in self._EVAL_KEEPS if be is not None and hasattr(be, k)}
        try:
            return evaluate_views(self.model, cameras, gts, self.Rasterizer, self.Settings, self.bg,
                                  camera_keys=[("trainer", self.uid, "eval", i) for i in range(len(cameras))], **kw)
        finally:
            for k, v in saved.items():
                setattr(be, k, v)

    def wef_report(self, camera=0, bands="level2", path=None, titled=False, tile_cols=3):
        """The Wavelet Error Field of one training camera (gsplat_amd.wef): {"LL2", "LH2", "HL2", "WEF"} (bands="level2") or the
        eight bands and "COMBINED" (bands="all") of clamp(render, 0, 1) against the camera's ground truth, [1,1,H,W] each, plus
        "grid": their heatmap grid, uint8 [rows * H, tile_cols * W, 3] (titled: with the keys stamped on), written as a PNG
        when `path` is given.  The view is rendered as evaluate() renders: sync() first, the plain forward under no_grad with
        its own camera key, the backend's records restored - no optimizer counter, running mean, random stream or per-camera
        entry is touched.  Trainers with an evaluate() of their own (DNGaussian's) render differently and raise."""
        from . import wef
        if bands not in ("level2", "all"):
            raise ValueError("wef_report: bands is 'level2' or 'all' (got %r)" % (bands,))
        if type(self).evaluate is not Trainer.evaluate:
            raise NotImplementedError("wef_report renders as Trainer.evaluate does; %s renders its views differently" % type(self).__name__)
        self.sync()
        ci = int(camera)
        be = self._backend()
        saved = {k: getattr(be, k) for k in self._EVAL_KEEPS if be is not None and hasattr(be, k)}
        try:
            with torch.no_grad():
                img = render(self.cameras[ci], self.model, self.Rasterizer, self.Settings, self.bg, filter_as_indices=None,
                             clamp=False, camera_key=("trainer", self.uid, "eval", ci))["render"].clamp(0, 1)
        finally:
            for k, v in saved.items():
                setattr(be, k, v)
        gt = self.gts[ci].to(img.device)
        maps = wef.compute_wef_all_subbands(img, gt) if bands == "all" else wef.compute_wef_maps(img, gt)
        grid = (wef.make_wef_grid_image_titled if titled else wef.make_wef_grid_image)(maps, list(maps), tile_cols=tile_cols)
        if path is not None:
            from .imageio import write_png
            write_png(path, grid)
        return dict(maps, grid=grid)

    # -- DNGaussian's prunes between iterations (train_llff.py:206-213, 264-274): a re-layout each, so both are preceded by what
    # the densification branch of train_iteration does before it touches the model
    def _before_relayout(self, on_device, opt):
        """-> on_device resolved (None: densify_on_device of `opt`, else of the options train_iteration last ran with, else off)"""
        self.sync()
        self.gather_optimizer_state()
        if on_device is None:
            on_device = getattr(opt if opt is not None else self.last_options, "densify_on_device", False)
        return bool(on_device)

    def prune_near_cameras(self, centers, near_range, on_device=None, opt=None):
        """DNGaussian/train_llff.py:208-213: remove the Gaussians within `near_range` of any of the camera centres [K,3] (the
        spiral path's) - near_camera_mask (one launch, no read-back; on a CPU model the reference's own torch statements) handed
        to GaussianModelLite.prune_points.  on_device=None: densify_on_device of `opt`, or of the options train_iteration last
        ran with; False when there are none.
        Returns the number of rows removed."""
        on_device = self._before_relayout(on_device, opt)
        m = self.model
        with torch.no_grad():
            xyz = m.params["xyz"].detach()
            centers = torch.as_tensor(centers, dtype=torch.float32).reshape(-1, 3).to(xyz.device)
            if xyz.is_cuda:
                from .dng_reg import near_camera_mask
                mask = near_camera_mask(xyz, centers, near_range)
            else:
                mask = None
                for c in centers:
                    near = (xyz - c.repeat(xyz.shape[0], 1)).norm(dim=1, keepdim=True) < near_range
                    mask = mask + near if mask is not None else near
                mask = mask.squeeze(1)
        return m.prune_points(mask, on_device=on_device)

    def prune_unseen(self, camera_indices=None, on_device=None, opt=None):
        """clean_views (DNGaussian/train_llff.py:264-274): remove the Gaussians no training view sees.  One forward-only render
        per camera (default: all of the trainer's) as evaluate() makes them - plain forward under no_grad, own camera keys,
        the backend's hints restored -, `radii > 0` ORed on the model's device with no read-back, then prune_points.
        Returns the number of rows removed."""
        on_device = self._before_relayout(on_device, opt)
        m = self.model
        idx = range(len(self.cameras)) if camera_indices is None else list(camera_indices)
        be = self._backend()
        saved = {k: getattr(be, k) for k in self._EVAL_KEEPS if be is not None and hasattr(be, k)}
        seen = torch.zeros((m.P,), dtype=torch.bool, device=m.flat.device)
        try:
            with torch.no_grad():
                for ci in idx:
                    radii = render(self.cameras[ci], m, self.Rasterizer, self.Settings, self.bg, filter_as_indices=None,
                                   clamp=False, camera_key=("trainer", self.uid, "eval", ci))["radii"]
                    seen |= radii.reshape(-1) > 0
        finally:
            for k, v in saved.items():
                setattr(be, k, v)
        return m.prune_points(~seen, on_device=on_device)

    # The single-GPU fused step without the autograd engine: its graph is two custom nodes in a row (rasterizer, criterion) whose
    # gradients end inside gs_backward_step, so the step calls their forward / backward bodies itself (a stand-in context
    # object each) - no graph construction, no engine thread hand-off: ~0.15 ms less host time per step, which is what
    # keeps the eager step GPU-bound on slow hosts.  Same kernels, same arguments, same bits.  GS_MANUAL_BACKWARD=0: autograd.
    MANUAL_BACKWARD = __import__("os").environ.get("GS_MANUAL_BACKWARD", "1") != "0"

    class _ManualCtx:
        """What a torch.autograd.Function's forward / backward use of their context, and nothing else."""

        def __init__(self):
            self.saved_tensors = ()

        def save_for_backward(self, *tensors):
            self.saved_tensors = tensors

        def mark_non_differentiable(self, *a):
            pass

        def set_materialize_grads(self, v):
            pass

    def _manual_step_ok(self, fused_step, fused):
        fn = getattr(self.Rasterizer, "_fn", None)
        return (self.MANUAL_BACKWARD and fused_step and fused and (not self._image_extras() or self._stage_ok()) and fn is not None
                and getattr(getattr(fn, "_impl", None), "backend", None) is not None
                and type(self)._render_view is Trainer._render_view and type(self)._criterion_backward is Trainer._criterion_backward)

    def _raster_settings(self, ci):
        m, cam = self.model, self.cameras[ci]
        return self.Settings(
            image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=self.bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=m.active_sh_degree, campos=cam.camera_center, prefiltered=False,
            debug=False, antialiasing=False)

    # The early geometry pass (RasterBackend.EARLY_GEOMETRY): a step that is told its next camera (step(k): a pure function of k)
    # asks the backend to run that view's geometry kernel behind its side launch.  The result is used only by a forward for that
    # camera that finds the rows as this step's backward leaves them: the token below changes with every re-layout (generation,
    # P), every optimizer step (Adam's counter), every write through torch to a parameter tensor or a camera matrix (their
    # version counters: opacity reset, another optimizer) and with the SH degree.  Only for the plain eager fused step with
    # deferred depth limits: not TrainerNIR, not the data-parallel forms, not rows_override, not a GraphedStep's capture.
    def _early_token(self, ci):
        m, cam = self.model, self.cameras[ci]
        return (m.generation, m.P, m.active_sh_degree, id(m.optimizer), m.optimizer.t, m.flat._version,
                tuple(p._version for p in m.params.values()),
                tuple(t._version for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)))

    def _early_geometry_ok(self, backend, fused_step, deferred):
        m = self.model
        return (fused_step and deferred and not m.with_nir and not self.RENDERS_NIR and self.world_size == 1
                and getattr(self, "rows_override", None) is None and hasattr(backend, "request_early_geometry")
                and backend.static_capacity is None and getattr(self, "_graphed", None) is None
                and type(self)._render_view is Trainer._render_view)

    def _manual_step(self, ci, mask, backend, deferred):
        """render -> criterion -> backward of the fused single-GPU step, by hand (see MANUAL_BACKWARD) -> (pkg, loss, parts,
        the forward's deferred verdict or None)"""
        m = self.model
        fn = self.Rasterizer._fn
        rs = self._raster_settings(ci)
        backend.camera_key = ("trainer", self.uid, ci)   # (as GaussianRasterizer.forward does with its camera_key)
        backend.camera_key_limits = False
        empty = getattr(self, "_empty_cpu", None)
        if empty is None:
            empty = self._empty_cpu = torch.Tensor([])
        rctx, lctx = self._ManualCtx(), self._ManualCtx()
        with torch.no_grad():
            p = m.params
            color, radii, depth = fn.forward(rctx, p["xyz"], None, p["features"], empty, p["opacity"], p["scaling"], p["rotation"],
                                             empty, rs)
            verdict = backend.take_deferred() if deferred else None
            loss, parts = self.criterion.fused_call(color, self.gts[ci], mask=mask, manual_ctx=lctx,
                                                    exposure=None if m.exposure is None else m.exposure[ci], alpha=self._alpha(ci))
            grad_depth = None
            prior = self._depth_prior(ci)
            if prior is not None:   # train.py:204-216: one launch gives the term and its inverse-depth image gradient
                dl, grad_depth = self.criterion.ops.depth_l1_step(depth, prior[0], prior[1], self.depth_l1_weight)
                loss = loss + dl
                parts = dict(parts, depth_l1=dl)
            self._arm_side_launch(backend.launch_uninstanced_early)
            from .losses import FusedLGDWTLoss
            grad_img = FusedLGDWTLoss.backward(lctx, self.criterion.ops.unit_grad(loss.device), None)[1]
            fn.backward(rctx, grad_img, None, grad_depth)
        pkg = {"render": color, "viewspace_points": None, "visibility_filter": None, "radii": radii, "depth": depth}
        return pkg, loss, parts, verdict

    # -- what differs between the RGB step and the multispectral one (TrainerNIR)
    def _render_view(self, ci, fused, raw):
        m = self.model
        return render(self.cameras[ci], m, self.Rasterizer, self.Settings, self.bg, filter_as_indices=None,
                      clamp=not fused, fused=True, use_trained_exp=m.exposure is not None and not self._use_stage, camera_index=ci,
                      raw_activations=raw, camera_key=("trainer", self.uid, ci))

    def load_depth_priors(self, keys, depths_dir, depth_params=None, resolutions=None, nerf_synthetic=False):
        """Fill depth_priors from a folder of 16-bit inverse-depth PNGs (gsplat_amd/depth_priors.py::load_depth_priors): keys = per
        camera the image's name without extension, depth_params = read_depth_params' dict; resolutions default to the ground
        truths' (W, H).  The maps land on the ground truths' device."""
        from .depth_priors import load_depth_priors
        if resolutions is None:
            resolutions = [(int(g.shape[-1]), int(g.shape[-2])) for g in self.gts]
        self.depth_priors = load_depth_priors(keys, depths_dir, depth_params, resolutions, nerf_synthetic=nerf_synthetic,
                                              device=self.gts[0].device)
        return self.depth_priors

    def _depth_prior(self, ci):
        """(mono_invdepth, depth_mask) of camera ci when the depth term is on for it (train.py:206), else None"""
        if self.depth_priors is None or not self.depth_l1_weight > 0:
            return None
        return self.depth_priors[ci]

    def _depth_term(self, pkg, ci, loss, parts):
        prior = self._depth_prior(ci)
        if prior is None:
            return loss, parts
        dl = self.depth_l1_weight * self.criterion.ops.depth_l1(pkg["depth"], prior[0], prior[1])
        return loss + dl, dict(parts, depth_l1=dl.detach())

    def _criterion_backward(self, pkg, ci, mask, fused, side_launch):
        """-> (loss, parts); runs the backward.  side_launch: callable that issues the two-phase step's side launch (or None)"""
        alpha = self._alpha(ci)
        if self._use_stage:   # exposure and mask in the criterion's node (gs_image_stage_*); the exposure's sums in parts
            m = self.model
            loss, parts = self.criterion.fused_call(pkg["render"], self.gts[ci], mask=mask,
                                                    exposure=None if m.exposure is None else m.exposure.detach()[ci], alpha=alpha)
            loss, parts = self._depth_term(pkg, ci, loss, parts)
            self._arm_side_launch(side_launch)
            torch.autograd.backward(loss, self.criterion.ops.unit_grad(loss.device))
            return loss, parts
        if alpha is not None:   # train.py:121-124 in torch: image = clamp(render) * alpha_mask
            pkg = dict(pkg, render=(pkg["render"].clamp(0, 1) if fused else pkg["render"]) * alpha.reshape(pkg["render"].shape[-2:]))
        if fused:
            loss, parts = self.criterion.fused_call(pkg["render"], self.gts[ci], mask=mask)
            loss, parts = self._depth_term(pkg, ci, loss, parts)
            # two-phase step: the Adam stream of the Gaussians without instances starts on its side stream from inside the
            # criterion's backward (_arm_side_launch) - it needs nothing of the loss - and runs beside the blend
            self._arm_side_launch(side_launch)
            # (seeded with the criterion's cached constant 1: no fill kernel for the implicit seed, no multiply by it)
            torch.autograd.backward(loss, self.criterion.ops.unit_grad(loss.device))
        else:
            loss, parts = self.criterion(pkg["render"], self.gts[ci], mask=mask)
            loss, parts = self._depth_term(pkg, ci, loss, parts)
            loss.backward()
        return loss, parts

    def _arm_side_launch(self, side_launch):
        # the criterion's backward issues it before its last kernel (ssim_bwd): C3 0.983 ms/step, against 1.024 issued before
        # the criterion's backward and 1.01-1.15 at the start of the rasterizer's backward (no head start on the blend)
        self.criterion.ops.before_last_backward_kernel = side_launch

    def _unfused_tail(self, pkg, radii, optimizer_step, skip):
        m = self.model
        self.last_radii = radii
        with torch.no_grad():
            m.collect_grads()
            m.update_view_statistics(radii, pkg["viewspace_points"].grad, into_delta=self.world_size > 1)
            if self.world_size > 1:   # (a culled Gaussian's gradient row is all zero, rasterize_points.cu:163-172)
                torch.gt(radii, 0, out=m.grad_mask.view(torch.bool))
            self.exchange_and_step(optimizer_step, skip)

    def _step_camera(self, ci, optimizer_step, skip, exposure_step=None, next_ci=None):
        self.sync()
        m = self.model
        if exposure_step is None:
            exposure_step = optimizer_step
        m.zero_grad()
        backend = self._backend()
        fused_step = self._fused_step_ok(backend, optimizer_step)
        fused_dp = self._fused_dp_ok(backend, optimizer_step)
        fused = getattr(self.criterion, "fused", False)
        # exposure / alpha mask through the image stage: the exposure's step is a gated device launch (ExposureAdam), so a
        # view whose limits fail changes nothing and is repeated like any other.  Without the stage (TrainerNIR, sparse_adam,
        # the unfused forms) a trainable exposure keeps the eager form: torch has stepped it before the verdict arrives.
        stage_ok = self._stage_ok()
        self._use_stage = bool(fused and (fused_step or fused_dp) and stage_ok
                               and (m.exposure is not None or self.alpha_masks is not None))
        deferred = (fused_step or fused_dp) and self.depth_limit == "deferred" and getattr(self, "_coef_dev", None) is None \
            and (not self._image_extras() or stage_ok)
        early_ok = self._early_geometry_ok(backend, fused_step, deferred)
        if early_ok:   # (before this step's counters advance: the token of the rows as they stand)
            backend.early_token = self._early_token(ci)
        if deferred:
            counters = (m.optimizer.t, dict(m.optimizer.seg_steps))
            backend.depth_limit_request = "defer"
        if fused_dp:
            backend.raw_activations = self.RAW_ACTIVATIONS
            backend.fused_step = m.optimizer.grads_out_request()
            if not self.RAW_ACTIVATIONS:
                raise RuntimeError("the data-parallel fused backward takes the raw parameter rows (Trainer.RAW_ACTIVATIONS)")
        elif fused_step:
            backend.raw_activations = self.RAW_ACTIVATIONS
            backend.fused_step = m.optimizer.fused_request(skip, coef_dev=getattr(self, "_coef_dev", None))
            rows = getattr(self, "rows_override", None)  # parity tests: blend sums to use instead of stage 1
            if rows is not None:
                backend.fused_step.rows_override = rows.data_ptr()
            if self._use_stage and m.exposure is not None:   # the backward writes the view's verdict: the exposure's gate
                backend.fused_step.fail_flag = m.exposure_optimizer.gate.data_ptr()
            if early_ok and next_ci is not None:   # (the token of the rows as THIS step's backward will leave them)
                backend.request_early_geometry(self._raster_settings(next_ci), ("trainer", self.uid, next_ci),
                                               self._early_token(next_ci))
        elif backend is not None and hasattr(backend, "grad_arena") and not m.with_nir:
            m.arm_grad_arena(backend)
        mask = None if self.masks is None else self.masks[ci]
        rm = None
        path = "fused" if (fused_step or fused_dp) else "unfused"
        exp_steps = m.exposure_optimizer.steps if (self._use_stage and m.exposure is not None) else None
        if self.RAW_ACTIVATIONS and self._manual_step_ok(fused_step, fused):
            path = "manual"
            # (the deferred verdict of THIS forward is picked up inside: the backend parks it when the forward returns)
            pkg, loss, parts, verdict = self._manual_step(ci, mask, backend, deferred)
        else:
            pkg = self._render_view(ci, fused, (fused_step or fused_dp) and self.RAW_ACTIVATIONS)
            verdict = backend.take_deferred() if deferred else None
            if self.world_size > 1 and self.sparse_exchange:
                # which rows this view's gradient can touch is known NOW: the exchange of the masks starts behind the forward
                # (side stream), under the criterion and the backward
                if fused_dp and hasattr(backend, "export_row_mask") and backend.export_row_mask(m.union_mask):
                    self._begin_union()
                else:
                    self._begin_union(pkg["radii"] > 0)
            if verdict is not None and not fused:
                rm = getattr(self.criterion, "dwt_running_mean", None)
                rm = None if rm is None else rm.clone()
            loss, parts = self._criterion_backward(pkg, ci, mask, fused,
                                                   backend.launch_uninstanced_early if (fused_step and fused) else None)
        radii = pkg["radii"]
        if fused_dp:
            # gradients, statistic increments and the validity flag are in the exchange buffer: reduce, then the gated
            # optimizer; every rank learns the reduced flag one step later (sync) and repeats the step if it is set
            if backend.fused_step is not None:
                backend.fused_step = None
                raise RuntimeError("fused data-parallel step armed but the rasterizer backward did not run")
            with torch.no_grad():
                self.exchange_and_step(optimizer_step, skip, gate=m.fail_flag)
            if deferred:
                host = self._flag_blocks[self._flag_i % len(self._flag_blocks)] if getattr(self, "_flag_blocks", None) else None
                if host is None:
                    self._flag_blocks = [torch.zeros((1,), dtype=torch.float32).pin_memory() for _ in range(4)]
                    self._flag_i = 0
                    host = self._flag_blocks[0]
                self._flag_i += 1
                host.copy_(m.fail_flag, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(m.flat.device))
                if fused:
                    rm = parts.get("running_mean_before")
                self._pending = dict(verdict=verdict, flag_host=host, event=ev, ci=ci, skip=skip, counters=counters,
                                     running_mean=rm, loss=loss.detach(), exposure_steps=exp_steps, exposure_step=exposure_step)
        elif verdict is not None:
            if fused:  # (the criterion's combine kernel leaves the running mean it started from in its output: no clone)
                rm = parts.get("running_mean_before")
            self._pending = dict(verdict=verdict, ci=ci, skip=skip, counters=counters, running_mean=rm, loss=loss.detach(),
                                 exposure_steps=exp_steps, exposure_step=exposure_step)
        if fused_dp:
            pass
        elif fused_step:
            # gs_backward_step has already applied the activation backward, the view statistics and Adam
            if backend.fused_step is not None:
                backend.fused_step = None
                raise RuntimeError("fused train step armed but the rasterizer backward did not run")
        else:
            self._unfused_tail(pkg, radii, optimizer_step, skip)
        partials = parts.get("exposure_partials") if self._use_stage else None
        if partials is not None:
            # the image stage left camera ci's gradient as per-workgroup sums: one launch adds them up and steps (gated by
            # the view's verdict: the backward's flag on one GPU, the reduced one on N)
            eo = m.exposure_optimizer
            gate = m.fail_flag if fused_dp else eo.gate
            if self.world_size > 1:
                eo.grad_row(partials, ci)
                dist.all_reduce(m.exposure.grad, op=dist.ReduceOp.SUM)
                if exposure_step:
                    eo.step(gate=gate)
            elif exposure_step:
                eo.step_from_partials(partials, ci, gate=gate)
            else:
                eo.grad_row(partials, ci)
            eo.zero_grad(set_to_none=True)
        elif m.exposure_optimizer is not None:
            # train.py:280-281: the exposure optimizer steps with the main one; a camera's row is only touched by the
            # rank that rendered it, the others hold a zero gradient for it (N > 1: summed like every other gradient)
            if m.exposure.grad is not None:
                if self.world_size > 1:
                    dist.all_reduce(m.exposure.grad, op=dist.ReduceOp.SUM)
                if exposure_step:
                    m.exposure_optimizer.step()
            m.exposure_optimizer.zero_grad(set_to_none=True)
        self.last = dict(loss=loss.detach(), radii=radii, parts=parts, path=path)
        return loss.detach()

    DP_CHUNKS = 4

    def exchange_and_step(self, optimizer_step, skip=(), gate=None):
        """The one exchange step of the data-parallel path and the optimizer step.  The exchange buffer = the 59-
        floats-per-Gaussian gradients (236 B x P) followed by this step's increments of the densification statistics
        (8 B x P) is summed over ranks in DP_CHUNKS consecutive all-reduces (RCCL over xGMI; gloo in the CPU tests)
        issued back to back; as soon as chunk k has arrived its slice of the flat Adam update runs while chunks
        k+1.. are still on the links, so the optimizer (0.3 ms at 1 M Gaussians) hides behind the communication.
        A max over max_radii2D travels alongside.  The summed increments are then added to the running totals, so
        every replica holds the statistics of ALL cameras of the step."""
        m = self.model
        opt = m.optimizer
        chunked = isinstance(opt, FlatAdam)
        if self.world_size <= 1:
            if optimizer_step:
                if getattr(opt, "sparse", False):   # train.py:283: visible = radii > 0
                    opt.step(skip, row_mask=(self.last_radii > 0).to(torch.float32))
                else:
                    opt.step(*([skip] if skip else []))
            return
        timed = getattr(self, "exchange_events", None) is not None and m.flat.is_cuda
        if timed:  # bench.py: how long the compute stream sees the exchange + optimizer take
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(m.flat.device))
        try:
            return self._exchange_and_step(optimizer_step, skip, gate)
        finally:
            if timed:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(torch.cuda.current_stream(m.flat.device))
                self.exchange_events.append((e0, e1))

    def _exchange_and_step(self, optimizer_step, skip=(), gate=None):
        m = self.model
        opt = m.optimizer
        chunked = isinstance(opt, FlatAdam)
        if self.sparse_exchange and chunked:
            return self._exchange_and_step_sparse(optimizer_step, skip, gate)
        if self.sharded_optimizer and chunked:
            return self._exchange_and_step_sharded(optimizer_step, skip, gate)
        n_grad = m.flat_grad.numel()
        nch = self.DP_CHUNKS if chunked else 1
        n_stat_end = m.exchange.numel() - 4     # (the last four floats: validity flag + padding)
        wflag = None
        if gate is not None:  # the flag first, on its own: every chunk's gated update needs it
            wflag = dist.all_reduce(m.exchange[n_stat_end:], op=dist.ReduceOp.SUM, async_op=True)
        bounds = [(i * n_grad // nch) // 4 * 4 for i in range(nch)] + [n_stat_end]
        works = [dist.all_reduce(m.exchange[bounds[i]:bounds[i + 1]], op=dist.ReduceOp.SUM, async_op=True)
                 for i in range(nch)]
        if wflag is not None:
            wflag.wait()
        wmax = dist.all_reduce(m.max_radii2D, op=dist.ReduceOp.MAX, async_op=True)
        if optimizer_step and chunked:
            opt.begin_step(skip)
        sparse = chunked and opt.sparse
        for i, w in enumerate(works):
            w.wait()
            if optimizer_step and chunked and not sparse:
                opt.step_range(bounds[i], min(bounds[i + 1], n_grad), skip, gate=gate)
        if optimizer_step and sparse:
            # sparse_adam: the rows to step are those visible in some rank's view - the summed `denom` increments, which
            # travel behind the gradients in the last chunk: one update when everything has arrived
            opt.step_range(0, n_grad, skip, gate=gate, row_mask=m.stat_delta[1])
        if optimizer_step and not chunked:
            opt.step()
        wmax.wait()
        self._add_statistics(gate)

    def _add_statistics(self, gate):
        """running totals += the summed increments of all ranks' views - unless some rank's view was invalid (gate != 0):
        the step is about to be repeated, nothing of it may stay."""
        m = self.model
        if gate is None:
            m.xyz_gradient_accum += m.stat_delta[0].unsqueeze(1)
            m.denom += m.stat_delta[1].unsqueeze(1)
        else:
            ok = (gate == 0).to(torch.float32)
            m.xyz_gradient_accum += (m.stat_delta[0] * ok).unsqueeze(1)
            m.denom += (m.stat_delta[1] * ok).unsqueeze(1)

    # ---- the visibility-sparse exchange
    SPLIT_SPARSE_ADAM = True   # the optimizer of the sparse exchange in two parts, the first under the collective (False: one pass)

    def _begin_union(self, mask_src=None):
        """Start the exchange of the row masks NOW: `union_mask` <- this rank's mask (mask_src, or what the forward's geometry
        state says: Gaussians with instances), all-reduced (MAX) over the ranks, then its prefix (the packed row of every
        member) and its size K.  On the GPU all of it is enqueued on a SIDE stream right behind the forward - the collective is
        1 byte per Gaussian - while the criterion and the backward run on the main stream; K travels to a pinned host word,
        and the host reads it only when the backward has been enqueued (_exchange_and_step_sparse): off the critical path.
        No-op unless the sparse exchange is on."""
        if not (self.sparse_exchange and self.world_size > 1):
            return
        m = self.model
        dev = m.flat.device

        def work():
            if mask_src is not None:
                m.union_mask.copy_(mask_src.view(torch.uint8) if mask_src.dtype == torch.bool else mask_src)
            dist.all_reduce(m.union_mask, op=dist.ReduceOp.MAX)
            torch.cumsum(m.union_mask, dim=0, dtype=torch.int32, out=m.union_pos)
            m.union_pos.sub_(1)
            m.union_rows_f[0].copy_(m.union_mask)             # (uint8 -> float: 1.0 for the members)
            m.union_rows_f[1].copy_(m.union_mask == 0)
        if dev.type == "cuda":
            main = torch.cuda.current_stream(dev)
            side = getattr(self, "_union_stream", None)
            if side is None:
                side = self._union_stream = torch.cuda.Stream(device=dev)
                self._union_k = torch.zeros((1,), dtype=torch.int32).pin_memory()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                work()
                self._union_k.copy_(m.union_pos[-1:], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            self._union = dict(event=ev, stream=side)
        else:
            work()
            self._union = dict(event=None, stream=None, K=int(m.union_pos[-1]) + 1 if m.P else 0)

    def _exchange_and_step_sparse(self, optimizer_step, skip=(), gate=None):
        """Only Gaussians that emitted instances in SOME rank's view of this step have a non-zero gradient row - with
        depth-limited lists a fifth of them per view, and never more than the ~40 % any camera reaches - so: the union of the
        ranks' row masks (1 byte per Gaussian, exchanged early: _begin_union), the union's rows of the field-major gradient
        buffer packed into one contiguous buffer by ONE kernel (gs_rows_pack), THAT all-reduced, the sums scattered back
        (gs_rows_unpack), and the dense gated Adam on every replica (rows outside the union hold the exact sum already: zero
        on every rank - their update is the zero-gradient one, identical everywhere, no traffic).  Statistics + flag
        (8 B/Gaussian) and max_radii2D travel dense as in the other forms.  With two ranks the sums are the dense
        all-reduce's bit for bit (a + b commutes); with more the reduction order is the library's choice in either form.  The
        host reads the union's size (the collective's message length) from a pinned word the side stream filled while the
        backward ran."""
        import ctypes as C
        m, opt = self.model, self.model.optimizer
        P, W = m.P, m.width
        n_grad = m.flat_grad.numel()
        u = getattr(self, "_union", None)
        self._union = None
        if u is None:   # (nobody started it early: the backward's own mask, now)
            self._begin_union(m.grad_mask)
            u, self._union = self._union, None
        ws = dist.all_reduce(m.stat_tail, op=dist.ReduceOp.SUM, async_op=True)   # statistic increments + validity flag
        wmax = dist.all_reduce(m.max_radii2D, op=dist.ReduceOp.MAX, async_op=True)
        if u["event"] is not None:
            u["event"].synchronize()          # (recorded behind the mask exchange on the side stream: long done)
            K = int(self._union_k[0]) + 1
            torch.cuda.current_stream(m.flat.device).wait_stream(u["stream"])
        else:
            K = u["K"]
        if K:
            need = (K * W + 3) // 4 * 4
            buf = getattr(self, "_packed", None)
            if buf is None or buf.numel() < need or buf.device != m.flat.device:
                buf = self._packed = torch.empty((int(need * 1.25) + 1024,), dtype=torch.float32, device=m.flat.device)
            widths = (C.c_int32 * len(m.fields))(*[n for _, n in m.fields])
            stream = C.c_void_p(torch.cuda.current_stream(m.flat.device).cuda_stream) if m.flat.is_cuda else None
            opt.api.call("rows_pack", m.flat_grad.data_ptr(), P, len(m.fields), widths, m.union_mask.data_ptr(),
                         m.union_pos.data_ptr(), K, buf.data_ptr(), stream)
            wrows = dist.all_reduce(buf[:K * W], op=dist.ReduceOp.SUM, async_op=True)
        self.last_exchange = dict(union_rows=K, rows=P, sparse_bytes=4 * K * W + P + 4 * int(m.stat_tail.numel()),
                                  dense_bytes=4 * (n_grad + int(m.stat_tail.numel())))
        if gate is not None or opt.sparse:
            ws.wait()  # the gate is the reduced flag; sparse_adam: the summed visibility is the rows to step
        # The optimizer in two parts.  Rows OUTSIDE the union need nothing from the links: their summed gradient is zero on
        # every rank, so their (zero-gradient, gated) update runs NOW, on the compute stream, while the union's rows are on the
        # links - more than half of the dense Adam pass hides under the collective.  The union's rows follow when their sums
        # have been scattered back.  Every row is stepped exactly once with the same bias corrections: the same bits as one
        # dense pass (tests/test_dp_gloo.py compares with the all-reduce form).  sparse_adam keeps its single masked pass (its
        # rows - visible in SOME rank's view - are known from the summed statistics only).
        split = optimizer_step and not opt.sparse and self.SPLIT_SPARSE_ADAM
        if optimizer_step:
            opt.begin_step(skip)
        if split:
            opt.step_range(0, n_grad, skip, gate=gate, row_mask=m.union_rows_f[1])
        if K:
            wrows.wait()
            opt.api.call("rows_unpack", m.flat_grad.data_ptr(), P, len(m.fields), widths, m.union_mask.data_ptr(),
                         m.union_pos.data_ptr(), K, buf.data_ptr(), stream)
        if split:
            if K:
                opt.step_range(0, n_grad, skip, gate=gate, row_mask=m.union_rows_f[0])
        elif optimizer_step:
            opt.step_range(0, n_grad, skip, gate=gate, row_mask=m.stat_delta[1] if opt.sparse else None)
        ws.wait()
        wmax.wait()
        self._add_statistics(gate)

    def gather_optimizer_state(self):
        """Sharded optimizer only: every rank holds current Adam moments for ITS shard; before anything that needs them
        all (densification re-layout, checkpoint) they are all-gathered in place.  No-op otherwise."""
        m, opt = self.model, self.model.optimizer
        if not (self.sharded_optimizer and self.world_size > 1 and isinstance(opt, FlatAdam)) or self.sparse_exchange:
            return   # (all-reduce and sparse forms: every replica holds all moments)
        S = m.flat_padded.numel() // self.world_size
        for buf in (opt.exp_avg_padded, opt.exp_avg_sq_padded):
            dist.all_gather_into_tensor(buf, buf[self.rank * S:(self.rank + 1) * S])

    def _exchange_and_step_sharded(self, optimizer_step, skip=(), gate=None):
        """The sharded form of exchange_and_step: rank r owns elements [r S, (r+1) S) of the padded flat
        buffers.  reduce-scatter (SUM) leaves the summed gradients of its shard on each rank, Adam runs on that shard
        only (1/N of the 28 B/element pass), all-gather returns the updated parameters to every replica; the view
        statistics (8 B/Gaussian) and max_radii2D are all-reduced alongside.  Same bytes on the links as the all-reduce
        (which is a reduce-scatter + all-gather inside RCCL), 1/N of the optimizer pass.  Both collectives run in place
        on the padded buffers.  Replicas stay bit-identical: every parameter is computed once, by its owner.  With two
        ranks the sums equal the all-reduce path's bit for bit (a + b is commutative); with more the reduction order
        is the library's choice in both paths."""
        m, opt = self.model, self.model.optimizer
        world, rank = self.world_size, self.rank
        n, n_pad = m.flat.numel(), m.flat_padded.numel()
        S = n_pad // world
        lo, hi = rank * S, min((rank + 1) * S, n)
        gshard = m.grad_padded[rank * S:(rank + 1) * S]
        wg = dist.reduce_scatter_tensor(gshard, m.grad_padded, op=dist.ReduceOp.SUM, async_op=True)
        ws = dist.all_reduce(m.stat_tail, op=dist.ReduceOp.SUM, async_op=True)   # statistic increments + validity flag
        wmax = dist.all_reduce(m.max_radii2D, op=dist.ReduceOp.MAX, async_op=True)
        wg.wait()
        if gate is not None:
            ws.wait()  # the gate is the reduced flag
        if optimizer_step:
            opt.begin_step(skip)
            if hi > lo:
                opt.step_range(lo, hi, skip, grads=gshard, gate=gate)
            dist.all_gather_into_tensor(m.flat_padded, m.flat_padded[rank * S:(rank + 1) * S])
        ws.wait()
        wmax.wait()
        self._add_statistics(gate)


# ----------------------------------------------------------------------------------------------------------------
# multispectral (RGB + NIR) step: counterpart of LGDWT-GS/mult-dwtgs/train_nir.py:81-125 on the fused 4-channel pass
# ----------------------------------------------------------------------------------------------------------------
def render_rgb_nir(viewpoint_camera, pc, Settings, bg_color, scaling_modifier=1.0, antialiasing=False, debug=False,
                   two_pass_rasterizer=None, clamp=True, raw_activations=False, camera_key=None):
    """= render() + render_nir() of mult-dwtgs/gaussian_renderer/__init__.py:18-258: {render (clamped to [0,1] as
    :119 does), nir (channel 0 of the NIR pass, not clamped), viewspace_points, visibility_filter, radii, depth}.
    Default: ONE pass with the NIR albedo as a 4th blended channel (gsplat_amd.nir).  two_pass_rasterizer = a
    `GaussianRasterizer` class: the reference's two 3-channel passes through it (used as the parity target).
    raw_activations (the fused train step's form; the caller has told the backend, RasterBackend.raw_activations): the
    rasterizer gets the RAW scaling / rotation / opacity / albedo rows and the gain and activates them in its kernels.
    clamp=False: the fused criterion clamps (and differentiates the clamp of) the render itself."""
    from .nir import GaussianRasterizerX, nir_colors
    rs = Settings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=debug, antialiasing=antialiasing)
    if raw_activations:
        if two_pass_rasterizer is not None:
            raise RuntimeError("raw activations serve the fused 4-channel pass only")
        ssp = torch.empty_like(pc.get_xyz).requires_grad_(True)
        rast = GaussianRasterizerX(rs)
        if camera_key is not None:
            rast.camera_key, rast.camera_limits = camera_key, False
        color, radii, depth, nir_img = rast(
            means3D=pc.get_xyz, means2D=ssp, opacities=pc.params["opacity"], extra=pc.params["nir_albedo"],
            shs=pc.get_features, scales=pc.params["scaling"], rotations=pc.params["rotation"], extra_gain=pc.nir_gain)
        return {"render": color.clamp(0, 1) if clamp else color, "nir": nir_img, "viewspace_points": ssp,
                "viewspace_points_nir": None, "visibility_filter": None, "radii": radii, "depth": depth}
    act = pc.fused_activations()
    if act is None:
        act = (pc.get_scaling, pc.get_rotation, pc.get_opacity)
    scales, rotations, opacities = act
    nir = nir_colors(torch.sigmoid(pc.params["nir_albedo"]), pc.nir_gain)  # get_nir_albedo * clamp(gain), render_nir:166-169
    ssp = torch.zeros_like(pc.get_xyz, requires_grad=True)
    if two_pass_rasterizer is None:
        rast = GaussianRasterizerX(rs)
        if camera_key is not None:
            rast.camera_key, rast.camera_limits = camera_key, False
        color, radii, depth, nir_img = rast(
            means3D=pc.get_xyz, means2D=ssp, opacities=opacities, extra=nir, shs=pc.get_features, scales=scales,
            rotations=rotations)
        ssp2 = None
    else:
        rast = two_pass_rasterizer(raster_settings=rs)
        color, radii, depth = rast(means3D=pc.get_xyz, means2D=ssp, shs=pc.get_features, opacities=opacities,
                                   scales=scales, rotations=rotations)
        ssp2 = torch.zeros_like(pc.get_xyz, requires_grad=True)
        img3, _, _ = rast(means3D=pc.get_xyz, means2D=ssp2, shs=None, colors_precomp=nir[:, None].repeat(1, 3),
                          opacities=opacities, scales=scales, rotations=rotations)
        nir_img = img3[0:1]
    return {"render": color.clamp(0, 1) if clamp else color, "nir": nir_img, "viewspace_points": ssp,
            "viewspace_points_nir": ssp2, "visibility_filter": radii > 0, "radii": radii, "depth": depth}


class NirCriterion:
    """train_nir.py:88-104: (1 - l) L1 + l (1 - SSIM) on RGB, plus nir_weight * (L1 + 0.2 (1 - SSIM)) on the NIR image
    (mult-dwtgs/utils/loss_utils.py:93-144; the reference evaluates the single-channel SSIM on three identical
    copies, whose mean is the single-channel value).
    fused=True (device kernels available): both terms as FusedLGDWTLoss nodes - the RGB one on the un-clamped render
    (with the global / patch DWT terms when rgb_criterion asks for them), the NIR one through the same kernels on one
    channel with its own two weights (GsLgdwtParams.custom_base), no clamp; no torch pass over an image."""

    def __init__(self, ops, lambda_dssim=0.2, nir_weight=1.0, nir_l1_weight=1.0, nir_ssim_weight=0.2, rgb_criterion=None,
                 fused=False):
        """rgb_criterion: an LGDWTCriterion to use for the RGB term instead of train_nir.py's plain L1 + SSIM - the
        multispectral step WITH the global / patch DWT terms of LGDWT-GS/train.py:128-202 (BASELINE configs[4] names a
        patch-DWT loss; the reference's train_nir.py itself has none)."""
        from .losses import LGDWTCriterion
        self.ops, self.lambda_dssim, self.nir_weight = ops, lambda_dssim, nir_weight
        self.nir_l1_weight, self.nir_ssim_weight = nir_l1_weight, nir_ssim_weight
        self.rgb_criterion = rgb_criterion
        self.fused = bool(fused)
        if self.fused:
            if rgb_criterion is None:
                self.rgb_criterion = LGDWTCriterion(ops, lambda_dssim=lambda_dssim, dwt_enable=False, patch_dwt_enable=False)
            self._nir = LGDWTCriterion(ops, dwt_enable=False, patch_dwt_enable=False)
            self._nir.custom_base = (nir_weight * nir_l1_weight, nir_weight * nir_ssim_weight)
            self._nir.clamp = False

    # (the running mean of the RGB criterion's DWT scale: what a step that has to be taken back restores)
    @property
    def dwt_running_mean(self):
        return None if self.rgb_criterion is None else self.rgb_criterion.dwt_running_mean

    @dwt_running_mean.setter
    def dwt_running_mean(self, v):
        if self.rgb_criterion is not None:
            self.rgb_criterion.dwt_running_mean = v

    def elf_mask(self, gt_image):
        return self.rgb_criterion.elf_mask(gt_image)

    def fused_call(self, raw_image, gt_image, nir_pred, nir_gt, mask=None):
        """-> ((rgb_loss, nir_loss), parts): two scalars to seed the backward with (their sum is the step's loss)"""
        rgb, parts = self.rgb_criterion.fused_call(raw_image, gt_image, mask=mask)
        nir, nparts = self._nir.fused_call(nir_pred, nir_gt)
        parts = dict(parts)
        parts.update(rgb=rgb.detach(), nir=nir.detach(), nir_l1=nparts["l1"], nir_ssim=nparts["ssim"])
        return (rgb, nir), parts

    def __call__(self, image, gt_image, nir_pred, nir_gt, mask=None):
        o = self.ops
        if self.rgb_criterion is not None:
            rgb, _ = self.rgb_criterion(image, gt_image, mask=mask)
        else:
            l1 = o.l1_loss(image, gt_image)
            rgb = (1.0 - self.lambda_dssim) * l1 + self.lambda_dssim * (1.0 - o.ssim(image, gt_image))
        nir = self.nir_l1_weight * o.l1_loss(nir_pred, nir_gt) + self.nir_ssim_weight * (1.0 - o.ssim(nir_pred, nir_gt))
        return rgb + self.nir_weight * nir, dict(rgb=rgb.detach(), nir=nir.detach())


class TrainerNIR(Trainer):
    """Trainer for a model created with with_nir=True: one fused 4-channel pass per view, RGB + NIR losses, Adam over
    the 60-float rows (59 + raw NIR albedo) and the global gain.  With a fused NirCriterion on the GPU the step is the RGB
    trainer's: raw parameter rows, region-binned depth-limited lists with the deferred verdict, the criterion as two fused
    nodes, gs_backward_step_x (backward + activation backward + statistics + Adam over the six rows and the gain in the
    per-Gaussian kernels, two-phase with the side stream), hipGraph replay, and the data-parallel form."""
    RENDERS_NIR = True

    def __init__(self, model, cameras, gt_images, nir_images, criterion, Settings, bg, two_pass_rasterizer=None, **kw):
        from .nir import GaussianRasterizerX
        super().__init__(model, cameras, gt_images, criterion, None if two_pass_rasterizer is not None else GaussianRasterizerX,
                         Settings, bg, **kw)
        self.nirs = nir_images
        self.two_pass = two_pass_rasterizer

    def _fused_step_ok(self, backend, optimizer_step):
        return self.two_pass is None and getattr(self.criterion, "fused", False) and super()._fused_step_ok(backend, optimizer_step)

    def _fused_dp_ok(self, backend, optimizer_step):
        return self.two_pass is None and getattr(self.criterion, "fused", False) and super()._fused_dp_ok(backend, optimizer_step)

    def _render_view(self, ci, fused, raw):
        m = self.model
        if m.nir_gain.grad is not None:
            m.nir_gain.grad = None
        return render_rgb_nir(self.cameras[ci], m, self.Settings, self.bg, two_pass_rasterizer=self.two_pass,
                              clamp=not fused, raw_activations=raw,
                              camera_key=None if self.two_pass is not None else ("trainer", self.uid, ci))

    def _criterion_backward(self, pkg, ci, mask, fused, side_launch):
        kw = {} if mask is None else {"mask": mask}
        if fused:
            (rgb, nir), parts = self.criterion.fused_call(pkg["render"], self.gts[ci], pkg["nir"], self.nirs[ci], **kw)
            self._arm_side_launch(side_launch)
            unit = self.criterion.ops.unit_grad(rgb.device)
            torch.autograd.backward([rgb, nir], [unit, unit])
            with torch.no_grad():
                loss = rgb + nir
        else:
            loss, parts = self.criterion(pkg["render"], self.gts[ci], pkg["nir"], self.nirs[ci], **kw)
            loss.backward()
        return loss, parts

    def _unfused_tail(self, pkg, radii, optimizer_step, skip):
        m = self.model
        self.last_radii = radii
        with torch.no_grad():
            m.collect_grads()
            vg = pkg["viewspace_points"].grad
            if pkg["viewspace_points_nir"] is not None and pkg["viewspace_points_nir"].grad is not None:
                vg = vg + pkg["viewspace_points_nir"].grad
            m.update_view_statistics(radii, vg.contiguous(), into_delta=self.world_size > 1)
            if self.world_size > 1:
                dist.all_reduce(m.nir_gain.grad, op=dist.ReduceOp.SUM)
                torch.gt(radii, 0, out=m.grad_mask.view(torch.bool))
            self.exchange_and_step(optimizer_step, skip)
            if optimizer_step:
                # the reference keeps the global gain in the main Adam (mult-dwtgs/scene/gaussian_model.py:266-280): it
                # is stepped whenever optimizer.step() runs - and, like every group, not on a densification iteration.
                # Its step count is the main optimizer's (FlatAdam.seg_steps["nir_gain"], advanced by the step above)
                opt = m.optimizer
                if isinstance(opt, FlatAdam):
                    m.nir_gain_optimizer.state[m.nir_gain]["step"].fill_(float(opt.seg_steps["nir_gain"] - 1))
                m.nir_gain_optimizer.step()

    def exchange_and_step(self, optimizer_step, skip=(), gate=None):
        super().exchange_and_step(optimizer_step, skip, gate)
        if gate is not None and optimizer_step and self.world_size > 1:
            # fused data-parallel step: the gain's gradient travelled in the exchange tail (summed with the flag); its
            # Adam step, gated like every other row's, on every rank
            m, opt = self.model, self.model.optimizer
            gs = m.nir_gain_optimizer.state[m.nir_gain]
            segs = (opt._Seg * 1)()
            segs[0].begin, segs[0].end, segs[0].lr_a, segs[0].step = 0, 1, opt.lr["nir_gain"], opt.seg_steps["nir_gain"]
            gbuf = getattr(self, "_gain_grad_buf", None)   # (the kernel wants 16-byte aligned pointers: the word is not)
            if gbuf is None:
                gbuf = self._gain_grad_buf = torch.zeros((4,), dtype=torch.float32, device=m.flat.device)
            gbuf[:1].copy_(m.gain_grad_word)
            opt.api.call("adam_step_gated", m.nir_gain.data_ptr(), gbuf.data_ptr(), gs["exp_avg"].data_ptr(),
                         gs["exp_avg_sq"].data_ptr(), 1, segs, 1, opt.betas[0], opt.betas[1], opt.eps, opt.t,
                         gate.data_ptr(), _stream_of(m.flat))


# ----------------------------------------------------------------------------------------------------------------
# FSGS: the train loop of FSGS/train.py on the FSGS rasterizer generation
# ----------------------------------------------------------------------------------------------------------------
class FsgsOptions(TrainOptions):
    """FSGS/arguments/__init__.py:76-99 (OptimizationParams) over the fields of TrainOptions."""

    def __init__(self, **kw):
        super().__init__()
        self.iterations = 10_000
        self.position_lr_max_steps = 10_000
        self.densify_until_iter = 10_000
        self.densify_grad_threshold = 0.0005
        self.min_opacity = 0.005           # prune_threshold
        self.prune_from_iter = 500
        self.dist_thres = 10.0
        self.start_sample_pseudo = 2000
        self.end_sample_pseudo = 9500
        self.sample_pseudo_interval = 10
        self.depth_weight = 0.05
        self.depth_pseudo_weight = 0.5
        self.late_depth_weight = 0.001     # train.py:111-112: what depth_weight becomes beyond end_sample_pseudo
        self.opacity_reset_value = 0.05    # scene/gaussian_model.py:231
        self.sh_increase_interval = 500    # train.py:82
        self.densify_rule = "fsgs"
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)


def render_fsgs(viewpoint_camera, pc, Rasterizer, Settings, bg_color, confidence, scaling_modifier=1.0, debug=False,
                raw_activations=False, torch_activations=False):
    """= render() of FSGS/gaussian_renderer/__init__.py:20-132 (SH evaluated by the rasterizer, scale + rotation given, no
    trainable background): {render, viewspace_points, visibility_filter, radii, depth, alpha}; the image is NOT clamped.
    raw_activations: the rasterizer gets the RAW scaling / rotation / opacity rows (the caller has told the backend) - the
    fused train step's form; the view-space leaf is then never filled.  visibility_filter is None: the statistics read radii.
    torch_activations: exp / normalize / sigmoid as torch ops instead of the model's fused activation node, whose backward
    WRITES the three gradients into the model's flat gradient buffer - right for one render per backward, wrong for two."""
    if raw_activations:
        scales, rotations, opacities = pc.params["scaling"], pc.params["rotation"], pc.params["opacity"]
        screenspace_points = torch.empty_like(pc.get_xyz).requires_grad_(True)
    else:
        act = None if torch_activations else pc.fused_activations()
        scales, rotations, opacities = act if act is not None else (pc.get_scaling, pc.get_rotation, pc.get_opacity)
        screenspace_points = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True) + 0
        try:
            screenspace_points.retain_grad()
        except Exception:
            pass
    rs = Settings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=debug, confidence=confidence)
    rendered_image, radii, depth, alpha = Rasterizer(raster_settings=rs)(
        means3D=pc.get_xyz, means2D=screenspace_points, shs=pc.get_features, colors_precomp=None, opacities=opacities,
        scales=scales, rotations=rotations, cov3D_precomp=None)
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": None, "radii": radii,
            "depth": depth, "alpha": alpha}


class TrainerFSGS(Trainer):
    """The loop of FSGS/train.py:81-176 on the FSGS rasterizer generation (dgr_fsgs: colour, depth and alpha outputs), one GPU.

    A plain iteration - one camera, one optimizer step - takes the fused train step: raw parameter rows into
    gs_forward_render_fsgs, FsgsCriterion as one node on the un-clamped image and the depth image, gs_backward_step_fsgs
    (backward, activation backward, view statistics and Adam in the per-Gaussian kernel).  A pseudo-view iteration
    (train.py:116-131) renders a second camera before the one backward: two views feed one Adam step, so it takes the
    UN-fused path on purpose - both backwards accumulate into the model's gradients, then FlatAdam.step.  A densifying
    iteration is un-fused too (no optimizer step, as in Trainer).

    midas_depths: per training camera the monocular depth map [H,W] (viewpoint_cam.depth_image).
    pseudo_cameras + depth_estimator: the pseudo leg.  depth_estimator(rendered image [3,H,W]) -> depth [H,W] stands for
    FSGS's estimate_depth(..., mode='train') (MiDaS, which this package does not ship); its result may carry gradient.
    Without both the pseudo leg is OFF - a divergence from the reference, whose loop always samples pseudo views.
    pearson / pseudo_pearson: the depth terms of the un-fused path as callables (rendered, midas) -> loss, for models that do
    not live on the GPU (gsplat_amd.pearson has no CPU path); default: gsplat_amd.pearson's two functions.
    Closed to this trainer: world_size > 1, with_nir models, trained exposure, alpha masks, depth limits, "sparse_adam",
    the two-phase side launch and GraphedStep."""

    def __init__(self, model, cameras, gt_images, midas_depths, criterion, bg, Rasterizer=None, Settings=None,
                 pseudo_cameras=None, depth_estimator=None, pearson=None, pseudo_pearson=None, depth_weight=0.05,
                 opacity_lr=0.05, depth_limit=None, **kw):
        if Rasterizer is None or Settings is None:
            import dgr_fsgs
            Rasterizer = Rasterizer or dgr_fsgs.GaussianRasterizer
            Settings = Settings or dgr_fsgs.GaussianRasterizationSettings
        closed = None
        if kw.get("world_size", 1) > 1:
            closed = "data parallelism (world_size > 1)"
        elif getattr(model, "with_nir", False):
            closed = "a multispectral (with_nir) model"
        elif getattr(model, "exposure", None) is not None:
            closed = "a trained exposure"
        elif kw.get("alpha_masks") is not None:
            closed = "alpha masks"
        elif depth_limit is not None:
            closed = "depth-limited lists (depth_limit)"
        elif kw.get("optimizer_type", "default") == "sparse_adam":
            closed = 'optimizer_type = "sparse_adam"'
        if closed is not None:
            raise RuntimeError("TrainerFSGS: %s is closed to the FSGS rasterizer generation's trainer" % closed)
        super().__init__(model, cameras, gt_images, criterion, Rasterizer, Settings, bg, **kw)
        if len(midas_depths) != len(cameras):
            raise ValueError("TrainerFSGS: one MiDaS depth map per training camera")
        self.midas = midas_depths
        self.pseudo_cameras = pseudo_cameras
        self.depth_estimator = depth_estimator
        self.pearson, self.pseudo_pearson = pearson, pseudo_pearson
        self.depth_weight = depth_weight      # args.depth_weight: train_iteration lowers it beyond end_sample_pseudo
        self._weight_from_options = False
        self._pseudo_stack = []
        self._conf = None
        # FSGS/arguments/__init__.py:82: opacity_lr 0.05 (the model's default is LGDWT-GS's 0.025)
        opt = model.optimizer
        if isinstance(opt, FlatAdam):
            opt.lr["opacity"] = opacity_lr
        else:
            for g in opt.opt.param_groups:
                if g["name"] == "opacity":
                    g["lr"] = opacity_lr

    @property
    def depth_limit(self):
        return None

    @depth_limit.setter
    def depth_limit(self, v):
        if v is not None:
            raise RuntimeError("TrainerFSGS: depth-limited lists (depth_limit) are closed to the FSGS rasterizer generation's "
                               "trainer")

    def pseudo_on(self):
        return bool(self.pseudo_cameras) and self.depth_estimator is not None

    def _confidence(self):
        """torch.ones_like(pc.confidence), gaussian_renderer/__init__.py:42 (pipe.use_confidence is False): one tensor per size"""
        m = self.model
        c = self._conf
        if c is None or c.shape[0] != m.P or c.device != m.flat.device:
            c = self._conf = torch.ones((m.P, 1), dtype=torch.float32, device=m.flat.device)
        return c

    def _fused_step_ok(self, backend, optimizer_step):
        return (getattr(self.criterion, "fused", False) and super()._fused_step_ok(backend, optimizer_step)
                and hasattr(backend.api, "_backward_step_fsgs"))

    def _fused_dp_ok(self, backend, optimizer_step):
        return False

    def _render_camera(self, cam, raw, two_views=False):
        return render_fsgs(cam, self.model, self.Rasterizer, self.Settings, self.bg, self._confidence(), raw_activations=raw,
                           torch_activations=two_views)

    def _render_view(self, ci, fused, raw):
        return self._render_camera(self.cameras[ci], raw)

    def _loss(self, pkg, ci, fused):
        """FSGS/train.py:94-109 for training camera ci -> (loss, parts); no backward"""
        if fused:
            return self.criterion.fused_call(pkg["render"], pkg["depth"], self.gts[ci], self.midas[ci], self.depth_weight)
        return self.criterion(pkg["render"], pkg["depth"], self.gts[ci], self.midas[ci], self.depth_weight, pearson=self.pearson)

    def _criterion_backward(self, pkg, ci, mask, fused, side_launch):
        loss, parts = self._loss(pkg, ci, fused)
        self._arm_side_launch(None)   # (no side launch for this generation: nothing to issue from inside the criterion's backward)
        if fused:
            torch.autograd.backward(loss, self.criterion.ops.unit_grad(loss.device))
        else:
            loss.backward()
        return loss, parts

    def _step_pseudo(self, ci, pi, optimizer_step, skip, pseudo_scale):
        """An iteration with the pseudo leg (train.py:116-134): the training view's loss, the pseudo view's depth term, ONE
        backward through both renders, then the un-fused tail - statistics from the training view only.
        -> (loss, whether the pseudo term entered it)"""
        m = self.model
        m.zero_grad()
        fused = getattr(self.criterion, "fused", False)
        # (two renders under one backward: the activations are torch ops, whose gradients autograd ADDS up)
        pkg = self._render_camera(self.cameras[ci], False, two_views=True)
        loss, parts = self._loss(pkg, ci, fused)
        pkg2 = self._render_camera(self.pseudo_cameras[pi], False, two_views=True)
        midas2 = self.depth_estimator(pkg2["render"])
        pp = self.pseudo_pearson
        if pp is None:
            from .pearson import pseudo_depth_pearson_loss as pp
        term = pp(pkg2["depth"][0].reshape(-1, 1), midas2.reshape(-1, 1)).mean()
        entered = not bool(torch.isnan(term).sum())   # (train.py:129: the loop's one host read, on these iterations only)
        if entered:
            loss = loss + pseudo_scale * term
        loss.backward()
        self._unfused_tail(pkg, pkg["radii"], optimizer_step, skip)
        self.last = dict(loss=loss.detach(), radii=pkg["radii"], parts=dict(parts, pseudo=term.detach()), path="unfused")
        return loss.detach(), entered

    def _draw_pseudo(self):
        """train.py:117-119: pseudo cameras are drawn without replacement from their own stack, by the loop's one RNG"""
        if not self._pseudo_stack:
            self._pseudo_stack = list(range(len(self.pseudo_cameras)))
        return self._pseudo_stack.pop(self._rng.randint(0, len(self._pseudo_stack) - 1))

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of FSGS/train.py:81-176, in its order: SH ramp, camera draw, loss (depth_weight is lowered
        AFTER the loss of the first iteration beyond end_sample_pseudo is formed), the pseudo leg on its schedule, backward,
        statistics from the training view, FSGS's densification (size_threshold None), the optimizer step (none on a
        densifying iteration, as in Trainer), THEN the learning rate of this iteration - so the step of iteration k uses
        the rate of k - 1 and the first the initial one - and the opacity reset, after the step, no group skipped.
        Returns dict(loss, camera, sh_degree, xyz_lr (the rate the step used), depth_weight (the weight the loss used),
        stepped, densified (FSGS's 4-tuple or None), reset, pseudo (the pseudo term entered the loss), path, P).
        (The statistics are taken on every iteration, not only below densify_until_iter: nothing reads them afterwards.)"""
        self.last_options = opt
        m = self.model
        if not self._weight_from_options:
            self.depth_weight, self._weight_from_options = opt.depth_weight, True
        if iteration % opt.sh_increase_interval == 0:
            m.oneupSHdegree()
        ci = self.draw_cameras(opt.seed)
        pseudo = (self.pseudo_on() and iteration % opt.sample_pseudo_interval == 0
                  and opt.start_sample_pseudo < iteration < opt.end_sample_pseudo)
        will_densify = (iteration < opt.densify_until_iter and iteration > opt.densify_from_iter
                        and iteration % opt.densification_interval == 0)
        do_step = iteration < opt.iterations and not will_densify
        o = m.optimizer
        lr_used = o.lr["xyz"] if isinstance(o, FlatAdam) else next(g["lr"] for g in o.opt.param_groups if g["name"] == "xyz")
        weight_used = self.depth_weight
        entered = False
        if pseudo:
            pi = self._draw_pseudo()
            scale = min((iteration - opt.start_sample_pseudo) / 500., 1) * opt.depth_pseudo_weight
            loss, entered = self._step_pseudo(ci, pi, do_step, (), scale)
        else:
            loss = self._step_camera(ci, do_step, ())
        if iteration > opt.end_sample_pseudo:   # train.py:111-112
            self.depth_weight = opt.late_depth_weight
        densified = None
        if will_densify:
            densified = self._densify(iteration, opt, opt.min_opacity, None, rule="fsgs")
        m.update_learning_rate(iteration, opt.position_lr_final, opt.position_lr_delay_mult, opt.position_lr_max_steps)
        reset = (iteration - opt.start_sample_pseudo - 1) % opt.opacity_reset_interval == 0 and iteration > opt.start_sample_pseudo
        if reset:
            m.reset_opacity(opt.opacity_reset_value)
        return dict(loss=loss, camera=ci, sh_degree=m.active_sh_degree, xyz_lr=lr_used, depth_weight=weight_used,
                    stepped=do_step, densified=densified, reset=reset, pseudo=entered, path=self.last["path"], P=m.P)


# ----------------------------------------------------------------------------------------------------------------
# DNGaussian: DNGaussian/train_llff.py:68-228
# ----------------------------------------------------------------------------------------------------------------
class DngOptions(TrainOptions):
    """DNGaussian/arguments/__init__.py:75-108 (OptimizationParams) over the fields of TrainOptions, and the constants
    train_llff.py hard-codes as options, so that a test can compress the schedule."""

    def __init__(self, **kw):
        super().__init__()
        self.iterations = 30_000
        self.position_lr_start = 0
        self.opacity_lr = 0.05             # (position 0.00016, feature 0.0025, scaling 0.005, rotation 0.001: the model's own, LRS)
        self.neural_grid = 5e-3
        self.neural_net = 5e-4
        self.error_tolerance = 0.2
        self.split_opacity_thresh = 0.1
        self.soft_depth_start = 1000
        self.hard_depth_start = 0
        self.shape_pena = 0.001
        self.scale_pena = 0.001
        self.opa_pena = 0.01
        self.lambda_dssim = 0.2
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0001
        self.min_opacity = 0.01            # prune_threshold
        self.densify_rule = "dng"
        self.patch_range = (5, 17)         # train_llff.py:64 ("LLFF")
        self.smooth_start = 3000           # train_llff.py:106,132: `iteration > 3000`
        self.near_prune_interval = 25      # train_llff.py:206
        self.near_prune_start = 2000       # train_llff.py:209
        self.clean_iterations = [6000, 1]  # train_llff.py:184: testing_iterations + [first_iter]
        # True: the depth legs as forward + loss + ONE fused backward-and-step (gs_depth_backward_step) on a GPU model - the same
        # bits as the un-fused legs, which are the arbiter.  Opt-in: at the LLFF size the measured gain (3-5 % of an iteration)
        # is smaller than the window-to-window spread of the timing tool (profiles/dng_step_timing.txt)
        self.fused_depth_legs = False
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)


def _settings_of(Settings, cam, bg_color, sh_degree, P, scaling_modifier=1.0, debug=False):
    """The settings tuple of a DNGaussian pass; a tuple type with FSGS's `confidence` field gets the neutral one."""
    kw = dict(image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
              tanfovy=math.tan(cam.FoVy * 0.5), bg=bg_color, scale_modifier=scaling_modifier, viewmatrix=cam.world_view_transform,
              projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=debug)
    if "confidence" in getattr(Settings, "_fields", ()):
        kw["confidence"] = torch.ones((P, 1), dtype=torch.float32, device=cam.camera_center.device)
    return Settings(**kw)


def render_dng(viewpoint_camera, pc, neural, Rasterizer, Settings, bg_color, scaling_modifier=1.0, debug=False, view_dirs=None,
               activations=None):
    """= render() of DNGaussian/gaussian_renderer/__init__.py:21-123: colours from the neural renderer, the FSGS-generation
    rasterizer with colors_precomp -> {render, depth, alpha, viewspace_points, visibility_filter, radii, opacity, color}; the
    image is NOT clamped.
    (sigma, colour) = neural(xyz, unit view directions); the opacity is sigmoid(_opacity): the reference's combine_opacity
    returns the model's own opacity and ignores sigma, so sigma gets no gradient here and the first column of the sigma net's
    last layer never learns.
    view_dirs: (xyz, campos) -> unit directions [P,3]; default gsplat_amd.dng_reg.view_dirs (HIP tensors only).
    activations: (scales, rotations, opacities) already formed by the caller, who also hands them to the regulariser."""
    xyz = pc.get_xyz
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    if view_dirs is None:
        from .dng_reg import view_dirs
    dirs = view_dirs(xyz, viewpoint_camera.camera_center)
    sigma, colour = neural(xyz, dirs)
    scales, rotations, opacity = activations if activations is not None else (pc.get_scaling, pc.get_rotation, pc.get_opacity)
    rs = _settings_of(Settings, viewpoint_camera, bg_color, pc.active_sh_degree, xyz.shape[0], scaling_modifier, debug)
    image, radii, depth, alpha = Rasterizer(raster_settings=rs)(
        means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=colour, opacities=opacity, scales=scales,
        rotations=rotations, cov3D_precomp=None)
    return {"render": image, "depth": depth, "alpha": alpha, "viewspace_points": screenspace_points,
            "visibility_filter": radii > 0, "radii": radii, "opacity": opacity, "color": colour}


class TrainerDNG(Trainer):
    """The loop of DNGaussian/train_llff.py:68-228 in its order, one GPU: up to three optimizer steps per iteration.

      hard leg   (iteration > hard_depth_start) depth-only pass at opacity 0.95, the depth regulariser, Adam on `xyz` ONLY;
      soft leg   (iteration > soft_depth_start) the same loss on the pass at the model's opacities, Adam on `opacity` ONLY, on
                 the means the hard leg has just stepped;
      photometric  render_dng, L1 + lambda_dssim (1 - SSIM) + the per-Gaussian regulariser; clean / statistics / densification /
                 near-camera prune; then Adam on xyz, opacity, scaling, rotation - unless one of those re-layouts ran, the
                 near-camera prune with an empty mask included: the reference re-registers every per-Gaussian tensor there, the
                 new tensors have no gradient and torch skips them - and on the neural renderer's six tensors, always.
    Every tensor's bias corrections use its own step count (FlatAdam.seg_steps; torch keeps `step` per parameter): xyz and
    opacity run ahead of scaling and rotation, the neural tensors ahead of those after re-layouts.
    With DngOptions.fused_depth_legs = True a depth leg on a GPU model is forward + loss + gs_depth_backward_step
    (depth_pass.depth_leg_step): the per-Gaussian tail steps the row it has differentiated, same bits; the default (False) is
    pass -> backward -> FlatAdam.step on the one segment.

    depth_mono: one [H,W] map per training camera as stored; the loss target 255 - depth_mono is formed once.
    neural: nn.Module with forward(x, d) -> (sigma, colour) and get_params(lr, lr_net); default dng_neural.GridRenderer with
      bound (max - min).max() / 2 * 1.2 and coord_center mean(xyz) of the model at construction (gaussian_model.py:197-200).
    near_centers [K,3], near_range: the spiral render cameras' centres and --near.
    depth_loss / regulariser / view_dirs / near_mask: the pieces without a CPU path as callables, for models that are not on
      the GPU (defaults: gsplat_amd.depth_norm.depth_regulariser, dng_reg.gaussian_regulariser, dng_reg.view_dirs,
      dng_reg.near_camera_mask).  Off the GPU the depth legs go through `Rasterizer` as the reference's render_for_depth /
      render_for_opa do (colours of ones, the other inputs detached) and the neural tensors are stepped by torch's Adam.
    Not carried: the SH rows are never stepped (no gradient reaches them in this loop), and the reference's `_features [P,32]`
      and `_depth_err [P,1]` groups, which never get one either, do not exist here.
    Closed: world_size > 1, with_nir models, trained exposure, alpha masks, depth limits, "sparse_adam", the two-phase side
      launch, GraphedStep, and a fused photometric step (its colour and opacity gradients leave the rasterizer for the MLP and
      the regulariser: Adam cannot sit in that tail)."""

    after_backward = None   # parity instrument: callable(leg "hard" | "soft" | "photometric", trainer) behind an un-fused backward
    with_neural = True      # False (a subclass without a neural renderer): none is built, `neural` and its optimizer are None

    def __init__(self, model, cameras, gt_images, depth_mono, neural=None, near_centers=None, near_range=0.0, bg=None,
                 Rasterizer=None, Settings=None, criterion=None, depth_loss=None, regulariser=None, view_dirs=None, near_mask=None,
                 opacity_lr=0.05, neural_lrs=(5e-3, 5e-4), lambda_dssim=0.2, depth_limit=None, fused_step=False, side_launch=False,
                 **kw):
        if Rasterizer is None or Settings is None:
            import dgr_dng
            Rasterizer = Rasterizer or dgr_dng.GaussianRasterizer
            Settings = Settings or dgr_dng.GaussianRasterizationSettings
        closed = None
        if kw.get("world_size", 1) > 1:
            closed = "data parallelism (world_size > 1)"
        elif getattr(model, "with_nir", False):
            closed = "a multispectral (with_nir) model"
        elif getattr(model, "exposure", None) is not None:
            closed = "a trained exposure"
        elif kw.get("alpha_masks") is not None:
            closed = "alpha masks"
        elif depth_limit is not None:
            closed = "depth-limited lists (depth_limit)"
        elif kw.get("optimizer_type", "default") == "sparse_adam":
            closed = 'optimizer_type = "sparse_adam"'
        elif side_launch:
            closed = "the two-phase side launch"
        elif fused_step:
            closed = "a fused photometric step"
        if closed is not None:
            raise RuntimeError("TrainerDNG: %s is closed to DNGaussian's trainer" % closed)
        if not isinstance(model.optimizer, FlatAdam):
            raise RuntimeError("TrainerDNG needs the flat Adam state (a model built with an api)")
        if criterion is None:
            from .fsgs_criterion import FsgsCriterion
            from .losses import LossOps
            criterion = FsgsCriterion(LossOps(model.optimizer.api), lambda_dssim=lambda_dssim)
        dev = model.flat.device
        bg = torch.zeros(3, dtype=torch.float32, device=dev) if bg is None else bg
        super().__init__(model, cameras, gt_images, criterion, Rasterizer, Settings, bg, **kw)
        if len(depth_mono) != len(cameras):
            raise ValueError("TrainerDNG: one mono depth map per training camera")
        self.mono = self._mono_targets(depth_mono, dev)
        if neural is None and self.with_neural:
            from dng_neural import GridRenderer
            with torch.no_grad():
                xyz = model.params["xyz"].detach()
                neural = GridRenderer(bound=float((xyz.max(0).values - xyz.min(0).values).max()) / 2 * 1.2,
                                      coord_center=xyz.mean(0).cpu()).to(dev)
        self.neural = neural
        groups = neural.get_params(neural_lrs[0], neural_lrs[1]) if neural is not None else None
        if groups is None:
            self.neural_optimizer = None
        elif dev.type == "cuda":
            from .optim import FusedAdam
            self.neural_optimizer = FusedAdam(groups, lr=0.0, eps=1e-15, fuse_groups=True)
        else:
            self.neural_optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        self.near_centers = None if near_centers is None else torch.as_tensor(near_centers, dtype=torch.float32).reshape(-1, 3)
        self.near_range = float(near_range)
        self._depth_loss, self._regulariser, self._view_dirs, self._near_mask = depth_loss, regulariser, view_dirs, near_mask
        model.optimizer.lr["opacity"] = opacity_lr   # DNGaussian/arguments/__init__.py:85 (the model's default is LGDWT-GS's)

    def _mono_targets(self, depth_mono, dev):
        """the depth legs' targets, one [1,1,H,W] per camera, formed once: 255 - depth_mono"""
        return [(255.0 - torch.as_tensor(d, dtype=torch.float32).to(dev)).reshape(1, 1, *d.shape[-2:]) for d in depth_mono]

    @property
    def depth_limit(self):
        return None

    @depth_limit.setter
    def depth_limit(self, v):
        if v is not None:
            raise RuntimeError("TrainerDNG: depth-limited lists (depth_limit) are closed to DNGaussian's trainer")

    def _fused_step_ok(self, backend, optimizer_step):
        return False

    def _fused_dp_ok(self, backend, optimizer_step):
        return False

    def neural_parameters(self):
        if self.neural_optimizer is None:
            return []
        return [p for g in self.neural_optimizer.param_groups for p in g["params"]]

    def fused_legs_available(self):
        """the model lives on the GPU and the loaded library has gs_depth_backward_step"""
        m = self.model
        return m.flat.is_cuda and hasattr(m.optimizer.api, "_depth_backward_step")

    # -- the pieces
    def _activations(self):
        m = self.model
        return m.get_scaling, m.get_rotation, m.get_opacity

    def _render(self, cam, activations=None):
        return render_dng(cam, self.model, self.neural, self.Rasterizer, self.Settings, self.bg, view_dirs=self._view_dirs,
                          activations=activations)

    def _depth_images(self, cam, kind):
        """the un-fused leg's forward -> (depth [1,H,W], alpha): the depth-only pass on a GPU model, else the given Rasterizer
        as render_for_depth / render_for_opa call it"""
        m = self.model
        xyz = m.params["xyz"]
        scales, rotations = m.get_scaling.detach(), m.get_rotation.detach()
        if xyz.is_cuda and "confidence" not in getattr(self.Settings, "_fields", ()):
            from .depth_pass import depth_pass
            rs = _settings_of(self.Settings, cam, self.bg, m.active_sh_degree, m.P)
            if kind == "means":
                depth, alpha, _ = depth_pass(rs, xyz, 0.95, scales, rotations, grad="means")
            else:
                depth, alpha, _ = depth_pass(rs, xyz.detach(), m.get_opacity, scales, rotations, grad="opacity")
            return depth, alpha
        rs = _settings_of(self.Settings, cam, self.bg, m.active_sh_degree, m.P)
        ones = torch.ones((m.P, 3), dtype=torch.float32, device=xyz.device)
        if kind == "means":
            means, opacity = xyz, torch.ones((m.P, 1), dtype=torch.float32, device=xyz.device) * 0.95
        else:
            means, opacity = xyz.detach(), m.get_opacity
        _, _, depth, alpha = self.Rasterizer(raster_settings=rs)(
            means3D=means, means2D=torch.zeros_like(xyz, requires_grad=True), shs=None, colors_precomp=ones, opacities=opacity,
            scales=scales, rotations=rotations, cov3D_precomp=None)
        return depth, alpha

    def _leg_loss(self, ci, leg, depth, alpha, p_local, p_global, w_smooth, opt):
        """the loss of leg "hard" | "soft" on the pass's depth [1,H,W] and alpha images"""
        depth_loss = self._depth_loss
        if depth_loss is None:
            from .depth_norm import depth_regulariser as depth_loss
        return depth_loss(depth[None], self.mono[ci], p_local, p_global, opt.error_tolerance, w_local=0.1, w_global=1.0,
                          w_smooth=w_smooth)

    def _depth_leg(self, ci, kind, p_local, p_global, w_smooth, opt, stepping, leg=None, keep_grads=False, step_fields=None):
        """one depth leg -> (loss, "fused" | "unfused"); Adam on `xyz` (kind "means") or `opacity` alone when `stepping`.
        leg: the name _leg_loss and after_backward get (default "hard" / "soft" by kind).  keep_grads: the gradients an earlier
        leg left are not cleared, this leg's add to them (un-fused only); step_fields: the fields the un-fused step takes
        (default: this leg's one)."""
        m, o = self.model, self.model.optimizer
        cam = self.cameras[ci]
        field = "xyz" if kind == "means" else "opacity"
        leg = leg or ("hard" if kind == "means" else "soft")
        step_fields = (field,) if step_fields is None else tuple(step_fields)
        others = tuple(name for name, _ in m.fields if name not in step_fields)

        def loss_fn(depth, alpha):
            return self._leg_loss(ci, leg, depth, alpha, p_local, p_global, w_smooth, opt)
        if not keep_grads:
            m.zero_grad()
        if stepping and not keep_grads and step_fields == (field,) and opt.fused_depth_legs and self.fused_legs_available() and "confidence" not in getattr(self.Settings, "_fields", ()):
            from .depth_pass import depth_leg_step
            o.begin_step(others)
            rs = _settings_of(self.Settings, cam, self.bg, m.active_sh_degree, m.P)
            with torch.no_grad():
                scales, rotations = m.get_scaling, m.get_rotation
                opacity = 0.95 if kind == "means" else m.get_opacity
            loss, _ = depth_leg_step(rs, m.params["xyz"].detach(), opacity, scales, rotations, kind, loss_fn,
                                     m.params[field].detach(), o.field_views(o.exp_avg)[field], o.field_views(o.exp_avg_sq)[field],
                                     o.lr[field], o.seg_steps[field], o.betas, o.eps)
            o.invalidate_dormant()
            return loss, "fused"
        depth, alpha = self._depth_images(cam, kind)
        loss = loss_fn(depth, alpha)
        loss.backward()
        if self.after_backward is not None:
            self.after_backward(leg, self)
        if stepping:
            with torch.no_grad():
                views = m.grad_views()
                for name in step_fields:
                    g, view = m.params[name].grad, views[name]
                    if g is None:
                        view.zero_()
                    elif g.data_ptr() != view.data_ptr():
                        view.copy_(g)
                o.step(skip=others)
        return loss.detach(), "unfused"

    def prune_unseen(self, camera_indices=None, on_device=None, opt=None):
        """clean_views (train_llff.py:264-274) through render_dng: forward only, `radii > 0` ORed on the device, prune_points
        - a re-layout in the reference even when every Gaussian is seen"""
        on_device = self._before_relayout(on_device, opt)
        m = self.model
        idx = range(len(self.cameras)) if camera_indices is None else list(camera_indices)
        seen = torch.zeros((m.P,), dtype=torch.bool, device=m.flat.device)
        with torch.no_grad():
            for ci in idx:
                seen |= self._render(self.cameras[ci])["radii"].reshape(-1) > 0
        return m.prune_points(~seen, on_device=on_device)

    def prune_near_cameras(self, centers, near_range, on_device=None, opt=None):
        if self._near_mask is None:
            return super().prune_near_cameras(centers, near_range, on_device=on_device, opt=opt)
        on_device = self._before_relayout(on_device, opt)
        with torch.no_grad():
            xyz = self.model.params["xyz"].detach()
            mask = self._near_mask(xyz, torch.as_tensor(centers, dtype=torch.float32).reshape(-1, 3).to(xyz.device), near_range)
        return self.model.prune_points(mask.reshape(-1), on_device=on_device)

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of DNGaussian/train_llff.py:68-228 in its order: the learning rate of THIS iteration first
        (update_learning_rate(max(iteration - position_lr_start, 0)): every step of iteration k uses the rate of k), the camera
        draw, then by the same RNG the patch sizes of the legs that run (local, global; hard leg before soft leg), the hard leg,
        the soft leg, the photometric leg, clean / statistics + densification / near-camera prune under no_grad, and the
        photometric optimizer step - without the Gaussian groups when any of those re-layouts ran.
        Returns dict(loss, loss_hard, loss_soft, camera, patches (hard local, hard global, soft local, soft global; None for a leg
        that did not run), xyz_lr, stepped = dict(hard, soft, gaussians, neural), densified (DNGaussian's 4-tuple or None),
        near_pruned (rows removed, or None when the prune did not run), cleaned (likewise), P, path = dict(hard, soft))."""
        self.last_options = opt
        m = self.model
        xyz_lr = self._set_rates(iteration, opt)
        ci = self.draw_cameras(opt.seed)
        stepping = iteration < opt.iterations
        w_smooth = 0.1 if iteration > opt.smooth_start else 0.0
        lo, hi = opt.patch_range
        patches = [None, None, None, None]
        losses, path = dict(hard=None, soft=None), dict(hard=None, soft=None)
        stepped = dict(hard=False, soft=False, gaussians=False, neural=False)
        for k, (name, kind, start) in enumerate((("hard", "means", opt.hard_depth_start), ("soft", "opacity", opt.soft_depth_start))):
            if iteration > start:
                patches[2 * k] = self._rng.randint(lo, hi)
                patches[2 * k + 1] = self._rng.randint(lo, hi)
                losses[name], path[name] = self._depth_leg(ci, kind, patches[2 * k], patches[2 * k + 1], w_smooth, opt, stepping)
                stepped[name] = stepping
        pkg, loss = self._photometric_leg(ci, opt)
        cleaned, densified, near_pruned = self._after_photometric(iteration, opt, pkg, stepping, stepped)
        return dict(loss=loss.detach(), loss_hard=losses["hard"], loss_soft=losses["soft"], camera=ci, patches=tuple(patches),
                    xyz_lr=xyz_lr, stepped=stepped, densified=densified, near_pruned=near_pruned, cleaned=cleaned, P=m.P, path=path)

    def _set_rates(self, iteration, opt):
        """the learning rates of THIS iteration -> the means' rate"""
        m, o = self.model, self.model.optimizer
        xyz_lr = m.update_learning_rate(max(iteration - opt.position_lr_start, 0), opt.position_lr_final, opt.position_lr_delay_mult,
                                        opt.position_lr_max_steps)
        o.lr["opacity"] = opt.opacity_lr
        for g in self.neural_optimizer.param_groups:
            g["lr"] = opt.neural_grid if g["name"] == "neural_encoder" else opt.neural_net
        return xyz_lr

    def _photometric_leg(self, ci, opt, reg_scale=None):
        """render_dng, L1 + lambda_dssim (1 - SSIM) + the per-Gaussian regulariser (times reg_scale, a torch multiply on the 0-d
        term, when one is given), backward -> (pkg, loss)"""
        m = self.model
        m.zero_grad()
        for p in self.neural_parameters():
            p.grad = None
        act = self._activations()
        pkg = self._render(self.cameras[ci], act)
        base, l1, ssim_value = self.criterion.photometric(pkg["render"], self.gts[ci], l1_weight=1.0)
        regulariser = self._regulariser
        if regulariser is None:
            from .dng_reg import gaussian_regulariser as regulariser
        reg = regulariser(act[0], pkg["opacity"], opt.shape_pena, opt.scale_pena, opt.opa_pena)
        if reg_scale is not None:
            reg = reg * reg_scale
        loss = base + reg
        loss.backward()
        if self.after_backward is not None:
            self.after_backward("photometric", self)
        self.last = dict(loss=loss.detach(), radii=pkg["radii"], parts=dict(l1=l1.detach(), ssim=ssim_value.detach()), path="unfused")
        self.last_radii = pkg["radii"]
        return pkg, loss

    def _near_prune_due(self, iteration, opt):
        return (iteration - 1) % opt.near_prune_interval == 0 and iteration > opt.near_prune_start

    def _before_densify(self, iteration, opt, pkg):
        """behind the statistics of a densifying iteration, in front of densify_and_prune_dng (under no_grad)"""

    def _after_densify(self, iteration, opt):
        """behind densify_and_prune_dng, still under no_grad (a further prune here is part of the same re-layout)"""

    def _after_photometric(self, iteration, opt, pkg, stepping, stepped):
        """clean / statistics + densification / near-camera prune under no_grad, then the photometric optimizer step - without the
        Gaussian groups when any of those re-layouts ran -> (cleaned, densified, near_pruned)"""
        m, o = self.model, self.model.optimizer
        cleaned = densified = near_pruned = None
        with torch.no_grad():
            m.collect_grads()   # (into the flat gradient buffer, before anything replaces it; the SH rows: zeros, never stepped)
            relayout = False
            clean = iteration in opt.clean_iterations
            if clean:
                cleaned = self.prune_unseen(opt=opt)
                relayout = True
            if iteration < opt.densify_until_iter and not clean:
                m.update_view_statistics(pkg["radii"], pkg["viewspace_points"].grad)
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    self._before_densify(iteration, opt, pkg)
                    densified = self._densify(iteration, opt, opt.min_opacity, None, rule="dng")
                    self._after_densify(iteration, opt)
                    relayout = True
            if self._near_prune_due(iteration, opt):
                # (prune_points runs in the reference even when the mask is empty - the default --near 0 makes it so - and
                #  re-registers every tensor: a re-layout as far as the optimizer step below is concerned)
                centers = self.near_centers if self.near_centers is not None else torch.zeros((0, 3))
                near_pruned = self.prune_near_cameras(centers, self.near_range, opt=opt) if centers.shape[0] else 0
                relayout = True
            if stepping:
                if not relayout:
                    o.step(skip=("features",))
                    stepped["gaussians"] = True
                self.neural_optimizer.step()
                stepped["neural"] = True
            m.zero_grad()
            for p in self.neural_parameters():
                p.grad = None
        return cleaned, densified, near_pruned

    def checkpoint(self):
        """Trainer.checkpoint() plus the neural renderer's state_dict, its optimizer state and the loop's RNG and camera stack"""
        state = super().checkpoint()
        state["neural"] = {k: v.detach().cpu().clone() for k, v in self.neural.state_dict().items()}
        sd = self.neural_optimizer.state_dict()
        state["neural_optimizer"] = dict(param_groups=sd["param_groups"], state={
            k: {kk: (vv.detach().cpu().clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in sd["state"].items()})
        state["rng"] = None if self._rng is None else self._rng.getstate()
        state["stack"] = list(self._stack)
        return state

    def restore(self, state):
        """the inverse of checkpoint(): model, moments and counters, neural renderer and its optimizer, RNG and camera stack"""
        import random
        self.model.restore(state)
        self.neural.load_state_dict(state["neural"])
        self.neural_optimizer.load_state_dict(state["neural_optimizer"])
        if state.get("rng") is not None:
            self._rng = random.Random()
            self._rng.setstate(state["rng"])
        self._stack = list(state["stack"])

    def evaluate(self, cameras=None, gts=None, names=None, quantise=True, clamp=True, masks=None, lpips=None):
        """PSNR / SSIM / L1 over a test set (default: the trainer's cameras and ground truth), every view rendered through
        render_dng under no_grad -> gsplat_amd.evaluate.Evaluator.result(names).  No optimizer counter, statistic or random
        stream is touched.  lpips: the LpipsWeights, for the "LPIPS" entries."""
        from .evaluate import Evaluator
        cameras = self.cameras if cameras is None else cameras
        gts = self.gts if gts is None else gts
        ev = None
        with torch.no_grad():
            for i, (cam, gt) in enumerate(zip(cameras, gts)):
                img = self._render(cam)["render"]
                if ev is None:
                    ev = Evaluator(len(cameras), img.shape[0], img.shape[1], img.shape[2], img.device, lpips=lpips)
                ev.add(i, img, gt, mask=None if masks is None else masks[i], clamp=clamp, quantise=quantise)
        return ev.result(names)


# ----------------------------------------------------------------------------------------------------------------
# DNGaussian on DTU: DNGaussian/train_dtu.py:39-250
# ----------------------------------------------------------------------------------------------------------------
class DngDtuOptions(DngOptions):
    """DngOptions with what train_dtu.py hard-codes: the patch range, no smoothness term, no near-camera prune, the object
    mask's threshold and run, the soft leg's gate on the running hard loss, the alpha leg, and the two colour rules.
    A rule is (threshold, divisor, reset) or None; reset is False, True (every time the rule runs) or a period n (the
    iterations with iteration % n == 0)."""

    def __init__(self, **kw):
        super().__init__()
        self.patch_range = (17, 53)                 # train_dtu.py:62
        self.smooth_start = None                    # no smoothness term at any iteration
        self.near_prune_interval = None             # no spiral cameras, no near-camera prune
        self.near_prune_start = None
        self.bg_threshold = 30 / 255                # :87 (scan110: 15 / 255, :89)
        self.bg_run = 50                            # :91: the pixel and the 49 above it
        self.soft_gate = 0.1                        # :128
        self.ema = (0.1, 0.9)                       # :127
        self.alpha_leg = True                       # :155-159
        self.black_rule = (20 / 255, 10, True)      # :221-223
        self.white_rule = (240 / 255, 2, 2001)      # :226-230
        self.reset_opacity_to = 0.1                 # :223, :230
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)

    @classmethod
    def for_scan(cls, name, **kw):
        """the reference's three scan exceptions (it tests `'scan110' in source_path` and so on): scan110 has the lower mask
        threshold and no colour rule, scan114 and scan21 no white rule"""
        name = str(name)
        o = dict()
        if "scan110" in name:
            o.update(bg_threshold=15 / 255, black_rule=None, white_rule=None)
        elif "scan114" in name or "scan21" in name:
            o.update(white_rule=None)
        o.update(kw)
        return cls(**o)


def _rule_at(rule, iteration):
    """a DngDtuOptions rule at an iteration -> (threshold, divisor, reset now) or None"""
    if rule is None:
        return None
    thr, div, reset = rule
    return thr, div, bool(reset) and iteration % int(reset) == 0


class TrainerDNGDTU(TrainerDNG):
    """The loop of DNGaussian/train_dtu.py:39-250 in its order - TrainerDNG's with what the DTU script adds:

      mask       per camera, once (:84-94; it depends on the ground truth alone): the object mask, the ground truth with the
                 masked pixels zeroed (what the photometric leg sees), and the mono target 255 - depth_mono FILLED with the
                 mean of its unmasked pixels (:104, :137);
      hard leg   as TrainerDNG's on the depth image filled the same way (:105), no smoothness term; then
                 ema_loss_hard = 0.1 loss_hard + 0.9 ema_loss_hard, a Python float: 4 bytes read back, the loop's ONE
                 synchronisation - it decides host work;
      soft leg   iff iteration > soft_depth_start AND ema_loss_hard < soft_gate (:128); its patch sizes are drawn only then;
      alpha leg  every iteration (:155-159): the soft pass again, mean(alpha[mask] ** 2), Adam on `opacity` alone - with an
                 empty mask a NaN loss and a zero gradient that Adam still steps on;
      photometric  against the zeroed ground truth; in front of every densification the colour rules (:218-230) on the
                 per-Gaussian colour of THIS iteration's photometric render (nothing has been stepped since: the reference's
                 second render gives the same tensor); no near-camera prune.
    The last iteration (iteration == opt.iterations): the reference leaves out every step but the alpha leg's, and does not
    clear the gradients in between - so that one step takes `xyz` with the hard leg's gradient and `opacity` with the soft
    leg's plus the alpha leg's.  The same here (un-fused: no fused form steps two tensors).
    With DngDtuOptions.fused_depth_legs = True all three legs go through depth_pass.depth_leg_step on a GPU model.

    background_mask / masked_fill / alpha_penalty / colour_rule: the new pieces as callables for models that are not on the GPU
      (defaults: gsplat_amd.dng_dtu's).  opt: the DngDtuOptions whose bg_threshold / bg_run form the masks (default: its
      defaults).  self.gts holds the ZEROED images: evaluate() compares against them unless given others.
    train_iteration's dict gains loss_alpha, ema_loss_hard, soft_gate_open, rule_counts ((black, white) device counts of a
      densifying iteration, else None), stepped["alpha"], path["alpha"].  Everything closed to TrainerDNG is closed here."""

    def __init__(self, model, cameras, gt_images, depth_mono, opt=None, background_mask=None, masked_fill=None, alpha_penalty=None,
                 colour_rule=None, **kw):
        super().__init__(model, cameras, gt_images, depth_mono, **kw)
        opt = DngDtuOptions() if opt is None else opt
        if background_mask is None or masked_fill is None or alpha_penalty is None or colour_rule is None:
            from . import dng_dtu
            background_mask = background_mask or dng_dtu.dtu_background_mask
            masked_fill = masked_fill or dng_dtu.masked_mean_fill
            alpha_penalty = alpha_penalty or dng_dtu.alpha_penalty
            colour_rule = colour_rule or dng_dtu.colour_rule
        self._masked_fill, self._alpha_penalty, self._colour_rule = masked_fill, alpha_penalty, colour_rule
        dev = model.flat.device
        self.bg_masks, gts, mono = [], [], []
        with torch.no_grad():
            for gt, mn in zip(self.gts, self.mono):
                mask, zeroed = background_mask(torch.as_tensor(gt, dtype=torch.float32).to(dev).contiguous(), opt.bg_threshold,
                                               opt.bg_run)
                self.bg_masks.append(mask)
                gts.append(zeroed)
                mono.append(masked_fill(mn.reshape(mask.shape), mask).reshape(mn.shape))
        self.gts, self.mono = gts, mono
        self.ema_loss_hard = 0.0
        from .dng_dtu import reset_value
        self._reset_value = reset_value

    def _leg_loss(self, ci, leg, depth, alpha, p_local, p_global, w_smooth, opt):
        if leg == "alpha":
            return self._alpha_penalty(alpha, self.bg_masks[ci])
        return super()._leg_loss(ci, leg, self._masked_fill(depth, self.bg_masks[ci]), alpha, p_local, p_global, w_smooth, opt)

    def _near_prune_due(self, iteration, opt):
        return False

    def _before_densify(self, iteration, opt, pkg):
        black, white = _rule_at(opt.black_rule, iteration), _rule_at(opt.white_rule, iteration)
        self._rule_counts = None
        if black is None and white is None:
            return
        m = self.model
        self._rule_counts = self._colour_rule(pkg["color"].detach(), m.xyz_gradient_accum, m.params["opacity"].detach(),
                                              black=black, white=white, value=self._reset_value(opt.reset_opacity_to))

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of train_dtu.py:64-247 in its order: learning rate, camera draw, hard leg, the `ema`
        read-back, soft leg if the gate is open, alpha leg, photometric leg against the zeroed ground truth, clean / statistics /
        colour rules + densification, photometric step under TrainerDNG's re-layout rule.  The patch sizes of a leg are drawn
        only when it runs, by the loop's one RNG, hard before soft.
        Returns TrainerDNG's dict (near_pruned: always None) plus loss_alpha, ema_loss_hard, soft_gate_open (None while the
        soft leg is before its start), rule_counts, stepped["alpha"], path["alpha"]."""
        self.last_options = opt
        m = self.model
        xyz_lr = self._set_rates(iteration, opt)
        ci = self.draw_cameras(opt.seed)
        stepping = iteration < opt.iterations
        last = not stepping
        lo, hi = opt.patch_range
        patches = [None, None, None, None]
        losses, path = dict(hard=None, soft=None, alpha=None), dict(hard=None, soft=None, alpha=None)
        stepped = dict(hard=False, soft=False, alpha=False, gaussians=False, neural=False)
        kept = False    # the last iteration: a leg that ran left its gradient behind
        if iteration > opt.hard_depth_start:
            patches[0], patches[1] = self._rng.randint(lo, hi), self._rng.randint(lo, hi)
            losses["hard"], path["hard"] = self._depth_leg(ci, "means", patches[0], patches[1], 0.0, opt, stepping)
            stepped["hard"] = stepping
            kept = last
            self.ema_loss_hard = opt.ema[0] * float(losses["hard"]) + opt.ema[1] * self.ema_loss_hard   # (the read-back)
        gate = None
        if iteration > opt.soft_depth_start:
            gate = self.ema_loss_hard < opt.soft_gate
            if gate:
                patches[2], patches[3] = self._rng.randint(lo, hi), self._rng.randint(lo, hi)
                losses["soft"], path["soft"] = self._depth_leg(ci, "opacity", patches[2], patches[3], 0.0, opt, stepping,
                                                               keep_grads=kept)
                stepped["soft"] = stepping
                kept = last
        if opt.alpha_leg:
            fields = ("opacity",) if not (last and losses["hard"] is not None) else ("xyz", "opacity")
            losses["alpha"], path["alpha"] = self._depth_leg(ci, "opacity", None, None, 0.0, opt, True, leg="alpha",
                                                             keep_grads=kept, step_fields=fields)
            stepped["alpha"] = True
        self._rule_counts = None
        pkg, loss = self._photometric_leg(ci, opt)
        cleaned, densified, _ = self._after_photometric(iteration, opt, pkg, stepping, stepped)
        return dict(loss=loss.detach(), loss_hard=losses["hard"], loss_soft=losses["soft"], loss_alpha=losses["alpha"], camera=ci,
                    patches=tuple(patches), xyz_lr=xyz_lr, stepped=stepped, densified=densified, near_pruned=None, cleaned=cleaned,
                    P=m.P, path=path, ema_loss_hard=self.ema_loss_hard, soft_gate_open=gate, rule_counts=self._rule_counts)

    def checkpoint(self):
        state = super().checkpoint()
        state["ema_loss_hard"] = float(self.ema_loss_hard)
        return state

    def restore(self, state):
        super().restore(state)
        self.ema_loss_hard = float(state.get("ema_loss_hard", 0.0))


# ----------------------------------------------------------------------------------------------------------------
# DNGaussian on NeRF-synthetic: DNGaussian/train_blender.py:41-235 (`training`) and :240-395 (`training_sh`)
# ----------------------------------------------------------------------------------------------------------------
class DngBlenderOptions(DngOptions):
    """DngOptions with what train_blender.py hard-codes: the patch range, depth legs every tenth iteration and only before
    densify_until_iter, no smoothness term, no near-camera prune, the white-background mask's threshold, the white rule
    (threshold, opacity factor) or None, the regulariser's decay after densify_until_iter, the height prune (a threshold on the
    last coordinate, or None), and for the SH loop (`use_sh`) the plain 3DGS densification's prune opacity and size threshold
    and the opacity reset at densify_from_iter."""

    def __init__(self, **kw):
        super().__init__()
        self.patch_range = (5, 17)                  # train_blender.py:64, :263
        self.smooth_start = None                    # no smoothness term at any iteration
        self.near_prune_interval = None             # no spiral cameras, no near-camera prune
        self.near_prune_start = None
        self.white_background = True                # run_blender.sh: every scene
        self.depth_leg_interval = 10                # :90, :116, :289: iteration % 10 == 0, and iteration < densify_until_iter
        self.bg_threshold = 254 / 255               # :87, :286
        self.white_rule = (253 / 255, 0.1)          # :208-211, :367-370
        self.reg_decay = 0.1                        # :168-169: iteration > densify_until_iter
        self.height_prune = None                    # :215-218, :372-375: ship -0.5, hotdog -0.2
        self.use_sh = False                         # --use_SH: training_sh (TrainerDNGBlenderSH)
        self.prune_opacity = 0.005                  # :363 (SH loop; the neural loop takes --prune_threshold = min_opacity)
        self.size_threshold = 20                    # :362 (SH loop), after opacity_reset_interval
        self.reset_at_densify_from = True           # :378 (SH loop): dataset.white_background and iteration == densify_from_iter
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)

    SETTINGS = {   # scripts/run_blender.sh, its three settings as plain options
        1: dict(use_sh=False, iterations=6000, lambda_dssim=0.2, densify_grad_threshold=0.0005, min_opacity=0.01,
                densify_until_iter=6000, densify_from_iter=500, position_lr_final=0.0000016, position_lr_max_steps=1000,
                position_lr_start=5000, hard_depth_start=0, soft_depth_start=9999999, split_opacity_thresh=0.1,
                error_tolerance=0.001, shape_pena=0.0, opa_pena=0.0, scale_pena=0.0, clean_iterations=[1000, 2000, 3000, 4500, 6000, 1]),
        2: dict(use_sh=True, iterations=6000, lambda_dssim=0.2, densify_grad_threshold=0.0005, min_opacity=0.005,
                densify_until_iter=6000, densify_from_iter=500, position_lr_final=0.0000016, position_lr_max_steps=1000,
                position_lr_start=5000, hard_depth_start=0, error_tolerance=0.01, shape_pena=0.0, opa_pena=0.0, scale_pena=0.0,
                clean_iterations=[1000, 2000, 3000, 4500, 6000, 1]),
        3: dict(use_sh=True, iterations=30000, lambda_dssim=0.2, densify_grad_threshold=0.0002, min_opacity=0.005,
                densify_until_iter=15000, densify_from_iter=500, position_lr_final=0.0000016, position_lr_max_steps=30000,
                position_lr_start=0, hard_depth_start=99999, error_tolerance=0.2, shape_pena=0.0, opa_pena=0.0, scale_pena=0.0,
                clean_iterations=[1000, 2000, 3000, 4500, 6000, 1]),
    }
    SCENES = dict(drums=1, materials=1, ship=2, lego=2, ficus=2, hotdog=2, chair=3, mic=3)

    @classmethod
    def for_scene(cls, name, **kw):
        """scripts/run_blender.sh for one of the eight NeRF-synthetic scenes (the script tests `$dataset =~ name`, so a path
        that contains the name will do): which loop, thresholds, learning-rate schedule, depth-leg starts, tolerance,
        penalties, iterations - and train_blender.py's own scene tests: ship and hotdog prune below a height, chair skips the
        white rule in the SH loop.  (--scaling_lr 0.005 and --position_lr_init 0.00016 are the model's own rates;
        --percent_dense 0.01 its own constant.)"""
        name = str(name)
        hits = [k for k in cls.SCENES if k in name]
        if not hits:
            raise ValueError("for_scene: %r names none of %s" % (name, ", ".join(sorted(cls.SCENES))))
        o = dict(cls.SETTINGS[cls.SCENES[hits[0]]])
        if "ship" in name:
            o.update(height_prune=-0.5)
        if "hotdog" in name:
            o.update(height_prune=-0.2)        # (a path naming both: the script prunes twice, the higher threshold decides)
        if "chair" in name and o["use_sh"]:
            o.update(white_rule=None)
        o.update(kw)
        return cls(**o)


def _legs_due(iteration, opt):
    return iteration < opt.densify_until_iter and iteration % opt.depth_leg_interval == 0


def _blender_targets(trainer, depth_mono, opt, background_mask):
    """per camera, once: the white-background mask of the ground truth and the depth legs' target 255 - mono, zero under it
    (they depend on the inputs alone; the reference forms them again in every leg) -> (masks, targets [1,1,H,W])"""
    dev = trainer.model.flat.device
    masks, targets = [], []
    with torch.no_grad():
        for gt, d in zip(trainer.gts, depth_mono):
            stored = torch.as_tensor(d, dtype=torch.float32).to(dev).contiguous()
            mask, target = background_mask(torch.as_tensor(gt, dtype=torch.float32).to(dev).contiguous(), opt.bg_threshold,
                                           mono=stored)
            masks.append(mask)
            targets.append(target.reshape(1, 1, *stored.shape[-2:]))
    return masks, targets


def _height_prune(trainer, opt):
    """train_blender.py:215-218: prune_points(get_xyz[:, -1] < h) - the mask is one torch comparison, no stall"""
    if opt.height_prune is None:
        return None
    m = trainer.model
    return m.prune_points(m.params["xyz"].detach()[:, -1] < opt.height_prune, on_device=bool(opt.densify_on_device))


class TrainerDNGBlender(TrainerDNG):
    """The neural loop of DNGaussian/train_blender.py:66-228 (`training`) in its order - TrainerDNG's with what the Blender
    script changes for a white background:

      target     per camera, once (:87, :96-97): the background mask gt.min(0) > bg_threshold and the mono target
                 255 - depth_mono with the masked pixels zero.  The depth IMAGE is not masked;
      hard / soft legs   only on iterations divisible by depth_leg_interval and below densify_until_iter (inside their start
                 bounds); no smoothness term; a leg's patch sizes are drawn only when it runs, hard before soft;
      photometric  TrainerDNG's, the regulariser times reg_decay once iteration > densify_until_iter (a torch multiply on the
                 0-d term, as the reference writes it);
      white rule in front of every densification (:207-211), on the per-Gaussian colour of THIS iteration's photometric
                 render (nothing has stepped since: the reference's second render gives the same tensor): statistic zeroed,
                 raw opacity to inverse_sigmoid(factor sigmoid(opacity)); then densify_and_prune_dng; then the height prune.
    No near-camera prune.  The last iteration steps nothing.  `clean_views` resolves to the script's SECOND definition (through
    render_sh) in both loops; only `radii > 0` is read from it, which no colour reaches: prune_unseen through render_dng is
    the same mask.

    background_mask / white_rule: the new pieces as callables for models that are not on the GPU (defaults:
      gsplat_amd.dng_blender's).  opt: the DngBlenderOptions whose bg_threshold forms the masks (default: its defaults).
      bg defaults to white.
    train_iteration's dict gains rule_count (the device count of a densifying iteration, else None) and height_pruned.
    Everything closed to TrainerDNG is closed here."""

    def __init__(self, model, cameras, gt_images, depth_mono, opt=None, background_mask=None, white_rule=None, bg=None, **kw):
        if bg is None:
            bg = torch.ones(3, dtype=torch.float32, device=model.flat.device)
        if background_mask is None or white_rule is None:
            from . import dng_blender
            background_mask = background_mask or dng_blender.blender_background_mask
            white_rule = white_rule or dng_blender.white_rule
        self._white_rule, self._background_mask = white_rule, background_mask
        self._target_options = DngBlenderOptions() if opt is None else opt
        super().__init__(model, cameras, gt_images, depth_mono, bg=bg, **kw)
        self._rule_count = self._height_pruned = None

    def _mono_targets(self, depth_mono, dev):
        self.bg_masks, targets = _blender_targets(self, depth_mono, self._target_options, self._background_mask)
        return targets

    def _near_prune_due(self, iteration, opt):
        return False

    def _before_densify(self, iteration, opt, pkg):
        self._rule_count = None
        if opt.white_rule is None:
            return
        m = self.model
        thr, factor = opt.white_rule
        self._rule_count = self._white_rule(pkg["color"].detach(), m.xyz_gradient_accum, m.params["opacity"].detach(), thr, factor)

    def _after_densify(self, iteration, opt):
        self._height_pruned = _height_prune(self, opt)

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of train_blender.py:66-228 in its order.  Returns TrainerDNG's dict (near_pruned: always
        None) plus rule_count and height_pruned."""
        self.last_options = opt
        m = self.model
        xyz_lr = self._set_rates(iteration, opt)
        ci = self.draw_cameras(opt.seed)
        stepping = iteration < opt.iterations
        lo, hi = opt.patch_range
        patches = [None, None, None, None]
        losses, path = dict(hard=None, soft=None), dict(hard=None, soft=None)
        stepped = dict(hard=False, soft=False, gaussians=False, neural=False)
        due = _legs_due(iteration, opt)
        for k, (name, kind, start) in enumerate((("hard", "means", opt.hard_depth_start), ("soft", "opacity", opt.soft_depth_start))):
            if due and iteration > start:
                patches[2 * k] = self._rng.randint(lo, hi)
                patches[2 * k + 1] = self._rng.randint(lo, hi)
                losses[name], path[name] = self._depth_leg(ci, kind, patches[2 * k], patches[2 * k + 1], 0.0, opt, stepping)
                stepped[name] = stepping
        self._rule_count = self._height_pruned = None
        pkg, loss = self._photometric_leg(ci, opt, reg_scale=opt.reg_decay if iteration > opt.densify_until_iter else None)
        cleaned, densified, _ = self._after_photometric(iteration, opt, pkg, stepping, stepped)
        return dict(loss=loss.detach(), loss_hard=losses["hard"], loss_soft=losses["soft"], camera=ci, patches=tuple(patches),
                    xyz_lr=xyz_lr, stepped=stepped, densified=densified, near_pruned=None, cleaned=cleaned, P=m.P, path=path,
                    rule_count=self._rule_count, height_pruned=self._height_pruned)


def render_dng_sh(viewpoint_camera, pc, Rasterizer, Settings, bg_color, scaling_modifier=1.0, debug=False):
    """= render_sh() of DNGaussian/gaussian_renderer/__init__.py:285-367: the FSGS-generation rasterizer with the model's SH rows
    -> {render, depth, alpha, viewspace_points, visibility_filter, radii, opacity}; the image is NOT clamped.  The reference's
    "color" key (the per-Gaussian colour, evaluated in Python on every call and read only by the white rule) is not formed
    here: dng_blender.white_rule_sh evaluates it inside its kernel when the rule runs and hands it back."""
    xyz = pc.get_xyz
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    opacity = pc.get_opacity
    rs = _settings_of(Settings, viewpoint_camera, bg_color, pc.active_sh_degree, xyz.shape[0], scaling_modifier, debug)
    image, radii, depth, alpha = Rasterizer(raster_settings=rs)(
        means3D=xyz, means2D=screenspace_points, shs=pc.get_features, colors_precomp=None, opacities=opacity,
        scales=pc.get_scaling, rotations=pc.get_rotation, cov3D_precomp=None)
    return {"render": image, "depth": depth, "alpha": alpha, "viewspace_points": screenspace_points,
            "visibility_filter": radii > 0, "radii": radii, "opacity": opacity}


class TrainerDNGBlenderSH(TrainerDNG):
    with_neural = False

    """The SH loop of DNGaussian/train_blender.py:265-388 (`training_sh`) in its order, one GPU: a plain SH model, no neural
    renderer, no soft leg, no regulariser.

      SH ramp    oneupSHdegree every sh_increase_interval (1000) iterations;
      hard leg   as TrainerDNGBlender's (the depth-only pass at opacity 0.95, the zeroed target, Adam on `xyz` ONLY);
      photometric  render_dng_sh, L1 + lambda_dssim (1 - SSIM), backward, then - un-fused - Adam on every group;
      densification  the plain 3DGS rule, densify_and_prune(max_grad, prune_opacity, extent, size_threshold after
                 opacity_reset_interval);  AFTER it the white rule through white_rule_sh on the re-laid-out model with this
                 camera's centre (the statistic it zeroes has just been zeroed by the re-layout; the opacity edit is what a
                 user's model shows), then the height prune;
      reset_opacity()  every opacity_reset_interval and, for a white background, at densify_from_iter - there WITHOUT a
                 densification: only the opacity group's step is cancelled and its moments zeroed.
    A re-layout cancels the step of every group, as in the siblings.  The last iteration steps nothing.
    start_checkpoint: `training_sh` calls gaussians.load_shape, which no class of the reference defines - starting the SH loop
      from a (neural) checkpoint cannot work there and is refused here.
    background_mask / white_rule_sh / depth_loss: callables for models that are not on the GPU (defaults:
      gsplat_amd.dng_blender's and depth_norm.depth_regulariser).  Everything closed to TrainerDNG is closed here."""

    def __init__(self, model, cameras, gt_images, depth_mono, opt=None, bg=None, Rasterizer=None, Settings=None, criterion=None,
                 depth_loss=None, background_mask=None, white_rule_sh=None, opacity_lr=0.05, lambda_dssim=0.2, depth_limit=None,
                 fused_step=False, side_launch=False, start_checkpoint=None, **kw):
        if start_checkpoint is not None:
            raise RuntimeError("TrainerDNGBlenderSH: train_blender.py's training_sh restores a checkpoint through "
                               "gaussians.load_shape, which no class of the reference defines; starting the SH loop from a "
                               "neural checkpoint is refused")
        if background_mask is None or white_rule_sh is None:
            from . import dng_blender
            background_mask = background_mask or dng_blender.blender_background_mask
            white_rule_sh = white_rule_sh or dng_blender.white_rule_sh
        self._white_rule_sh, self._background_mask = white_rule_sh, background_mask
        self._target_options = DngBlenderOptions(use_sh=True) if opt is None else opt
        if bg is None:
            bg = torch.ones(3, dtype=torch.float32, device=model.flat.device)
        super().__init__(model, cameras, gt_images, depth_mono, bg=bg, Rasterizer=Rasterizer, Settings=Settings, criterion=criterion,
                         depth_loss=depth_loss, opacity_lr=opacity_lr, lambda_dssim=lambda_dssim, depth_limit=depth_limit,
                         fused_step=fused_step, side_launch=side_launch, **kw)
        self.last_colour = None   # the per-Gaussian colour of the last white rule (render_sh's "color"), or None

    _mono_targets = TrainerDNGBlender._mono_targets

    def _render(self, cam, activations=None):
        return render_dng_sh(cam, self.model, self.Rasterizer, self.Settings, self.bg)

    def train_iteration(self, iteration, opt):
        """One iteration (1-based) of train_blender.py:265-388 in its order.  Returns dict(loss, loss_hard, camera, patches
        (hard local, hard global; None when the leg did not run), xyz_lr, sh_degree, stepped = dict(hard, gaussians, opacity),
        densified (3DGS's 3-tuple or None), rule_count (device count or None), height_pruned, cleaned, reset, P, path)."""
        self.last_options = opt
        m, o = self.model, self.model.optimizer
        xyz_lr = m.update_learning_rate(max(iteration - opt.position_lr_start, 0), opt.position_lr_final, opt.position_lr_delay_mult,
                                        opt.position_lr_max_steps)
        o.lr["opacity"] = opt.opacity_lr
        if iteration % opt.sh_increase_interval == 0:
            m.oneupSHdegree()
        ci = self.draw_cameras(opt.seed)
        cam = self.cameras[ci]
        stepping = iteration < opt.iterations
        lo, hi = opt.patch_range
        patches, loss_hard, path = [None, None], None, None
        stepped = dict(hard=False, gaussians=False, opacity=False)
        if iteration > opt.hard_depth_start and _legs_due(iteration, opt):
            patches = [self._rng.randint(lo, hi), self._rng.randint(lo, hi)]
            loss_hard, path = self._depth_leg(ci, "means", patches[0], patches[1], 0.0, opt, stepping)
            stepped["hard"] = stepping
        m.zero_grad()
        pkg = self._render(cam)
        loss, l1, ssim_value = self.criterion.photometric(pkg["render"], self.gts[ci], l1_weight=1.0)
        loss.backward()
        if self.after_backward is not None:
            self.after_backward("photometric", self)
        self.last = dict(loss=loss.detach(), radii=pkg["radii"], parts=dict(l1=l1.detach(), ssim=ssim_value.detach()), path="unfused")
        self.last_radii = pkg["radii"]
        cleaned = densified = rule_count = height_pruned = None
        relayout = reset = False
        with torch.no_grad():
            m.collect_grads()
            clean = iteration in opt.clean_iterations
            if clean:
                cleaned = self.prune_unseen(opt=opt)
                relayout = True
            if iteration < opt.densify_until_iter and not clean:
                m.update_view_statistics(pkg["radii"], pkg["viewspace_points"].grad)
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    thr = opt.size_threshold if iteration > opt.opacity_reset_interval else None
                    densified = self._densify(iteration, opt, opt.prune_opacity, thr, rule="3dgs")
                    if opt.white_rule is not None:
                        rule_thr, factor = opt.white_rule
                        rule_count, self.last_colour = self._white_rule_sh(
                            m.params["xyz"].detach(), m.params["features"].detach(), m.active_sh_degree, cam.camera_center,
                            m.xyz_gradient_accum, m.params["opacity"].detach(), rule_thr, factor, return_colour=True)
                    height_pruned = _height_prune(self, opt)
                    relayout = True
                if iteration % opt.opacity_reset_interval == 0 or (
                        opt.white_background and opt.reset_at_densify_from and iteration == opt.densify_from_iter):
                    m.reset_opacity()
                    reset = True
            if stepping and not relayout:
                o.step(skip=("opacity",) if reset else ())
                stepped["gaussians"], stepped["opacity"] = True, not reset
            m.zero_grad()
        return dict(loss=loss.detach(), loss_hard=loss_hard, camera=ci, patches=tuple(patches), xyz_lr=xyz_lr,
                    sh_degree=m.active_sh_degree, stepped=stepped, densified=densified, rule_count=rule_count,
                    height_pruned=height_pruned, cleaned=cleaned, reset=reset, P=m.P, path=path)

    def checkpoint(self):
        """Trainer.checkpoint() plus the loop's RNG and camera stack"""
        state = Trainer.checkpoint(self)
        state["rng"] = None if self._rng is None else self._rng.getstate()
        state["stack"] = list(self._stack)
        return state

    def restore(self, state):
        """the inverse of checkpoint() - of THIS loop's checkpoints; one that carries a neural renderer is the other loop's"""
        import random
        if "neural" in state:
            raise RuntimeError("TrainerDNGBlenderSH: a neural checkpoint (the reference would go through load_shape, which no class "
                               "defines) is refused")
        self.model.restore(state)
        if state.get("rng") is not None:
            self._rng = random.Random()
            self._rng.setstate(state["rng"])
        self._stack = list(state["stack"])


# ----------------------------------------------------------------------------------------------------------------
# hipGraph replay of the steady-state single-GPU step
# ----------------------------------------------------------------------------------------------------------------
def _status_check(tag, num_rendered, overflow, trunc_failed):
    """include/gsplat.h GS_STATUS_CHECK"""
    m = 0xFFFFFFFF
    return (((tag & m) * 2654435761) & m) ^ (((num_rendered & m) * 40503) & m) ^ ((overflow << 30) & m) ^ ((trunc_failed << 31) & m) \
        ^ 0x5bd1e995


class GraphedStep:
    """Captures the train step of a Trainer (forward, fused criterion, gs_backward_step) into hipGraphs - ONE PER CAMERA -
    and replays them: the kernel launches of a step, their Python glue and the forward's host wait become one graph launch.
    Everything that belongs to a camera is baked into its own graph - matrices, ground truth, patch mask, the criterion's
    per-camera accumulator and the backend's per-camera tile order and depth limits (the same entry the eager step of that
    camera uses, RasterBackend.camera_entry, read and rewritten in place by the captured kernels) - so a replay copies
    nothing: only Adam's step-dependent constants (`coef`, GsStepState.coef_dev) and the replay's tag are uploaded.  (One
    graph fed through static buffers copied the 25 MB ground truth and a dozen small tensors per replay: 35 us of a 1.1 ms
    step at 1080p, most of a C1 step.)  The graphs share one memory pool: replays run one at a time on one stream and no
    intermediate outlives its replay.
    Everything frozen at capture is checked before a replay (model buffers, image size, field of view, active SH degree,
    the camera's tensors, the binning capacity); when it no longer holds the camera is captured again.  A view that needs
    more binning capacity than was captured, or whose depth limits failed, did nothing on the device (gs_backward_step
    skips on either flag): the step is then taken eagerly (settle).  SINGLE-THREADED by contract: while a capture is open
    nothing else in the process may free device memory (the cyclic collector is fenced in _capture; a tensor another thread
    drops by refcount is not).  Results are those of the eager fused step: same
    kernels, same arguments."""

    def __init__(self, trainer, capacity_margin=1.5, warmup=3, capacity=None):
        """capacity: binning capacity (instances) to capture with; default = capacity_margin x the largest view the
        backend has seen recently.  warmup: un-captured steps before the FIRST capture (allocator and library state
        settle); every later camera takes one."""
        if isinstance(trainer, TrainerFSGS):
            raise RuntimeError("GraphedStep (hipGraph replay) is closed to the FSGS rasterizer generation's trainer")
        if isinstance(trainer, TrainerDNG):
            raise RuntimeError("GraphedStep (hipGraph replay) is closed to DNGaussian's trainer")
        self.tr = trainer
        trainer._graphed = self   # Trainer.sync() settles the last replay too
        self.fixed_capacity = capacity
        self.capacity_margin = capacity_margin
        self.warmup = warmup
        self.graphs = {}          # camera index -> dict(graph, key, loss, rm_before)
        self.pool = None
        self.capacity = None
        self.coef = None
        self.replays = self.eager_steps = self.captures = 0
        self.fail_kinds = {"limits": 0, "capacity": 0}   # why replays had to be repeated eagerly
        self._replay_pending = None
        self.s_loss = None

    # (compatibility: "is anything captured", the key of the last camera stepped)
    @property
    def graph(self):
        return next(iter(self.graphs.values()))["graph"] if self.graphs else None

    # -- what a capture froze
    def _key(self, ci):
        tr = self.tr
        m, cam = tr.model, tr.cameras[ci]
        mask = None if tr.masks is None else tr.masks[ci]
        # m.generation: a re-layout / restore / load_ply with the SAME number of Gaussians still replaces every buffer the
        # captured kernels point into; the statistic tensors are re-created by densify_and_prune on their own
        return (m.P, m.generation, m.denom.data_ptr(), m.max_radii2D.data_ptr(), m.xyz_gradient_accum.data_ptr(),
                m.active_sh_degree, int(cam.image_height), int(cam.image_width), float(cam.FoVx), float(cam.FoVy),
                cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(), cam.camera_center.data_ptr(),
                tr.gts[ci].data_ptr(), None if mask is None else mask.data_ptr(), self.capacity, bool(tr.depth_limit),
                self._entry_ptrs(ci), self._backend().rows_epoch,
                m.optimizer.dormant_flags().data_ptr() if m.optimizer.USE_DORMANT else None)

    def _entry_ptrs(self, ci):
        """The addresses a capture of camera `ci` bakes in from the backend's per-camera entry (tile order, depth limits,
        slack): the entry the backend holds NOW - should it ever be replaced, the key changes and the camera is captured again."""
        ent = self.camera_entry(ci)
        return None if ent is None else (ent["order"].data_ptr(), ent["limit"].data_ptr(), ent["slack"].data_ptr())

    def _drop_graph(self, ci):
        g = self.graphs.pop(ci, None)
        if g is not None and g.get("entry") is not None:
            g["entry"]["pinned"] = max(0, g["entry"].get("pinned", 0) - 1)

    def _drop_all_graphs(self):
        for ci in list(self.graphs):
            self._drop_graph(ci)

    def _backend(self):
        tr = self.tr
        be = getattr(getattr(getattr(tr.Rasterizer, "_fn", None), "_impl", None), "backend", None)
        return be

    def camera_entry(self, ci):
        """The backend's per-camera state (tile order, depth limits) of camera `ci` - shared with the eager step."""
        tr = self.tr
        cam = tr.cameras[ci]
        return self._backend().camera_entry(int(cam.image_width), int(cam.image_height), camera_key=("trainer", tr.uid, ci),
                                            device_index=tr.model.flat.device.index)

    def _shared_init(self, dev):
        be = self._backend()
        self.coef = torch.zeros((15,), dtype=torch.float32, device=dev)
        self.coef_host = torch.zeros((15,), dtype=torch.float32).pin_memory()
        be._pinned_by_device.setdefault((dev.index, "static"), torch.zeros((16,), dtype=torch.int32).pin_memory())
        # the replay's identity: uploaded before every replay, copied out with the status words by the captured
        # gs_forward_status (GsScratch.step_tag) - the host polls the pinned block for it instead of draining the stream
        self.s_tag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.tag_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
        self._tag = 0
        self._tag_event = None
        self._coef_event = None
        crit = self.tr.criterion
        if getattr(crit, "dwt_running_mean", None) is None and hasattr(crit, "dwt_running_mean"):
            crit.dwt_running_mean = torch.ones((1,), dtype=torch.float32, device=dev)

    def _one_step(self, ci):
        """One step of camera `ci` in the capture-safe form (fixed capacity, no host wait, constants from `coef`)."""
        tr, be = self.tr, self._backend()
        be.static_capacity = self.capacity
        be.static_step_tag = self.s_tag
        be.depth_limit_request = "graph" if tr.depth_limit else None
        tr._coef_dev = self.coef
        try:
            return tr._step_camera(ci, True, ())
        finally:
            be.static_capacity = None
            be.static_step_tag = None
            be.depth_limit_request = None
            tr._coef_dev = None

    def _capture(self, ci):
        import gc
        tr, be = self.tr, self._backend()
        m = tr.model
        dev = m.flat.device
        if self.coef is None:
            self._shared_init(dev)
        first = not self.graphs
        if first or self.capacity is None:
            # binning capacity: the largest view seen so far with head-room (one number for every camera's graph)
            self.capacity = int(self.fixed_capacity) if self.fixed_capacity is not None else \
                int(max(be._capacity_hint, 4096) * self.capacity_margin)
        crit = tr.criterion
        opt = m.optimizer
        counters = (opt.t, dict(opt.seg_steps))
        rm0 = None if getattr(crit, "dwt_running_mean", None) is None else crit.dwt_running_mean.clone()
        # warm-up on a side stream, then capture; every one of these runs is a real train step of camera `ci`: counters
        # and parameters advance as in eager mode.  The first capture settles allocator and library state; a later camera
        # takes one un-captured step, which creates what a step creates lazily per camera (the backend's entry, the
        # criterion's accumulator - nothing may come from host memory inside a capture) and gives the capture a tile-order
        # hint to bake in.
        n_warm = max(1, self.warmup) if first else 1
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(n_warm):
                self._coef_for_next()  # (_step_camera's fused_request advances the counters itself)
                self._one_step(ci)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        fits = self._view_ok(be)
        if fits:   # the warm-up steps happened: what a failed first replay has to put back is the state after them
            counters = (opt.t, dict(opt.seg_steps))
            rm0 = None if rm0 is None else crit.dwt_running_mean.clone()
        if fits:
            # A cyclic-garbage sweep INSIDE the capture may free tensors of an earlier capture's pool (autograd contexts are
            # cycles) - a device free while the stream is capturing aborts the process.  So: this camera's old graph goes
            # first, garbage is collected now, and the collector stays off until the capture has ended.
            self._drop_graph(ci)
            gc.collect()
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            self._coef_for_next()
            if opt.USE_DORMANT:
                opt.dormant_flags()   # (derived from the moments by torch kernels: now, not inside the capture)
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph, pool=self.pool):
                    loss = self._one_step(ci)
            finally:
                if gc_was_on:
                    gc.enable()
            if self.pool is None:
                self.pool = graph.pool()
            rm_before = (tr.last.get("parts") or {}).get("running_mean_before")  # (a view of the captured output)
            # the capture itself launched nothing: replay once so that this call ends with a step
            self._upload_tag()
            graph.replay()
            torch.cuda.synchronize(dev)
            fits = self._view_ok(be)
        if not fits:
            # this view needs more instances than the capacity (or its depth limits were stale): none of the steps above
            # changed anything on the device (gs_backward_step skips on either flag).  Put the counters back and take ONE
            # eager step instead.
            self._invalidate(ci, be.last_status())
            opt.t, opt.seg_steps = counters[0], dict(counters[1])
            if rm0 is not None:
                crit.dwt_running_mean.copy_(rm0)
            self.eager_steps += 1
            self.s_loss = tr._step_camera(ci, True, ())
            return self.s_loss
        # the graph holds the addresses of this camera's entry: the entry is pinned (never evicted from the backend's cache)
        # and referenced from here for as long as the graph lives
        ent = self.camera_entry(ci)
        if ent is not None:
            ent["pinned"] = ent.get("pinned", 0) + 1
        self.graphs[ci] = dict(graph=graph, key=self._key(ci), loss=loss, rm_before=rm_before, entry=ent)
        self.captures += 1
        self.s_loss = loss
        return loss

    def _invalidate(self, ci, status):
        """After a step that did nothing on the device.  Limits that failed: the camera forgets them (its graph stays - the
        eager step that follows measures new ones into the same buffers).  A view that did not fit the capacity: every
        graph was captured with that capacity - all go, the next capture sizes it from the backend's grown hint."""
        num_rendered, overflow, trunc_failed = status
        self.fail_kinds["limits" if trunc_failed else "capacity"] += 1
        be = self._backend()
        ent = self.camera_entry(ci)
        if trunc_failed and ent is not None:
            ent["limit_ok"] = False
            ent["limit"].fill_(float("inf"))
            be.depth_limit_stats["failed"] += 1
            be.limits_failed(ent)     # (this camera's exported bounds get more slack: RasterBackend.SLACK)
        if overflow or num_rendered > self.capacity:
            self._drop_all_graphs()
            self.capacity = None   # (the eager step that follows grows the backend's hint; the next capture reads it)

    def _view_ok(self, be):
        num_rendered, overflow, trunc_failed = be.last_status()
        return num_rendered <= self.capacity and not overflow and not trunc_failed

    def _coef_for_next(self):
        """Constants of the step the NEXT launch performs: the launch (eager inside _one_step, or a replay) is step t + 1."""
        opt = self.tr.model.optimizer
        saved_t, saved_seg = opt.t, dict(opt.seg_steps)
        opt.begin_step(())
        coefs = torch.from_numpy(opt.step_coefficients(()))
        opt.t, opt.seg_steps = saved_t, saved_seg
        if self._coef_event is not None:
            self._coef_event.synchronize()  # the previous upload has read the pinned staging buffer
        self.coef_host.copy_(coefs)
        self.coef.copy_(self.coef_host, non_blocking=True)
        self._coef_event = torch.cuda.Event()
        self._coef_event.record(torch.cuda.current_stream(self.coef.device))

    def _upload_tag(self):
        self._tag = (self._tag + 1) & 0x7FFFFFFF
        if self._tag_event is not None:
            self._tag_event.synchronize()  # the previous upload has read the pinned word
        self.tag_host[0] = self._tag
        self.s_tag.copy_(self.tag_host, non_blocking=True)
        self._tag_event = torch.cuda.Event()
        self._tag_event.record(torch.cuda.current_stream(self.s_tag.device))

    def settle(self):
        """The verdict of the last replay (did the view fit the captured capacity, did its depth limits hold?), read from
        the status words the replay's forward copied out.  The host does not drain the stream for it: it polls the pinned
        block for the replay's tag, which arrives when the FORWARD of that replay has finished - the rest of the step is
        still queued behind it, so the GPU never waits for the host.  A failed replay changed nothing on the device
        (gs_backward_step is a no-op on either flag): counters and the criterion's running mean are put back and the step
        is taken eagerly."""
        p, self._replay_pending = getattr(self, "_replay_pending", None), None
        if p is None:
            return
        tr, be = self.tr, self._backend()
        st = be._pinned_by_device[(self.s_tag.device.index, "static")]
        spins = 0
        while int(st[8]) != p["tag"]:
            spins += 1
            if spins > 2000:  # (not there after ~2 ms of polling: wait for the stream the ordinary way)
                torch.cuda.current_stream(self.s_tag.device).synchronize()
                if int(st[8]) != p["tag"]:
                    raise RuntimeError("replay %d never delivered its status (block holds tag %d)" % (p["tag"], int(st[8])))
                break
        # The tag and the status words arrive with ONE 48-byte device-to-host copy, but nothing promises a host poller that
        # the bytes of a copy land in address order: the block is accepted when its check word (written by the same kernel
        # that wrote the tag, include/gsplat.h GS_STATUS_CHECK) matches the words read
        def read():
            w = (int(st[0]), int(st[1]), int(st[2]), int(st[8]), int(st[9]) & 0xFFFFFFFF)
            return w, w[3] == p["tag"] and w[4] == _status_check(w[3], w[0], w[1], w[2])
        seen, ok = read()
        spins = 0
        while not ok:
            spins += 1
            if spins == 2000:
                torch.cuda.current_stream(self.s_tag.device).synchronize()
            if spins > 2001:
                raise RuntimeError("replay %d delivered an inconsistent status block %r" % (p["tag"], seen))
            seen, ok = read()
        num_rendered, overflow, trunc_failed = seen[0], seen[1], seen[2]
        if num_rendered <= p["capacity"] and not overflow and not trunc_failed:
            if tr.depth_limit:
                ent = self.camera_entry(p["ci"])
                if ent is not None and ent["limit_ok"]:
                    be.limits_held(ent)
            return
        ci = p["ci"]
        self._invalidate(ci, (num_rendered, overflow, trunc_failed))
        opt = tr.model.optimizer
        opt.t -= 1
        for name in opt.seg_steps:
            opt.seg_steps[name] -= 1
        crit = tr.criterion
        if p["rm_before"] is not None:  # the criterion's running mean saw the loss of an un-rendered image
            crit.dwt_running_mean.copy_(p["rm_before"])
        self.eager_steps += 1
        self.s_loss = tr._step_camera(ci, True, ()).clone()

    def step(self, k):
        tr = self.tr
        tr.sync()
        self.settle()
        ci = tr.camera_index(k)
        be = self._backend()
        if tr._image_extras() or not tr._fused_step_ok(be, True) or be._capacity_hint <= 0 or \
                tr._depth_prior(ci) is not None:
            # what the capture cannot hold (an exposure, alpha masks or a random background - not wired into the capture -,
            # N > 1, the depth term's weight - a kernel
            # argument that changes every iteration - ...), or no view has been rendered yet to size the binning capacity from
            self.eager_steps += 1
            self.s_loss = tr._step_camera(ci, True, ())
            return self.s_loss
        g = self.graphs.get(ci)
        if g is None or g["key"] != self._key(ci):
            return self._capture(ci)
        self._coef_for_next()
        self._upload_tag()
        if tr.model.optimizer.USE_DORMANT:
            tr.model.optimizer.dormant_flags()   # (in place: the graph holds the tensor's address; a no-op while they are current)
        g["graph"].replay()
        if tr.depth_limit:
            ent = self.camera_entry(ci)
            if ent is not None and ent["limit_ok"]:
                be.depth_limit_stats["used"] += 1
        tr.model.optimizer.begin_step(())
        self.replays += 1
        self._replay_pending = dict(tag=self._tag, ci=ci, capacity=self.capacity, rm_before=g["rm_before"])
        self.s_loss = g["loss"]
        return self.s_loss

    def sync(self):
        """Settle everything that is pending (an eager deferred verdict, the last replay's): call before reading the model."""
        self.tr.sync()
        self.settle()

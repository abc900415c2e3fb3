"""`FusedAdam`: torch.optim.Adam's update (no weight decay, no amsgrad - what LGDWT-GS/scene/gaussian_model.py:192 builds:
`torch.optim.Adam(l, lr=0.0, eps=1e-15)`) as ONE streaming kernel per parameter tensor (`gs_adam_step`, csrc/gs_adam.hip:
parameter, gradient and both moments read once, parameter and moments written once) instead of torch's multi-pass
foreach implementation.  A drop-in: same constructor arguments, same param_groups / state_dict layout
(`state[p] = {"step", "exp_avg", "exp_avg_sq"}`), so the reference's optimizer surgery (cat_tensors_to_optimizer,
_prune_optimizer, replace_tensor_to_optimizer: gaussian_model.py:316-393) works on it unchanged.  Arithmetic = torch's
single-tensor Adam (tests/test_adam.py pins gs_adam_step against torch.optim.Adam).
`FusedAdam(..., fuse_groups=True)`: the same update, bit for bit, with ONE launch per 8 tensors (`gs_adam_step_tensors`).

`SparseGaussianAdam`: the optimizer class LGDWT-GS/train.py:42-46 probes for (`from diff_gaussian_rasterization import
SparseGaussianAdam`) and steps with `optimizer.step(radii > 0, radii.shape[0])` (train.py:282-284): only the rows of the
Gaussians the view saw are stepped, every tensor of up to 8 groups in ONE launch whose traffic follows those rows.  It is
exported by the opt-in packages under sparse-view-3dgs-pack_amd/accel only."""
import ctypes as C

import torch


def _check_tensor(p, what):
    """A parameter the kernels can step in place (there is no fallback): RuntimeError naming `what` otherwise."""
    if not p.is_cuda:
        raise RuntimeError("%s: the optimizer steps tensors on the GPU only - there is no fallback (got %s)" % (what, p.device))
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError("%s: the optimizer steps contiguous fp32 tensors (got %s, contiguous=%s)"
                           % (what, p.dtype, p.is_contiguous()))
    if p.data_ptr() % 16 != 0:
        raise RuntimeError("%s: the tensor does not start on a 16-byte boundary" % what)


def _gradient(p, what):
    g = p.grad
    if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
        raise RuntimeError("%s: the gradient must be a dense fp32 tensor on the parameter's device" % what)
    if not g.is_contiguous() or g.data_ptr() % 16 != 0:
        g = g.contiguous() if not g.is_contiguous() else g.clone()
    return g


def _adam_state(state, p):
    """state[p] as torch.optim.Adam creates it (the reference's optimizer surgery and state_dict() rely on the layout)."""
    st = state[p]
    if len(st) == 0:
        st["step"] = torch.tensor(0.0, dtype=torch.float32)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    return st


def _step_tensors(entries, flags, mask, P):
    """gs_adam_step_tensors over `entries` = [(p, g, state, lr, row_width, (beta1, beta2, eps))]: one call - one launch - per
    run of up to 8 entries that share their device and hyper-parameters."""
    from ._lib import hip_api
    from .capi import ADAM_MAX_TENSORS, GsAdamTensor
    api = hip_api()
    i = 0
    while i < len(entries):
        key = (entries[i][0].device, entries[i][5])
        j = i
        while j < len(entries) and j - i < ADAM_MAX_TENSORS and (entries[j][0].device, entries[j][5]) == key:
            j += 1
        table = (GsAdamTensor * (j - i))()
        for t, (p, g, st, lr, row_width, _) in zip(table, entries[i:j]):
            t.param, t.grad, t.exp_avg, t.exp_avg_sq = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            t.n, t.row_width, t.step, t.lr = p.numel(), int(row_width), int(st["step"]), float(lr)
        (b1, b2, eps) = key[1]
        api.call("adam_step_tensors", table, j - i, int(P), float(b1), float(b2), float(eps), int(flags),
                 None if mask is None else mask.data_ptr(), C.c_void_p(torch.cuda.current_stream(key[0]).cuda_stream))
        i = j


class SparseGaussianAdam(torch.optim.Adam):
    """`SparseGaussianAdam(l, lr=0.0, eps=1e-15)` (scene/gaussian_model.py:194-196) over groups of ONE tensor each.

    step(visibility, N): visibility = torch.bool / uint8 [N], one entry per Gaussian; a group's tensor has N rows of
      numel // N floats, and only the rows with visibility != 0 are stepped - the others keep every bit of the parameter and
      of both moments.  step() without arguments steps every row.  Either way ONE launch for up to 8 groups.
    bias_correction=False (default): the accelerated rasterizer's rule, p -= lr * m / (sqrt(v) + eps) - Adam's moments, NO
      bias correction.  That optimizer's source is not in the reference tree; the rule is stated from this project's review
      notes.  True: torch.optim.Adam's rule, what gsplat_amd.trainer uses for optimizer_type="sparse_adam".
    state[p] = {"step", "exp_avg", "exp_avg_sq"} as torch keeps it; `step` counts the steps a group took (the upstream class
      leaves it at 0).  Groups whose tensor has no .grad are skipped, counter included.  Nothing is loaded before the first
      step; stepping CPU, non-contiguous, non-fp32 or misaligned tensors raises RuntimeError - there is no fallback."""

    def __init__(self, params, lr, eps, betas=(0.9, 0.999), bias_correction=False):
        super().__init__(params=params, lr=lr, eps=eps, betas=betas)
        self.bias_correction = bool(bias_correction)

    @torch.no_grad()
    def step(self, visibility=None, N=None):
        if (visibility is None) != (N is None):
            raise ValueError("step(visibility, N) takes both arguments, step() none")
        todo = []
        for gi, group in enumerate(self.param_groups):
            what = "param group %r" % (group.get("name", gi),)
            if len(group["params"]) != 1:
                raise ValueError("%s: SparseGaussianAdam steps ONE tensor per group (got %d)" % (what, len(group["params"])))
            p = group["params"][0]
            if p.grad is None:
                continue
            row_width = 0
            if visibility is not None:
                N = int(N)
                if visibility.numel() != N:
                    raise ValueError("visibility has %d entries, N = %d" % (visibility.numel(), N))
                if N <= 0 or p.numel() % N != 0:
                    raise ValueError("%s: %d elements do not divide into N = %d rows" % (what, p.numel(), N))
                row_width = p.numel() // N
            todo.append((what, group, p, row_width))
        mask = None
        for what, group, p, _ in todo:   # (every rule is checked before any state changes)
            _check_tensor(p, what)
            if visibility is not None:
                if visibility.dtype not in (torch.bool, torch.uint8) or visibility.device != p.device:
                    raise RuntimeError("%s: visibility must be a torch.bool / uint8 tensor on the parameter's device" % what)
                mask = visibility.contiguous()
        entries = []
        for what, group, p, row_width in todo:
            g = _gradient(p, what)
            st = _adam_state(self.state, p)
            st["step"] += 1
            b1, b2 = group["betas"]
            entries.append((p, g, st, group["lr"], row_width, (float(b1), float(b2), float(group["eps"]))))
        if entries:
            from .capi import ADAM_NO_BIAS_CORRECTION
            _step_tensors(entries, 0 if self.bias_correction else ADAM_NO_BIAS_CORRECTION, mask, 0 if N is None else N)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, fuse_groups=False):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        from ._lib import hip_api
        from .capi import GsAdamSeg
        self._api, self._Seg = hip_api(), GsAdamSeg
        # True: every tensor of every group in one launch per 8 tensors (gs_adam_step_tensors, flags = 0) - the same bits
        self.fuse_groups = bool(fuse_groups)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.fuse_groups:
            entries = []
            for group in self.param_groups:
                b1, b2 = group["betas"]
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    _check_tensor(p, "FusedAdam")
                    st = _adam_state(self.state, p)
                    st["step"] += 1
                    entries.append((p, _gradient(p, "FusedAdam"), st, group["lr"], 0, (float(b1), float(b2), float(group["eps"]))))
            _step_tensors(entries, 0, None, 0)
            return loss
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue   # (torch skips such a parameter: moments and step count untouched)
                if not (p.is_cuda and p.is_contiguous() and p.dtype == torch.float32):
                    raise RuntimeError("FusedAdam steps contiguous fp32 tensors on the GPU")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                seg = (self._Seg * 1)()
                seg[0].begin, seg[0].end, seg[0].lr_a, seg[0].step = 0, p.numel(), float(group["lr"]), int(st["step"])
                self._api.call("adam_step", p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                               p.numel(), seg, 1, float(b1), float(b2), float(group["eps"]), int(st["step"]),
                               C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream))
        return loss


class ExposureAdam:
    """The trained exposures' optimizer (LGDWT-GS/scene/gaussian_model.py:201: `torch.optim.Adam([self._exposure])`, rate
    set by update_learning_rate) on the device: ONE launch of gs_exposure_adam per step over the whole [n,3,4] tensor.
    The surface the training loop uses - param_groups[0]["lr"], step(), zero_grad() - is torch's; on top:
      step_from_partials(partials, camera, gate): the fast step's form - the image stage's per-workgroup sums of one camera's
        gradient are added up (fixed order), written to the gradient, and the step taken, in the same launch;
      gate (device float, gs_adam_step_gated's meaning): when non-zero on the device nothing changes - the step counter is
        the caller's to restore (Trainer.sync does, with the model's).
    Arithmetic: torch's foreach Adam (lerp for the first moment, bias corrections in double, lr / bc1 as the step size);
    rows without a gradient (other cameras) take the zero gradient and move as torch moves them."""

    def __init__(self, param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        from ._lib import hip_api
        if not (param.is_cuda and param.is_contiguous() and param.dtype == torch.float32 and param.dim() == 3
                and tuple(param.shape[1:]) == (3, 4)):
            raise ValueError("ExposureAdam steps a contiguous float32 [n,3,4] tensor on the GPU")
        self.api = hip_api()
        self.param = param
        self.param_groups = [dict(params=[param], lr=lr, betas=tuple(betas), eps=eps)]
        self.exp_avg = torch.zeros_like(param)
        self.exp_avg_sq = torch.zeros_like(param)
        self.grad_buf = torch.zeros_like(param)   # what param.grad is after step_from_partials / grad_row
        self.steps = 0
        self.gate = torch.zeros((1,), dtype=torch.float32, device=param.device)   # the fused step's verdict word

    @property
    def state(self):
        return {self.param: {"step": torch.tensor(float(self.steps)), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}}

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.param.device).cuda_stream)

    def _launch(self, partials, camera, grad, step, gate):
        g = self.param_groups[0]
        self.api.call("exposure_adam", None if partials is None else partials.data_ptr(),
                      0 if partials is None else partials.numel() // 12, int(camera),
                      None if grad is None else grad.data_ptr(), None if not step else self.param.data_ptr(),
                      None if not step else self.exp_avg.data_ptr(), None if not step else self.exp_avg_sq.data_ptr(),
                      int(self.param.shape[0]), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                      int(self.steps), None if gate is None else gate.data_ptr(), self._stream())

    @torch.no_grad()
    def step(self, gate=None):
        """torch's step on param.grad (skipped, counter included, when there is none - as torch does)."""
        grad = self.param.grad
        if grad is None:
            return
        if not grad.is_contiguous():
            grad = grad.contiguous()
        self.steps += 1
        self._launch(None, 0, grad, True, gate)

    @torch.no_grad()
    def grad_row(self, partials, camera, gate=None):
        """param.grad = the gradient the partial sums of `camera` add up to (zero rows elsewhere); no step (the data-parallel
        step reduces it over ranks first)."""
        self._launch(partials, camera, self.grad_buf, False, gate)
        self.param.grad = self.grad_buf

    @torch.no_grad()
    def step_from_partials(self, partials, camera, gate=None):
        self.steps += 1
        self._launch(partials, camera, self.grad_buf, True, gate)
        self.param.grad = self.grad_buf

    def zero_grad(self, set_to_none=True):
        if set_to_none:
            self.param.grad = None
        elif self.param.grad is not None:
            self.param.grad.zero_()

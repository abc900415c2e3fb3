"""`FusedAdam`: torch.optim.Adam's update (no weight decay, no amsgrad - what LGDWT-GS/scene/gaussian_model.py:192 builds:
`torch.optim.Adam(l, lr=0.0, eps=1e-15)`) as ONE streaming kernel per parameter tensor (`gs_adam_step`, csrc/gs_adam.hip:
parameter, gradient and both moments read once, parameter and moments written once) instead of torch's multi-pass
foreach implementation.  A drop-in: same constructor arguments, same param_groups / state_dict layout
(`state[p] = {"step", "exp_avg", "exp_avg_sq"}`), so the reference's optimizer surgery (cat_tensors_to_optimizer,
_prune_optimizer, replace_tensor_to_optimizer: gaussian_model.py:316-393) works on it unchanged.  Arithmetic = torch's
single-tensor Adam (tests/test_adam.py pins gs_adam_step against torch.optim.Adam)."""
import ctypes as C

import torch


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        from ._lib import hip_api
        from .capi import GsAdamSeg
        self._api, self._Seg = hip_api(), GsAdamSeg

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
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

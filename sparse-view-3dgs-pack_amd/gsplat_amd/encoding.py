"""DNGaussian's input encoders over libgsplat_hip.so: the multi-resolution hash / tiled grid (gridencoder/grid.py,
gridencoder/src/gridencoder.cu) and the Cartesian real spherical harmonics (shencoder/sphere_harmonics.py,
shencoder/src/shencoder.cu).  fp32 only; CPU tensors raise (no fallback).

The grid's embedding gradient is the same bits on every run (a stable sort of the (slot, contribution) pairs and a
fixed-order segmented sum, csrc/gs_encoding.hip), where the reference adds one float atomic per corner and channel."""

import numpy as np
import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of


def _need_gpu(what, *tensors):
    gpu_tensors(what, tensors, dtypes=None)


def _f32(t, what):
    return gpu_tensors(what, (t,), contiguous=True)[0]


class _GridEncode(Function):
    """grid_encode(inputs [B,D] in [0,1], embeddings [n_slots,C], offsets [L+1] int32, per_level_scale,
    base_resolution, calc_grad_inputs, gridtype, align_corners, interpolation) -> [B, L*C]."""

    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False, gridtype=0,
                align_corners=False, interpolation=0):
        if inputs.shape[-1] not in (2, 3, 4, 5) or embeddings.shape[-1] not in (1, 2, 4, 8):
            # (the reference's dispatch raises this text for an unsupported D too)
            raise RuntimeError("GridEncoding: C must be 1, 2, 4, or 8.")
        _need_gpu("grid_encode", inputs, embeddings)
        inputs = inputs.float().contiguous()
        embeddings = _f32(embeddings, "grid_encode embeddings")  # (the reference casts to half under autocast; not here)
        offsets = offsets.to(device=inputs.device, dtype=torch.int32).contiguous()
        B, D = inputs.shape
        L = offsets.shape[0] - 1
        n_slots, Cdim = embeddings.shape
        S = float(np.log2(per_level_scale))
        H = int(base_resolution)
        outputs = torch.empty((B, L * Cdim), dtype=torch.float32, device=inputs.device)
        dy_dx = torch.empty((B, L * D * Cdim), dtype=torch.float32, device=inputs.device) if calc_grad_inputs else None
        hip_api().call("grid_encode_fwd", inputs.data_ptr(), B, D, embeddings.data_ptr(), n_slots, Cdim, offsets.data_ptr(),
                       L, S, H, int(gridtype), int(bool(align_corners)), int(interpolation), outputs.data_ptr(),
                       dy_dx.data_ptr() if dy_dx is not None else None, stream_of(inputs))
        ctx.save_for_backward(inputs, offsets, dy_dx)
        ctx.dims = (B, D, Cdim, L, S, H, int(gridtype), int(bool(align_corners)), int(interpolation), n_slots)
        return outputs

    @staticmethod
    def backward(ctx, grad):
        inputs, offsets, dy_dx = ctx.saved_tensors
        B, D, Cdim, L, S, H, gridtype, align_corners, interp, n_slots = ctx.dims
        grad = grad.float().contiguous()
        want_emb = ctx.needs_input_grad[1]
        want_in = dy_dx is not None and ctx.needs_input_grad[0]
        grad_embeddings = torch.empty((n_slots, Cdim), dtype=torch.float32, device=grad.device) if want_emb else None
        grad_inputs = torch.empty((B, D), dtype=torch.float32, device=grad.device) if want_in else None
        if want_emb or want_in:
            api = hip_api()
            nbytes = int(api.raw("grid_encode_tmp_bytes")(B, D, L, Cdim, n_slots)) if want_emb else 0
            tmp = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=grad.device)
            api.call("grid_encode_bwd", grad.data_ptr(), inputs.data_ptr(), B, D, n_slots, Cdim, offsets.data_ptr(), L, S,
                     H, gridtype, align_corners, interp, dy_dx.data_ptr() if want_in else None,
                     grad_embeddings.data_ptr() if want_emb else None, grad_inputs.data_ptr() if want_in else None,
                     tmp.data_ptr(), nbytes, stream_of(grad))
        return grad_inputs, grad_embeddings, None, None, None, None, None, None, None


grid_encode = _GridEncode.apply


class _SHEncode(Function):
    """sh_encode(inputs [B,3], degree, calc_grad_inputs) -> [B, degree**2]."""

    @staticmethod
    def forward(ctx, inputs, degree, calc_grad_inputs=False):
        _need_gpu("sh_encode", inputs)
        inputs = inputs.float().contiguous()
        B = inputs.shape[0]
        outputs = torch.empty((B, degree * degree), dtype=torch.float32, device=inputs.device)
        hip_api().call("sh_encode_fwd", inputs.data_ptr(), B, int(degree), outputs.data_ptr(), stream_of(inputs))
        ctx.save_for_backward(inputs)
        ctx.degree = int(degree)
        ctx.calc_grad_inputs = bool(calc_grad_inputs)
        return outputs

    @staticmethod
    def backward(ctx, grad):
        if not ctx.calc_grad_inputs:
            return None, None, None
        (inputs,) = ctx.saved_tensors
        grad = grad.float().contiguous()
        grad_inputs = torch.empty_like(inputs)
        hip_api().call("sh_encode_bwd", grad.data_ptr(), inputs.data_ptr(), inputs.shape[0], ctx.degree,
                       grad_inputs.data_ptr(), stream_of(grad))
        return grad_inputs, None, None


sh_encode = _SHEncode.apply


def grid_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners):
    """The reference's per-level table sizes (float64 numpy): min(2^log2_hashmap_size, (res or res+1)^D), rounded up
    to a multiple of 8, as the offsets list [L+1]."""
    offsets, offset = [], 0
    max_params = 2 ** log2_hashmap_size
    for i in range(num_levels):
        resolution = int(np.ceil(base_resolution * per_level_scale ** i))
        params_in_level = min(max_params, (resolution if align_corners else resolution + 1) ** input_dim)
        params_in_level = int(np.ceil(params_in_level / 8) * 8)
        offsets.append(offset)
        offset += params_in_level
    offsets.append(offset)
    return offsets

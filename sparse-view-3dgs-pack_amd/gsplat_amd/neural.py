"""DNGaussian's per-Gaussian neural heads over libgsplat_hip.so (csrc/gs_mlp.hip): the two bias-free ReLU MLPs of
scene/neural_renderer.py's GridRenderer as ONE autograd node - one fused MFMA launch forward, one (plus a fixed-order
reduction of the weight gradients) backward.

    sigma_net  enc_x [B,32] -> 64 -> 64 -> 65: column 0 = sigma, columns 1..64 = geo_feat
    color_net  [enc_d [B,16] | geo_feat] -> 64 -> 3, color = sigmoid(.) * 1.002 - 0.001

Weights in torch.nn.Linear layout [out,in].  The backward recomputes the forward, so the node saves its inputs only; no
activation reaches device memory.  fp32 and CUDA(HIP) tensors only, no CPU path.  The weight gradients are the same bits on
every run."""

import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of

# GS_DNG_* of include/gsplat.h (tests/test_dng_neural_cpu.py holds them to the header)
ENC_X = 32
ENC_D = 16
HIDDEN = 64
GEO = 64
TILE_ROWS = 128
MAX_BLOCKS = 256
WEIGHT_SHAPES = ((HIDDEN, ENC_X), (HIDDEN, HIDDEN), (1 + GEO, HIDDEN), (HIDDEN, ENC_D + GEO), (3, HIDDEN))
WEIGHT_NAMES = ("w_s0", "w_s1", "w_s2", "w_c0", "w_c1")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _check(what, enc_x, enc_d, weights):
    """Shapes are checked before devices, devices before dtypes; -> B."""
    if enc_x.dim() != 2 or enc_x.shape[1] != ENC_X:
        raise ValueError("%s: enc_x must be [B,%d], got shape %s" % (what, ENC_X, tuple(enc_x.shape)))
    if enc_d is not None and (enc_d.dim() != 2 or tuple(enc_d.shape) != (enc_x.shape[0], ENC_D)):
        raise ValueError("%s: enc_d must be [%d,%d], got shape %s" % (what, enc_x.shape[0], ENC_D, tuple(enc_d.shape)))
    for w, name, shape in zip(weights, WEIGHT_NAMES, WEIGHT_SHAPES):
        if tuple(w.shape) != shape:
            raise ValueError("%s: %s must be %s, got shape %s" % (what, name, list(shape), tuple(w.shape)))
    every = [enc_x] + ([] if enc_d is None else [enc_d]) + list(weights)
    gpu_tensors(what, every)
    return int(enc_x.shape[0])


class _Heads(Function):
    """(enc_x, enc_d or None, w_s0, w_s1, w_s2, w_c0 or None, w_c1 or None, max_blocks) -> (sigma [B], color [B,3] or None)."""

    @staticmethod
    def forward(ctx, enc_x, enc_d, w_s0, w_s1, w_s2, w_c0, w_c1, max_blocks=0):
        ctx.set_materialize_grads(False)
        full = enc_d is not None
        B = int(enc_x.shape[0])
        x = enc_x.detach().contiguous()
        d = enc_d.detach().contiguous() if full else None
        ws = [w.detach().contiguous() for w in ((w_s0, w_s1, w_s2, w_c0, w_c1) if full else (w_s0, w_s1, w_s2))]
        sigma = torch.empty((B,), dtype=torch.float32, device=x.device)
        color = torch.empty((B, 3), dtype=torch.float32, device=x.device) if full else None
        wp = [w.data_ptr() for w in ws] + [None] * (5 - len(ws))
        hip_api().call("dng_heads_fwd", x.data_ptr(), _ptr(d), B, *wp, sigma.data_ptr(), _ptr(color), int(max_blocks), stream_of(x))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, *([d] if full else []), *ws)
        ctx.full = full
        ctx.B = B
        ctx.max_blocks = int(max_blocks)
        return sigma, color

    @staticmethod
    def backward(ctx, g_sigma, g_color):
        full, B = ctx.full, ctx.B
        saved = ctx.saved_tensors
        x = saved[0]
        d = saved[1] if full else None
        ws = list(saved[2 if full else 1:])
        need = ctx.needs_input_grad
        want_x, want_d = need[0], full and need[1]
        want_w = any(need[2:5]) or (full and any(need[5:7]))
        if (g_sigma is None and g_color is None) or not (want_x or want_d or want_w):
            return (None,) * 8
        dev = x.device
        g_sigma = None if g_sigma is None else g_sigma.float().contiguous()
        g_color = None if g_color is None else g_color.float().contiguous()
        gx = torch.empty((B, ENC_X), dtype=torch.float32, device=dev) if want_x else None
        gd = torch.empty((B, ENC_D), dtype=torch.float32, device=dev) if want_d else None
        gw = [torch.empty_like(w) for w in ws] if want_w else [None] * len(ws)
        api = hip_api()
        nbytes = int(api.raw("dng_heads_tmp_bytes")(B)) if want_w else 0
        tmp = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)  # alive until the launches are enqueued
        wp = [w.data_ptr() for w in ws] + [None] * (5 - len(ws))
        gwp = [_ptr(w) for w in gw] + [None] * (5 - len(gw))
        api.call("dng_heads_bwd", x.data_ptr(), _ptr(d), B, *wp, _ptr(g_sigma), _ptr(g_color), _ptr(gx), _ptr(gd), *gwp,
                 tmp.data_ptr(), nbytes, ctx.max_blocks, stream_of(x))
        gw = gw + [None] * (5 - len(gw))
        return (gx, gd) + tuple(g if n else None for g, n in zip(gw, need[2:7])) + (None,)


def dng_heads(enc_x, enc_d, w_s0, w_s1, w_s2, w_c0, w_c1, max_blocks=0):
    """-> (sigma [B], color [B,3]): GridRenderer.forward after its two encoders.
    max_blocks > 0 caps the kernels' grids (the ABI's max_blocks: a testing aid, every workgroup then strides over several tiles)."""
    _check("dng_heads", enc_x, enc_d, (w_s0, w_s1, w_s2, w_c0, w_c1))
    return _Heads.apply(enc_x, enc_d, w_s0, w_s1, w_s2, w_c0, w_c1, max_blocks)


def dng_heads_sigma(enc_x, w_s0, w_s1, w_s2, max_blocks=0):
    """-> sigma [B]: GridRenderer.density()['sigma'] alone (geo_feat and the colour net are not evaluated)."""
    _check("dng_heads_sigma", enc_x, None, (w_s0, w_s1, w_s2))
    return _Heads.apply(enc_x, None, w_s0, w_s1, w_s2, None, None, max_blocks)[0]

"""LPIPS (VGG16, version 0.1, forward only) over libgsplat_hip.so (csrc/gs_lpips.hip): the third column of the reference's
evaluation, lpips(renders[idx], gts[idx], net_type='vgg') (LGDWT-GS/metrics.py:74, DNGaussian/metrics.py:85,
metrics_dtu.py:98), from weight files the user names.

  LpipsWeights.from_files(vgg16_path, lin_path)   torchvision's vgg16-397923af.pth and the LPIPS v0.1 vgg.pth
  LpipsWeights.from_state_dicts(vgg_sd, lin_sd)   the same from two state dicts
  lpips_vgg(render, gt, weights, ...)             a 0-d float64 device tensor (and the five per-tap terms on request)
  conv3x3_relu / maxpool2 / tap_distance          the kernels' stages on NCHW tensors
  set_default_weights / find_weights              what the drop-in package lpipsPyTorch/ uses

Nothing is ever fetched: the reference's get_state_dict downloads vgg.pth by URL on every call and torchvision downloads the
VGG16 checkpoint; here both are files.  torchvision is not a dependency: the network is restated (thirteen 3 x 3
convolutions, four pools, five taps).  The image stays in [0, 1] as the reference has it - it is NOT rescaled to [-1, 1]
(DNGaussian/metrics_dtu.py:97 remarks on this); the quirk is kept because the published numbers carry it.

No run of this code has seen the real weight files: parity is against the reference's own lpipsPyTorch module on seeded
weights (tests/golden/make_golden_lpips.py)."""
import ctypes as C
import os

import torch

from ._lib import hip_api, stream_of
from .evaluate import _check, _flags

# torchvision.models.vgg16().features: the index of each convolution, its (Cin, Cout); the taps sit after relu1_2, relu2_2,
# relu3_3, relu4_3, relu5_3 (networks.py:93: target_layers 4, 9, 16, 23, 30), a 2 x 2 pool in front of every block but the first
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_SHAPE = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
              (512, 512), (512, 512), (512, 512))
BLOCK_CONVS = (2, 2, 3, 3, 3)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIZE = 16   # below it the fifth tap is empty (torch's max_pool2d raises there too)
VGG16_FILE, LIN_FILE = "vgg16-397923af.pth", "vgg.pth"


def _entry(sd, keys, shape, what):
    """the first of `keys` that `sd` has, as a contiguous fp32 CPU tensor of `shape`"""
    for k in keys:
        if k in sd:
            t = sd[k]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
                raise ValueError("%s: key %r has shape %s, expected %s"
                                 % (what, k, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, tuple(shape)))
            return t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    raise KeyError("%s: key %s is missing" % (what, " / ".join(repr(k) for k in keys)))


class LpipsWeights:
    """The thirteen convolutions (weight [Cout,Cin,3,3], bias [Cout]) and the five lin vectors ([C]) as fp32 CPU tensors.
    Parsing needs no GPU; the upload and the kernels' repack happen on the first use on a device and are kept per device."""

    def __init__(self, conv_w, conv_b, lin):
        self.conv_w, self.conv_b, self.lin = list(conv_w), list(conv_b), list(lin)
        self._device = {}

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd):
        """vgg_sd: torchvision's keys features.{i}.weight|bias.  lin_sd: lin{k}.model.1.weight (the file's naming) or {k}.1.weight
        (after the reference's get_state_dict renamed them), [1,C,1,1].  A missing or wrong-shaped entry raises, naming the key."""
        conv_w, conv_b = [], []
        for i, (cin, cout) in zip(CONV_INDEX, CONV_SHAPE):
            conv_w.append(_entry(vgg_sd, ("features.%d.weight" % i,), (cout, cin, 3, 3), "vgg16 weights"))
            conv_b.append(_entry(vgg_sd, ("features.%d.bias" % i,), (cout,), "vgg16 weights"))
        lin = [_entry(lin_sd, ("lin%d.model.1.weight" % k, "%d.1.weight" % k), (1, c, 1, 1), "lin weights").reshape(c)
               for k, c in enumerate(TAP_CHANNELS)]
        return cls(conv_w, conv_b, lin)

    @classmethod
    def from_files(cls, vgg16_path, lin_path):
        """Two files written by torch.save: torchvision's vgg16-397923af.pth and the LPIPS repository's weights/v0.1/vgg.pth."""
        return cls.from_state_dicts(torch.load(vgg16_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True))

    def on(self, device):
        """-> (packed weights [13], biases [13], float64 lin [5], and the three host pointer arrays) on `device`"""
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("LPIPS: CUDA(HIP) device only - there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            packed = [pack_conv_weight(w.to(device)) for w in self.conv_w]
            bias = [b.to(device) for b in self.conv_b]
            lin = [v.to(device=device, dtype=torch.float64) for v in self.lin]   # (widening is exact)
            ptrs = tuple((C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) for ts in (packed, bias, lin))
            self._device[device] = (packed, bias, lin, ptrs)
        return self._device[device]


def _f32(t, what, dim):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != dim:
        raise ValueError("%s: an fp32 CUDA(HIP) tensor of %d dimensions" % (what, dim))
    return t.contiguous()


def pack_conv_weight(w):
    """[Cout,Cin,3,3] on the device -> the kernels' [Cin (4 for 3)][9][Cout]"""
    w = _f32(w, "w", 4)
    cout, cin = int(w.shape[0]), int(w.shape[1])
    n = int(hip_api().raw("lpips_packed_floats")(cin, cout)) if tuple(w.shape[2:]) == (3, 3) else 0
    if n == 0:
        raise ValueError("conv3x3: weight %s is none of VGG16's eight (Cin, Cout) pairs" % (tuple(w.shape),))
    out = torch.empty((n,), dtype=torch.float32, device=w.device)
    hip_api().call("lpips_pack_weights", w.data_ptr(), cin, cout, out.data_ptr(), stream_of(w))
    return out


def conv3x3_relu(x, w, b):
    """relu(conv2d(x, w, b, padding=1)) of x [N,Cin,H,W] with w [Cout,Cin,3,3], b [Cout] -> [N,Cout,H,W]"""
    x, b = _f32(x, "x", 4), _f32(b, "b", 1)
    packed = pack_conv_weight(w)
    N, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    if int(w.shape[1]) != cin or int(b.shape[0]) != cout:
        raise ValueError("conv3x3: x %s, w %s and b %s do not fit" % (tuple(x.shape), tuple(w.shape), tuple(b.shape)))
    y = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device)
    hip_api().call("lpips_conv3x3_relu", x.data_ptr(), packed.data_ptr(), b.data_ptr(), N, cin, cout, H, W, y.data_ptr(), stream_of(x))
    return y


def maxpool2(x):
    """max_pool2d(x, 2, 2) of [N,C,H,W]: an odd last row or column is dropped"""
    x = _f32(x, "x", 4)
    N, Cn, H, W = (int(v) for v in x.shape)
    if H < 2 or W < 2:
        raise ValueError("maxpool2: at least 2 x 2 (got %d x %d) - torch raises there too" % (H, W))
    y = torch.empty((N, Cn, H // 2, W // 2), dtype=torch.float32, device=x.device)
    hip_api().call("lpips_maxpool2", x.data_ptr(), N * Cn, H, W, y.data_ptr(), stream_of(x))
    return y


def tap_distance(fx, fy, lin):
    """One tap of lpips.py:33-34 on features [1,C,H,W] (or [C,H,W]): the channel-normalised squared difference, its product
    with lin ([C] or [1,C,1,1]), the mean over the pixels -> a 0-d float64 device tensor.  float64 from the features on."""
    fx, fy = (_f32(t[0] if t.dim() == 4 and t.shape[0] == 1 else t, "features", 3) for t in (fx, fy))
    if fx.shape != fy.shape:
        raise ValueError("tap_distance: features %s and %s differ in shape" % (tuple(fx.shape), tuple(fy.shape)))
    Cn, H, W = (int(v) for v in fx.shape)
    lin = lin.reshape(-1).to(device=fx.device, dtype=torch.float64).contiguous()
    if lin.numel() != Cn:
        raise ValueError("tap_distance: %d lin weights for %d channels" % (lin.numel(), Cn))
    api = hip_api()
    tmp = torch.empty((int(api.raw("lpips_distance_tmp_bytes")(H, W)),), dtype=torch.uint8, device=fx.device)
    out = torch.empty((1,), dtype=torch.float64, device=fx.device)
    api.call("lpips_distance", fx.data_ptr(), fy.data_ptr(), lin.data_ptr(), Cn, H, W, tmp.data_ptr(), tmp.numel(),
             out.data_ptr(), stream_of(fx))
    return out[0]


def check_size(Cn, H, W):
    if Cn < 3:
        raise ValueError("LPIPS: images of at least three channels (got %d)" % Cn)
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError("LPIPS: images of at least %d x %d (got %d x %d) - the fifth tap would be empty, torch raises there too"
                         % (MIN_SIZE, MIN_SIZE, H, W))


def tmp_bytes(H, W):
    return int(hip_api().raw("lpips_tmp_bytes")(int(H), int(W)))


def launch(render, gt, mask, Cn, H, W, flags, weights, tmp, out):
    """out (six float64 words in device memory) <- the five per-tap terms and their sum; arguments as evaluate._check left them"""
    ptrs = weights.on(render.device)[3]
    hip_api().call("lpips_vgg", render.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), Cn, H, W, int(flags),
                   ptrs[0], ptrs[1], ptrs[2], tmp.data_ptr(), tmp.numel(), out.data_ptr(), stream_of(render))


def lpips_vgg(render, gt, weights, mask=None, clamp=False, quantise=False, return_taps=False, tmp=None):
    """LPIPS of render against gt ([C,H,W] or [1,C,H,W] fp32 on the device, the first three channels are used) after the
    evaluation's pixel transform (evaluate.image_metrics: clamp, 8-bit round trip, blend to white under the DTU mask).
    -> a 0-d float64 device tensor; with return_taps also the five per-tap terms ([5] float64) whose sum it is.
    tmp: scratch of at least tmp_bytes(H, W) bytes (uint8, on the device) to reuse; allocated when missing."""
    if not isinstance(weights, LpipsWeights):
        raise ValueError("lpips_vgg: weights must be LpipsWeights (from_files / from_state_dicts), got %s" % type(weights).__name__)
    render, gt, mask, Cn, H, W = _check(render, gt, mask)
    check_size(Cn, H, W)
    if tmp is None:
        tmp = torch.empty((tmp_bytes(H, W),), dtype=torch.uint8, device=render.device)
    out = torch.empty((6,), dtype=torch.float64, device=render.device)
    launch(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), weights, tmp, out)
    return (out[5], out[:5]) if return_taps else out[5]


_default = None


def set_default_weights(weights):
    """The weights lpipsPyTorch.lpips / LPIPS use (None: look for the files again)."""
    global _default
    if weights is not None and not isinstance(weights, LpipsWeights):
        raise ValueError("set_default_weights: LpipsWeights or None")
    _default = weights


def find_weights():
    """The two files where the reference's own downloads would have put them, torch.hub.get_dir()/checkpoints - looked for,
    never fetched.  A missing file raises FileNotFoundError naming both."""
    d = os.path.join(torch.hub.get_dir(), "checkpoints")
    paths = [os.path.join(d, VGG16_FILE), os.path.join(d, LIN_FILE)]
    if not all(os.path.isfile(p) for p in paths):
        raise FileNotFoundError("LPIPS needs two weight files and never downloads them: %s (torchvision's VGG16) and %s (LPIPS "
                                "v0.1 weights/v0.1/vgg.pth).  Put them there, or load them from anywhere with "
                                "LpipsWeights.from_files and pass them on (set_default_weights)" % (paths[0], paths[1]))
    return LpipsWeights.from_files(*paths)


def default_weights():
    global _default
    if _default is None:
        _default = find_weights()
    return _default

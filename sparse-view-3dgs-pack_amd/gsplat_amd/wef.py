"""LGDWT-GS's Wavelet Error Field (utils/loss_utils.py:156-329) and Charbonnier loss (:98-101): on device tensors through
csrc/gs_wef.hip, on CPU tensors as the torch statements below, in the tensor's own dtype (float32 or float64).

  compute_wef_maps(pred, gt)          {LL2, LH2, HL2, WEF}                 [1,1,H,W] each, in [0, 1]
  compute_wef_all_subbands(pred, gt)  {LL1 .. HH1, LL2 .. HH2, COMBINED}
  make_heatmap_rgb(x01)               [N,1,H,W] -> [N,3,H,W] blue - green - red
  make_wef_grid_image(maps, keys, tile_cols=3, as_pil=False)         uint8 [rows * H, cols * W, 3]
  make_wef_grid_image_titled(maps, keys, tile_cols=3, as_pil=False)  the same with a black box and the key in every tile
  charbonnier_loss(pred, target, epsilon=1e-3)                       one autograd node

The maps: 2-level Haar bands of the signed residual pred - gt, e = mean_c(scale * b_c^2) with scale 1 at level 1, 4 for LL2 and
2 for LH2 / HL2 / HH2, upsampled bilinearly (align_corners=False) to the image, n = (u - min) / (max - min + 1e-8) per map;
the field is the mean of the maps, normalised the same way.

Where this departs from the reference:
  * one image per call ([C,H,W] or [1,C,H,W]), as the module's other functions; a batch raises ValueError
  * device tensors are float32
  * the maps carry no gradient (the inputs are detached: it is a diagnostic)
  * the grids are bytes, uint8 [rows * H, cols * W, 3] on the maps' device (gsplat_amd.imageio.write_png writes them), not a
    PIL.Image: Pillow is no dependency.  as_pil=True imports it on demand and returns the Image
  * the titled grid's labels come from a 5 x 7 bitmap font held as data (_font5x7.py: A-Z, 0-9, '_'; any other character is
    a filled box), drawn at twice its size: Pillow's default font cannot be reproduced, so the label's pixels differ from the
    reference's.  The box is the reference's, [c W, c W + 120] x [r H, r H + 26] with both corners inclusive, clipped at the
    image border; a label is cut at its box
  * the device's bilinear formula (csrc/gs_haar.h) and torch's CPU one round differently: up to 4e-7 on a map in [0, 1]
  * a plane of ONE coefficient (images of up to 4 x 4 pixels at level 2, 2 x 2 at level 1) is upsampled as that coefficient,
    so its map is exactly 0 = 0 / (0 + 1e-8).  The reference's interpolate evaluates l0 * v + l1 * v with two rounded weights
    there, and its float32 map is then that rounding noise divided by 1e-8"""
import numpy as np
import torch
import torch.nn.functional as F

from ._font5x7 import GLYPH_H, GLYPH_W, GLYPHS

LEVEL2_KEYS = ("LL2", "LH2", "HL2", "WEF")
ALL_KEYS = ("LL1", "LH1", "HL1", "HH1", "LL2", "LH2", "HL2", "HH2", "COMBINED")
BAND_SCALE = {"LL1": 1.0, "LH1": 1.0, "HL1": 1.0, "HH1": 1.0, "LL2": 4.0, "LH2": 2.0, "HL2": 2.0, "HH2": 2.0}
GS_WEF_LEVEL2, GS_WEF_ALL = 0, 1
LABEL_W, LABEL_H = 121, 27          # the reference's rectangle [0, 120] x [0, 26], corners inclusive
LABEL_OFFSET, LABEL_SCALE = 6, 2
HC = 0.7071067811865476
_device_consts = {}


# ------------------------------------------------------------------------------------------------------------- inputs
def _image(t, what):
    if not torch.is_tensor(t):
        raise ValueError("%s: expected a tensor, got %s" % (what, type(t).__name__))
    t = t.detach()
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError("%s: one image per call, [C,H,W] or [1,C,H,W] (got a batch of %d: call once per image)"
                             % (what, t.shape[0]))
        t = t[0]
    if t.dim() != 3:
        raise ValueError("%s: [C,H,W] or [1,C,H,W] (got shape %s)" % (what, tuple(t.shape)))
    return t


def _pair(pred, gt):
    p, g = _image(pred, "pred"), _image(gt, "gt")
    if p.shape != g.shape:
        raise ValueError("pred %s and gt %s must have the same shape" % (tuple(p.shape), tuple(g.shape)))
    if p.device != g.device or p.dtype != g.dtype:
        raise ValueError("pred (%s, %s) and gt (%s, %s) differ in device or dtype" % (p.device, p.dtype, g.device, g.dtype))
    C, H, W = (int(s) for s in p.shape)
    if not 1 <= C <= 4 or H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("images of 1 to 4 channels, at least 1 x 1 and fewer than 2^31 pixels (got %s)" % (tuple(p.shape),))
    if p.is_cuda:
        if p.dtype != torch.float32:
            raise ValueError("device tensors are float32 (got %s)" % p.dtype)
    elif p.dtype not in (torch.float32, torch.float64):
        raise ValueError("CPU tensors are float32 or float64 (got %s)" % p.dtype)
    return p.contiguous(), g.contiguous()


# --------------------------------------------------------------------------------------------------- torch restatement
def haar_level(x):
    """x [C,H,W] -> (LL, LH, HL, HH) [C,ceil(H/2),ceil(W/2)]: one Haar level of pytorch_wavelets.DWTForward('db1',
    'symmetric') as csrc/gs_haar.h evaluates it - along W, then along H, an odd size repeating its last sample"""
    if x.shape[-1] % 2:
        x = torch.cat((x, x[..., -1:]), dim=-1)
    if x.shape[-2] % 2:
        x = torch.cat((x, x[..., -1:, :]), dim=-2)
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    lo_t, hi_t = HC * a + HC * b, HC * a - HC * b
    lo_b, hi_b = HC * c + HC * d, HC * c - HC * d
    return HC * lo_t + HC * lo_b, HC * lo_t - HC * lo_b, HC * hi_t + HC * hi_b, HC * hi_t - HC * hi_b


def residual_bands(pred, gt):
    """-> {LL1 .. HH2} of pred - gt, [C,h,w] each"""
    l1 = haar_level(pred - gt)
    l2 = haar_level(l1[0])
    return dict(zip(ALL_KEYS[:8], l1 + l2))


def _normalize_to_01(x, eps=1e-8):
    min_v = x.amin(dim=(-2, -1), keepdim=True)
    max_v = x.amax(dim=(-2, -1), keepdim=True)
    return (x - min_v) / (max_v - min_v + eps)


def upsampled_energies(pred, gt, keys):
    """-> {key: [1,1,H,W]} before the normalisation (loss_utils.py:188-206, :300-321)"""
    H, W = pred.shape[-2:]
    bands = residual_bands(pred, gt)
    out = {}
    for k in keys:
        e = bands[k][None] * bands[k][None]
        e = e * BAND_SCALE[k]
        e = e.mean(dim=1, keepdim=True)
        if e.shape[-2:] == (1, 1):   # one coefficient: the interpolant is that coefficient (two rounded weights would blur it)
            out[k] = e.expand(1, 1, H, W).clone()
        else:
            out[k] = F.interpolate(e, size=(H, W), mode="bilinear", align_corners=False)
    return out


def wef_maps_torch(pred, gt, all_bands=False):
    """The reference's statements on [C,H,W] tensors of one dtype -> the dict of [1,1,H,W] maps"""
    keys = ALL_KEYS[:8] if all_bands else LEVEL2_KEYS[:3]
    maps = {k: _normalize_to_01(u) for k, u in upsampled_energies(pred, gt, keys).items()}
    combo = None
    for k in keys:
        combo = maps[k] if combo is None else (combo + maps[k])
    maps[ALL_KEYS[8] if all_bands else LEVEL2_KEYS[3]] = _normalize_to_01(combo / (8.0 if all_bands else 3.0))
    return maps


# --------------------------------------------------------------------------------------------------------------- device
def _api_stream(t):
    from ._lib import hip_api, stream_of
    if not t.is_cuda:  # wef_maps_device and the Charbonnier function take the stream before any check of their own
        raise ValueError("Expected a cuda device, but got: %s" % t.device)
    return hip_api(), stream_of(t)


def wef_maps_device(pred, gt, all_bands=False):
    """pred, gt contiguous float32 [C,H,W] on one device -> out [K + 1,H,W]: six launches"""
    api, stream = _api_stream(pred)
    C, H, W = (int(s) for s in pred.shape)
    bands = GS_WEF_ALL if all_bands else GS_WEF_LEVEL2
    nb = int(api.raw("wef_tmp_bytes")(C, H, W, bands))
    if nb == 0:
        raise ValueError("gs_wef_maps refuses the shape %s" % ((C, H, W),))
    tmp = torch.empty((nb,), dtype=torch.uint8, device=pred.device)
    out = torch.empty(((8 if all_bands else 3) + 1, H, W), dtype=torch.float32, device=pred.device)
    api.call("wef_maps", pred.data_ptr(), gt.data_ptr(), C, H, W, bands, tmp.data_ptr(), nb, out.data_ptr(), None, stream)
    return out


def _compute(pred, gt, all_bands):
    p, g = _pair(pred, gt)
    keys = ALL_KEYS if all_bands else LEVEL2_KEYS
    if p.is_cuda:
        out = wef_maps_device(p, g, all_bands)
        return {k: out[i][None, None] for i, k in enumerate(keys)}
    with torch.no_grad():
        return wef_maps_torch(p, g, all_bands)


def compute_wef_maps(pred, gt):
    """Wavelet Error Field of the level-2 bands -> {'LL2', 'LH2', 'HL2', 'WEF'}, [1,1,H,W] each, normalised to [0, 1]"""
    return _compute(pred, gt, False)


def compute_wef_all_subbands(pred, gt):
    """The maps of all eight sub-bands and their combined field -> {'LL1' .. 'HH2', 'COMBINED'}, [1,1,H,W] each"""
    return _compute(pred, gt, True)


def make_heatmap_rgb(x01):
    """[N,1,H,W] in [0, 1] -> [N,3,H,W]: blue -> green -> red (loss_utils.py:223-236, the same statements)"""
    x = x01.clamp(0, 1)
    r = x
    g = 1.0 - (x - 0.5).abs() * 2.0
    b = 1.0 - x
    g = g.clamp(0, 1)
    return torch.cat([r, g, b], dim=1)


# ----------------------------------------------------------------------------------------------------------------- grid
def label_mask(key):
    """-> uint8 [LABEL_H, LABEL_W]: 1 where the key's glyphs are set, drawn from (LABEL_OFFSET, LABEL_OFFSET) at LABEL_SCALE and
    cut at the box"""
    m = np.zeros((LABEL_H, LABEL_W), dtype=np.uint8)
    s = LABEL_SCALE
    x = LABEL_OFFSET
    for ch in str(key):
        rows = GLYPHS.get(ch)
        g = np.ones((GLYPH_H, GLYPH_W), dtype=np.uint8) if rows is None else \
            np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)
        g = np.kron(g, np.ones((s, s), dtype=np.uint8))
        y = LABEL_OFFSET
        h, w = max(0, min(g.shape[0], LABEL_H - y)), max(0, min(g.shape[1], LABEL_W - x))
        m[y:y + h, x:x + w] = g[:h, :w]
        x += (GLYPH_W + 1) * s
    return m


def _tiles(maps, keys):
    if len(keys) == 0:
        raise ValueError("No images for grid")
    tiles = []
    for k in keys:
        t = maps[k]
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1:
            raise ValueError("maps[%r]: expected a [N,1,H,W] tensor" % (k,))
        tiles.append(t.detach()[0, 0])
    if any(t.shape != tiles[0].shape or t.device != tiles[0].device for t in tiles):
        raise ValueError("the maps of one grid share a shape and a device")
    return tiles


def grid_numpy(tiles, tile_cols, labels=None):
    """The reference's statements on host arrays [H,W] -> uint8 [rows * H, cols * W, 3] (labels: uint8 [n,LABEL_H,LABEL_W])"""
    H, W = tiles[0].shape
    cols, rows = tile_cols, (len(tiles) + tile_cols - 1) // tile_cols
    grid = np.zeros((rows * H, cols * W, 3), dtype=np.uint8)
    for idx, t in enumerate(tiles):
        hm = make_heatmap_rgb(torch.as_tensor(t)[None, None])[0]
        with np.errstate(invalid="ignore"):
            arr = (np.nan_to_num(hm.permute(1, 2, 0).clamp(0, 1).numpy()) * 255).astype("uint8")
        r, c = idx // cols, idx % cols
        grid[r * H:(r + 1) * H, c * W:(c + 1) * W] = arr
    if labels is not None:
        for idx in range(len(tiles)):   # in key order, each box over everything before it
            r, c = idx // cols, idx % cols
            box = grid[r * H:r * H + LABEL_H, c * W:c * W + LABEL_W]
            box[...] = (labels[idx][:box.shape[0], :box.shape[1], None] != 0) * np.uint8(255)
    return grid


def _const(device, key, make):
    index = device.index if device.index is not None else torch.cuda.current_device()
    if (index, key) not in _device_consts:
        _device_consts[(index, key)] = make().to(device)
    return _device_consts[(index, key)]


def _grid(maps, keys, tile_cols, titled, as_pil):
    keys = list(keys)
    tiles = _tiles(maps, keys)
    tile_cols = int(tile_cols)
    if tile_cols < 1:
        raise ValueError("tile_cols must be at least 1 (got %d)" % tile_cols)
    labels = np.stack([label_mask(k) for k in keys]) if titled else None
    if tiles[0].is_cuda:
        api, stream = _api_stream(tiles[0])
        H, W = (int(s) for s in tiles[0].shape)
        n = len(tiles)
        stack = torch.stack([t.to(torch.float32) for t in tiles]).contiguous()
        order = _const(stack.device, ("order", n), lambda: torch.arange(n, dtype=torch.int32))
        lab = None
        if titled:
            lab = _const(stack.device, ("labels",) + tuple(str(k) for k in keys), lambda: torch.from_numpy(labels))
        rows = (n + tile_cols - 1) // tile_cols
        out = torch.empty((rows * H, tile_cols * W, 3), dtype=torch.uint8, device=stack.device)
        api.call("wef_grid", stack.data_ptr(), n, H, W, order.data_ptr(), n, tile_cols, None if lab is None else lab.data_ptr(),
                 out.data_ptr(), stream)
    else:
        out = torch.from_numpy(grid_numpy([t.numpy() for t in tiles], tile_cols, labels))
    if as_pil:
        from PIL import Image   # (ImportError where Pillow is absent: it is no dependency)
        return Image.fromarray(out.cpu().numpy())
    return out


def make_wef_grid_image(maps, keys, tile_cols=3, as_pil=False):
    """maps[key] [N,1,H,W] (the first sample is used) -> uint8 [rows * H, tile_cols * W, 3] on the maps' device: tile idx at row
    idx // tile_cols, column idx % tile_cols, unused tiles black.  as_pil=True: the PIL.Image the reference returns."""
    return _grid(maps, keys, tile_cols, False, as_pil)


def make_wef_grid_image_titled(maps, keys, tile_cols=3, as_pil=False):
    """make_wef_grid_image with a black box and the key in white at the top-left corner of every tile"""
    return _grid(maps, keys, tile_cols, True, as_pil)


# ---------------------------------------------------------------------------------------------------------- Charbonnier
class _Charbonnier(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, epsilon):
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        api, stream = _api_stream(p)
        n = p.numel()
        nb = int(api.raw("charbonnier_tmp_bytes")(n))
        tmp = torch.empty((nb,), dtype=torch.uint8, device=p.device)
        out = torch.empty((), dtype=torch.float32, device=p.device)
        api.call("charbonnier_fwd", p.data_ptr(), t.data_ptr(), n, float(epsilon), tmp.data_ptr(), nb, out.data_ptr(), stream)
        ctx.save_for_backward(p, t)
        ctx.epsilon = float(epsilon)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        p, t = ctx.saved_tensors
        api, stream = _api_stream(p)
        g = grad_out.detach().to(torch.float32).contiguous()
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        if dp is None and dt is None:
            return None, None, None
        api.call("charbonnier_bwd", p.data_ptr(), t.data_ptr(), p.numel(), ctx.epsilon, g.data_ptr(),
                 None if dp is None else dp.data_ptr(), None if dt is None else dt.data_ptr(), stream)
        return dp, dt, None


def charbonnier_loss(pred, target, epsilon=1e-3):
    """mean(sqrt((pred - target)^2 + epsilon^2)) over all dimensions: equal shapes of any rank, at least one element.  Device
    tensors (float32): one autograd node on gs_charbonnier_fwd / gs_charbonnier_bwd; CPU tensors: the reference's statements."""
    if not torch.is_tensor(pred) or not torch.is_tensor(target):
        raise ValueError("charbonnier_loss: expected two tensors")
    if pred.shape != target.shape:
        raise ValueError("pred %s and target %s must have the same shape" % (tuple(pred.shape), tuple(target.shape)))
    if pred.numel() < 1:
        raise ValueError("charbonnier_loss: at least one element")
    if pred.device != target.device:
        raise ValueError("pred on %s and target on %s" % (pred.device, target.device))
    if pred.is_cuda:
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise ValueError("device tensors are float32 (got %s, %s)" % (pred.dtype, target.dtype))
        return _Charbonnier.apply(pred, target, float(epsilon))
    diff = pred - target
    return torch.sqrt(diff * diff + (epsilon * epsilon)).mean()

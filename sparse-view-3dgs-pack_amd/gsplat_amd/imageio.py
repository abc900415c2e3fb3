"""The evaluation's image files, without Pillow or torchvision: 8-bit PNG in and out (standard library: zlib, struct),
torchvision's save_image byte rule, and PIL.Image.resize's default filter on 8-bit images, bit for bit.

  write_png / read_png    8-bit grey, grey + alpha, RGB, RGBA; non-interlaced.  16-bit, palette and interlaced files raise.
  write_png16 / read_png16  the same four colour types at 16 bits per sample (the depth priors' files, gsplat_amd/depth_priors.py)
  save_image_bytes        the uint8 [H,W,C] image torchvision.utils.save_image writes for a [C,H,W] float tensor
                          (LGDWT-GS/render.py:45-46): mul(255).add(0.5).clamp(0, 255).to(uint8), one channel written as three
  resize_u8               Image.resize((W2, H2)) of a mode-L / mode-RGB image (DNGaussian/metrics_dtu.py:37-39): the antialiased
                          bicubic of Pillow's Resample.c.  Device tensors go through gs_resize_bicubic_u8 (csrc/gs_eval_files.hip);
                          CPU tensors and numpy arrays through the same integer arithmetic in numpy.  The same bits either way.
  to_planar               torchvision's to_tensor of a decoded 8-bit image: fp32 [C,H,W] = byte / 255 (the kernel's same-size path)
  resize_alpha_u8         Image.resize((W2, H2)) of a mode-LA / mode-RGBA image: the same filter on premultiplied bytes (the rule is
                          stated above the function; tests/golden/pil_resize_alpha.npz pins it).  resize_u8 itself keeps refusing alpha
  ingest_image            a decoded image -> the camera's (original_image, alpha_mask): NeRF-synthetic's composite, the resize,
                          byte / 255, the mask (gs_image_ingest, csrc/gs_image_ingest.hip, for device tensors; gsplat_amd/scene.py)

The resize restated (tests/golden/pil_resize.npz pins it to Pillow's bytes).  Per axis, in Python floats = C doubles:
  scale = in / out, filterscale = max(scale, 1), support = 2 filterscale, ksize = 2 ceil(support) + 1
  per output sample xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
  xmax = min(int(center + support + 0.5), in), n = xmax - xmin
  w(x) = bicubic((x + xmin - center + 0.5) / filterscale) with a = -0.5, x in [0, n); summed in index order, each divided
  by the sum; fixed point int(k 2^22 + 0.5) for k >= 0, int(k 2^22 - 0.5) for k < 0
  out = clamp((2^21 + sum k p) >> 22, 0, 255), integers throughout
The horizontal pass runs first into an 8-bit intermediate, then the vertical one; a pass whose sizes agree is skipped.
Divergences from Image.resize, raised: 1 or 3 channels only (Pillow premultiplies alpha for LA / RGBA), the default filter
only, no box, no reducing_gap."""
import math
import struct
import zlib

import numpy as np
import torch

PRECISION_BITS = 22   # Resample.c: 32 - 8 - 2
_SIG = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}            # PNG colour type -> channels (3 = palette: refused)
_COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}


# ------------------------------------------------------------------------------------------------------------ PNG
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _host_u8(img, what):
    if torch.is_tensor(img):
        img = img.detach().cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError("%s: uint8 only (got %s)" % (what, img.dtype))
    return img


def png_bytes(u8, level=6):
    """uint8 [H,W], [H,W,1], [H,W,3] or [H,W,4] -> the bytes of an 8-bit, non-interlaced PNG (filter type 0 on every row)"""
    u8 = _host_u8(u8, "png_bytes")
    if u8.ndim == 2:
        u8 = u8[:, :, None]
    if u8.ndim != 3 or u8.shape[2] not in _COLOUR_TYPE or u8.shape[0] < 1 or u8.shape[1] < 1:
        raise ValueError("png_bytes: [H,W], [H,W,1], [H,W,2], [H,W,3] or [H,W,4] of at least one pixel (got %s)" % (u8.shape,))
    H, W, Cn = u8.shape
    rows = np.zeros((H, 1 + W * Cn), dtype=np.uint8)
    rows[:, 1:] = u8.reshape(H, W * Cn)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, _COLOUR_TYPE[Cn], 0, 0, 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, u8):
    """Write uint8 [H,W], [H,W,1], [H,W,2], [H,W,3] or [H,W,4] (tensor or array) as an 8-bit, non-interlaced PNG."""
    data = png_bytes(u8)   # ([H,W,2], grey + alpha, is written too)
    with open(path, "wb") as fp:
        fp.write(data)


def _unfilter(raw, H, stride, bpp):
    """The five filter types of the PNG specification, row by row -> uint8 [H, stride]"""
    out = np.zeros((H, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    pos = 0
    for y in range(H):
        ft = raw[pos]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=pos + 1)
        pos += stride + 1
        up = out[y - 1] if y else zero
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = line + up   # (uint8 arithmetic wraps: modulo 256, as the specification asks)
        elif ft == 1:   # a running sum per channel, modulo 256
            cur = np.cumsum(line.reshape(-1, bpp), axis=0, dtype=np.uint8).reshape(-1)
        elif ft in (3, 4):
            # Average and Paeth depend on the decoded byte to the left: a loop over plain ints (bytearrays, not numpy
            # scalars), bpp zero bytes in front standing for the pixels left of the row
            row = bytearray(bpp) + bytearray(line.tobytes())
            above = bytes(bpp) + up.tobytes()
            if ft == 3:
                for i in range(bpp, stride + bpp):
                    row[i] = (row[i] + ((row[i - bpp] + above[i]) >> 1)) & 255
            else:
                for i in range(bpp, stride + bpp):
                    a, b, c = row[i - bpp], above[i], above[i - bpp]
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - c - c)
                    row[i] = (row[i] + (a if (pa <= pb and pa <= pc) else (b if pb <= pc else c))) & 255
            cur = np.frombuffer(bytes(row[bpp:]), dtype=np.uint8)
        else:
            raise ValueError("read_png: filter type %d in row %d" % (ft, y))
        out[y] = cur
    return out


def _png_parse(path, who):
    """-> (the IHDR fields, the concatenated IDAT bytes) of a PNG file whose chunks all pass their checksum"""
    with open(path, "rb") as fp:
        data = fp.read()
    if data[:8] != _SIG:
        raise ValueError("%s: %s is not a PNG file" % (who, path))
    pos, ihdr, idat, ended = 8, None, [], False
    while pos + 8 <= len(data) and not ended:
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("%s: %s is truncated" % (who, path))
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError("%s: %s: bad checksum in chunk %r" % (who, path, tag))
        pos += 12 + n
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
    if ihdr is None or not idat or not ended:
        raise ValueError("%s: %s has no IHDR / IDAT / IEND" % (who, path))
    return ihdr, b"".join(idat)


def read_png(path):
    """-> uint8 numpy [H,W,C], C = 1 (grey), 2 (grey + alpha), 3 (RGB) or 4 (RGBA).  8-bit, non-interlaced files only:
    16-bit (or 1 / 2 / 4-bit), palette and interlaced files raise ValueError (read_png16 reads 16-bit files)."""
    ihdr, idat = _png_parse(path, "read_png")
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if ctype == 3:
        raise ValueError("read_png: %s is a palette image - not supported (8-bit grey, grey + alpha, RGB, RGBA only)" % path)
    if depth != 8:
        raise ValueError("read_png: %s has %d bits per sample - 8-bit files only" % (path, depth))
    if interlace != 0:
        raise ValueError("read_png: %s is interlaced (Adam7) - not supported" % path)
    if ctype not in _CHANNELS or comp != 0 or filt != 0 or W < 1 or H < 1:
        raise ValueError("read_png: %s: unsupported header %r" % (path, ihdr))
    Cn = _CHANNELS[ctype]
    raw = zlib.decompress(idat)
    if len(raw) != H * (1 + W * Cn):
        raise ValueError("read_png: %s: %d bytes of image data for %d x %d x %d" % (path, len(raw), H, W, Cn))
    return _unfilter(raw, H, W * Cn, Cn).reshape(H, W, Cn)


def read_png16(path):
    """-> uint16 numpy [H,W] (grey) or [H,W,C], C = 2 (grey + alpha), 3 (RGB) or 4 (RGBA): what cv2.imread(path, -1) hands
    the reference's depth readers for a grey file.  16-bit samples are big-endian in the file; the five row filters work on
    BYTES and take their "left" byte one whole pixel back, 2 C bytes at 16 bits.  An 8-bit file comes back as uint16 holding
    the bytes' values, unscaled (as cv2.imread(-1).astype(float32) keeps them).  Palette, interlaced and 1 / 2 / 4-bit files
    raise ValueError.  Channels stay in file order (R, G, B): cv2 would hand B, G, R."""
    ihdr, idat = _png_parse(path, "read_png16")
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if ctype == 3:
        raise ValueError("read_png16: %s is a palette image - not supported" % path)
    if depth not in (8, 16):
        raise ValueError("read_png16: %s has %d bits per sample - 16-bit (or 8-bit) files only" % (path, depth))
    if interlace != 0:
        raise ValueError("read_png16: %s is interlaced (Adam7) - not supported" % path)
    if ctype not in _CHANNELS or comp != 0 or filt != 0 or W < 1 or H < 1:
        raise ValueError("read_png16: %s: unsupported header %r" % (path, ihdr))
    Cn, nb = _CHANNELS[ctype], depth // 8
    raw = zlib.decompress(idat)
    if len(raw) != H * (1 + W * Cn * nb):
        raise ValueError("read_png16: %s: %d bytes of image data for %d x %d x %d x %d" % (path, len(raw), H, W, Cn, nb))
    rows = _unfilter(raw, H, W * Cn * nb, Cn * nb)
    out = rows.astype(np.uint16) if nb == 1 else np.ascontiguousarray(rows).view(">u2").astype(np.uint16)
    return out.reshape(H, W) if Cn == 1 else out.reshape(H, W, Cn)


def png16_bytes(u16, level=6):
    """uint16 [H,W], [H,W,1], [H,W,2], [H,W,3] or [H,W,4] -> the bytes of a 16-bit, non-interlaced PNG (filter type 0)"""
    if torch.is_tensor(u16):
        u16 = u16.detach().cpu().numpy()
    u16 = np.asarray(u16)
    if u16.dtype != np.uint16:
        raise ValueError("png16_bytes: uint16 only (got %s)" % u16.dtype)
    if u16.ndim == 2:
        u16 = u16[:, :, None]
    if u16.ndim != 3 or u16.shape[2] not in _COLOUR_TYPE or u16.shape[0] < 1 or u16.shape[1] < 1:
        raise ValueError("png16_bytes: [H,W] or [H,W,1..4] of at least one pixel (got %s)" % (u16.shape,))
    H, W, Cn = u16.shape
    rows = np.zeros((H, 1 + 2 * W * Cn), dtype=np.uint8)
    rows[:, 1:] = np.ascontiguousarray(u16.astype(">u2")).view(np.uint8).reshape(H, 2 * W * Cn)
    ihdr = struct.pack(">IIBBBBB", W, H, 16, _COLOUR_TYPE[Cn], 0, 0, 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png16(path, u16):
    """Write uint16 [H,W] or [H,W,1..4] (tensor or array) as a 16-bit, non-interlaced PNG: the form of the depth files."""
    data = png16_bytes(u16)
    with open(path, "wb") as fp:
        fp.write(data)


# ------------------------------------------------------------------------------------------------ save_image's bytes
def save_image_bytes(tensor):
    """[C,H,W] (or [H,W], or [1,C,H,W]) float tensor -> uint8 [H,W,C] on the tensor's device: the bytes
    torchvision.utils.save_image writes.  A 1-channel image becomes three equal channels (make_grid).  Device tensors of up to
    4 channels get their bytes from gs_eval_metrics's quantised_out - a caller that scores the render anyway takes them from
    image_metrics(..., return_bytes=True) instead - and CPU tensors from torch's own float32 operations: the same bytes."""
    if not torch.is_tensor(tensor):
        raise ValueError("save_image_bytes: expected a tensor, got %s" % type(tensor).__name__)
    t = tensor.detach()
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError("save_image_bytes: one [C,H,W] image (got shape %s)" % (tuple(tensor.shape),))
    if t.shape[0] == 1:
        t = t.expand(3, -1, -1)
    t = t.to(torch.float32).contiguous()
    if t.is_cuda and t.shape[0] <= 4:
        from .evaluate import image_metrics
        return image_metrics(t, t, return_bytes=True)["bytes"]
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------------------------ resize
def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_tables = {}
_device_tables = {}
CACHE_PAIRS = 64   # (in, out) pairs either cache holds; an evaluation uses two or four, so a full cache is simply emptied


def resize_tables(n_in, n_out):
    """-> (bounds int32 [n_out,2] = (xmin, n), coef int32 [n_out,ksize]) of one axis, cached per (n_in, n_out)"""
    key = (int(n_in), int(n_out))
    if key in _tables:
        return _tables[key]
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError("resize_tables: sizes >= 1 (got %d -> %d)" % key)
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = [_bicubic((x + xmin - center + 0.5) / filterscale) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(k * (1 << PRECISION_BITS) + 0.5) if k >= 0 else int(k * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, n)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    if len(_tables) >= CACHE_PAIRS:
        _tables.clear()
    _tables[key] = (bounds, coef)
    return _tables[key]


def _pass_numpy(src, bounds, coef):
    """One pass along axis 0 of src uint8 [n_in, ...] -> uint8 [n_out, ...]"""
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    s = src.astype(np.int64)
    for o in range(bounds.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        k = coef[o, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (k * s[lo:lo + n]).sum(axis=0)
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)   # (>> on a signed integer is arithmetic, as in C)
    return out


def resize_u8_numpy(img, size):
    """uint8 numpy [H,W] or [H,W,C] -> Image.resize(size = (W2, H2))'s bytes, in numpy"""
    W2, H2 = int(size[0]), int(size[1])
    H, W = img.shape[:2]
    if W2 != W:
        img = np.swapaxes(_pass_numpy(np.swapaxes(img, 0, 1), *resize_tables(W, W2)), 0, 1)
    if H2 != H:
        img = _pass_numpy(img, *resize_tables(H, H2))
    return np.ascontiguousarray(img).copy() if (W2 == W and H2 == H) else np.ascontiguousarray(img)


def _tables_on(device, n_in, n_out):
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()   # "cuda" and "cuda:0": one entry
    key = (device.type, index, int(n_in), int(n_out))
    if key not in _device_tables:
        b, c = resize_tables(n_in, n_out)
        if len(_device_tables) >= CACHE_PAIRS:
            _device_tables.clear()   # (a launch that still reads a dropped table holds it: the allocator frees in stream order)
        _device_tables[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(c.copy()).to(device))
    return _device_tables[key]


def resize_u8(img, size, return_planar=False):
    """PIL-named: img.resize(size) with size = (W2, H2) and Pillow's default filter, for a uint8 [H,W], [H,W,1] or [H,W,3]
    image.  A CUDA(HIP) tensor goes through the kernel and stays on the device; a CPU tensor or a numpy array takes the
    numpy path and comes back as what it was.  return_planar: also the fp32 [C,H2,W2] image = bytes / 255 (to_tensor)."""
    W2, H2 = int(size[0]), int(size[1])
    if W2 < 1 or H2 < 1:
        raise ValueError("resize_u8: size = (W2, H2) with both >= 1 (got %r)" % (size,))
    is_tensor = torch.is_tensor(img)
    if (img.dtype != torch.uint8) if is_tensor else (np.asarray(img).dtype != np.uint8):
        raise ValueError("resize_u8: uint8 only (got %s)" % (img.dtype,))
    flat = img.dim() == 2 if is_tensor else np.asarray(img).ndim == 2
    shape = tuple(img.shape) + ((1,) if flat else ())
    if len(shape) != 3 or shape[2] not in (1, 3) or shape[0] < 1 or shape[1] < 1:
        raise ValueError("resize_u8: [H,W], [H,W,1] or [H,W,3] (got %s) - Pillow premultiplies alpha for LA / RGBA, which is "
                         "not restated here" % (tuple(img.shape),))
    H, W, Cn = shape
    if is_tensor and img.is_cuda:
        from ._lib import hip_api
        from ._lib import stream_of
        api = hip_api()
        src = img.contiguous()
        out = torch.empty((H2, W2, Cn), dtype=torch.uint8, device=img.device)
        planar = torch.empty((Cn, H2, W2), dtype=torch.float32, device=img.device) if return_planar else None
        xb, xc = _tables_on(img.device, W, W2) if W2 != W else (None, None)
        yb, yc = _tables_on(img.device, H, H2) if H2 != H else (None, None)
        nb = int(api.raw("resize_tmp_bytes")(H, W, Cn, H2, W2))
        tmp = torch.empty((nb,), dtype=torch.uint8, device=img.device) if nb else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        api.call("resize_bicubic_u8", src.data_ptr(), H, W, Cn, H2, W2, ptr(xb), ptr(xc), 0 if xc is None else xc.shape[1],
                 ptr(yb), ptr(yc), 0 if yc is None else yc.shape[1], ptr(tmp), nb, out.data_ptr(), ptr(planar), stream_of(img))
    else:
        arr = (img.numpy() if is_tensor else np.asarray(img)).reshape(H, W, Cn)
        res = resize_u8_numpy(arr, (W2, H2))
        pl = np.ascontiguousarray(res.transpose(2, 0, 1)).astype(np.float32) / np.float32(255) if return_planar else None
        out = torch.from_numpy(res) if is_tensor else res
        planar = None if pl is None else (torch.from_numpy(pl) if is_tensor else pl)
    if flat:
        out = out[:, :, 0]
    return (out, planar) if return_planar else out


def to_planar(u8):
    """torchvision's to_tensor of a decoded 8-bit image: uint8 [H,W], [H,W,1] or [H,W,3] -> fp32 [C,H,W] = byte / 255, where the
    input lives.  On the device this is the resize kernel's same-size path, whose division is one correctly rounded fp32
    operation (a device-side div by a scalar may multiply by the reciprocal instead)."""
    H, W = int(u8.shape[0]), int(u8.shape[1])
    return resize_u8(u8, (W, H), return_planar=True)[1]


# ------------------------------------------------------------------------------------------------------------ ingest
# What lies between a decoded image file and the tensors a Camera keeps (LGDWT-GS/utils/camera_utils.py:loadCam,
# scene/cameras.py:42-56): NeRF-synthetic's composite, Image.resize with Pillow's rule for images WITH alpha, byte / 255 and the
# alpha mask.  Device tensors go through gs_image_ingest (csrc/gs_image_ingest.hip), arrays and CPU tensors through numpy: the
# numpy path is the arbiter, tests/golden/pil_resize_alpha.npz pins it to Pillow's bytes.  (resize_u8 keeps refusing alpha.)
# Pillow's rule for LA / RGBA (Image.resize converts to La / RGBa and back):
#   premultiply      t = c a + 128, c' = ((t >> 8) + t) >> 8, alpha unchanged          (Convert.c: MULDIV255)
#   both passes of the integer bicubic on the premultiplied bytes, alpha included
#   un-premultiply   a == 0 or a == 255 -> c', else min(255, (255 c') // a)               (Convert.c: rgba2rgbA... la2lA)
#   same size        the bytes are copied: Pillow returns self.copy() before it converts
INGEST_COMPOSITE, INGEST_WHITE, INGEST_ZERO_LEFT, INGEST_ZERO_RIGHT = 1, 2, 4, 8   # GS_INGEST_*


def premultiply_u8(img):
    """uint8 numpy [H,W,2] / [H,W,4] -> the colour channels times alpha by Pillow's MULDIV255, alpha unchanged"""
    a = img[:, :, -1:].astype(np.int64)
    t = img[:, :, :-1].astype(np.int64) * a + 128
    out = img.copy()
    out[:, :, :-1] = ((t >> 8) + t) >> 8
    return out


def unpremultiply_u8(img):
    """uint8 numpy [H,W,2] / [H,W,4] premultiplied -> straight alpha: a in (0, 255) divides, in integers, clipped at 255"""
    a = img[:, :, -1:].astype(np.int64)
    c = img[:, :, :-1].astype(np.int64)
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out = img.copy()
    out[:, :, :-1] = np.where((a == 0) | (a == 255), c, q)
    return out


def resize_alpha_u8_numpy(img, size):
    """uint8 numpy [H,W,2] (LA) or [H,W,4] (RGBA) -> Image.resize(size = (W2, H2))'s bytes, in numpy"""
    W2, H2 = int(size[0]), int(size[1])
    if (W2, H2) == (img.shape[1], img.shape[0]):
        return np.ascontiguousarray(img).copy()
    return unpremultiply_u8(resize_u8_numpy(premultiply_u8(img), (W2, H2)))


def composite_u8_numpy(rgba, white_background):
    """uint8 numpy [H,W,4] -> uint8 [H,W,3]: the bytes of dataset_readers.py:353-359 (io.composite_rgba times 255), in float64"""
    norm = rgba.astype(np.float64) / 255.0
    bg = 1.0 if white_background else 0.0
    arr = norm[:, :, :3] * norm[:, :, 3:4] + bg * (1 - norm[:, :, 3:4])
    return (arr * 255.0).astype(np.int64).astype(np.uint8)


def _u8_image(img, who, channels):
    is_tensor = torch.is_tensor(img)
    if (img.dtype != torch.uint8) if is_tensor else (np.asarray(img).dtype != np.uint8):
        raise ValueError("%s: uint8 only (got %s)" % (who, img.dtype))
    shape = tuple(img.shape)
    if len(shape) != 3 or shape[2] not in channels or shape[0] < 1 or shape[1] < 1:
        raise ValueError("%s: [H,W,C] with C in %s (got %s)" % (who, "/".join(str(c) for c in channels), shape))
    return is_tensor, shape


def _ingest_call(src, size, flags, want_u8, want_planes):
    """gs_image_ingest on a device tensor uint8 [H,W,C] -> (bytes or None, original_image or None, alpha_mask or None)"""
    from ._lib import hip_api
    from ._lib import stream_of
    api = hip_api()
    src = src.contiguous()
    H, W, Cn = (int(v) for v in src.shape)
    W2, H2 = size
    Ce = 3 if flags & INGEST_COMPOSITE else Cn
    dev = src.device
    out = torch.empty((H2, W2, Ce), dtype=torch.uint8, device=dev) if want_u8 else None
    image = torch.empty((3, H2, W2), dtype=torch.float32, device=dev) if want_planes else None
    alpha = torch.empty((1, H2, W2), dtype=torch.float32, device=dev) if want_planes else None
    xb, xc = _tables_on(dev, W, W2) if W2 != W else (None, None)
    yb, yc = _tables_on(dev, H, H2) if H2 != H else (None, None)
    nb = int(api.raw("image_ingest_tmp_bytes")(H, W, Cn, H2, W2, flags))
    tmp = torch.empty((nb,), dtype=torch.uint8, device=dev) if nb else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    api.call("image_ingest", src.data_ptr(), H, W, Cn, H2, W2, ptr(xb), ptr(xc), 0 if xc is None else xc.shape[1], ptr(yb), ptr(yc),
             0 if yc is None else yc.shape[1], flags, ptr(tmp), nb, ptr(out), ptr(image), ptr(alpha), stream_of(src))
    return out, image, alpha


def resize_alpha_u8(img, size):
    """PIL-named: img.resize(size) with size = (W2, H2) and Pillow's default filter for a uint8 [H,W,2] (LA) or [H,W,4] (RGBA)
    image.  A CUDA(HIP) tensor goes through gs_image_ingest and stays on the device; a CPU tensor or a numpy array takes the
    numpy path and comes back as what it was.  The same bits either way."""
    W2, H2 = int(size[0]), int(size[1])
    if W2 < 1 or H2 < 1:
        raise ValueError("resize_alpha_u8: size = (W2, H2) with both >= 1 (got %r)" % (size,))
    is_tensor, _ = _u8_image(img, "resize_alpha_u8", (2, 4))
    if is_tensor and img.is_cuda:
        return _ingest_call(img, (W2, H2), 0, True, False)[0]
    res = resize_alpha_u8_numpy(img.numpy() if is_tensor else np.asarray(img), (W2, H2))
    return torch.from_numpy(res) if is_tensor else res


def ingest_image(u8, size, white_background=None, train_test_exp=False, is_test_view=False, is_test_dataset=False):
    """One decoded image, uint8 [H,W,3] or [H,W,4], -> (original_image fp32 [3,H2,W2], alpha_mask fp32 [1,H2,W2]) at
    size = (W2, H2): what the reference's Camera keeps of it.
      white_background  None: a COLMAP scene's image, resized as it is (an RGBA file's alpha becomes the mask, cameras.py:45-46).
                        True / False: NeRF-synthetic - composite onto white / black first, at the source size, with the byte
                        rule of dataset_readers.py:353-359 (an RGB file is given alpha 255, as its convert("RGBA") does); the
                        image is RGB from there and the mask ones
      train_test_exp, is_test_view, is_test_dataset   cameras.py:50-54: a test view keeps the half of its mask that its set scores
    A CUDA(HIP) tensor goes through gs_image_ingest (at most two launches, no synchronisation) and the results stay on its
    device; a CPU tensor gives CPU tensors and an array gives arrays through numpy - the same bits either way."""
    W2, H2 = int(size[0]), int(size[1])
    if W2 < 1 or H2 < 1:
        raise ValueError("ingest_image: size = (W2, H2) with both >= 1 (got %r)" % (size,))
    is_tensor, shape = _u8_image(u8, "ingest_image", (3, 4))
    half = train_test_exp and is_test_view
    if is_tensor and u8.is_cuda:
        flags = 0
        if white_background is not None:
            if shape[2] == 3:
                u8 = torch.cat((u8, torch.full(shape[:2] + (1,), 255, dtype=torch.uint8, device=u8.device)), dim=2)
            flags = INGEST_COMPOSITE | (INGEST_WHITE if white_background else 0)
        if half:
            flags |= INGEST_ZERO_LEFT if is_test_dataset else INGEST_ZERO_RIGHT
        _, image, alpha = _ingest_call(u8, (W2, H2), flags, False, True)
        return image, alpha
    arr = u8.numpy() if is_tensor else np.asarray(u8)
    if white_background is not None:
        if shape[2] == 3:
            arr = np.concatenate((arr, np.full(shape[:2] + (1,), 255, dtype=np.uint8)), axis=2)
        arr = composite_u8_numpy(arr, bool(white_background))
    res = resize_u8_numpy(arr, (W2, H2)) if arr.shape[2] == 3 else resize_alpha_u8_numpy(arr, (W2, H2))
    planes = np.ascontiguousarray(res.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    image = np.ascontiguousarray(planes[:3])
    alpha = planes[3:4].copy() if planes.shape[0] == 4 else np.ones((1, H2, W2), dtype=np.float32)
    if half:
        if is_test_dataset:
            alpha[..., :W2 // 2] = 0
        else:
            alpha[..., W2 // 2:] = 0
    return (torch.from_numpy(image), torch.from_numpy(alpha)) if is_tensor else (image, alpha)

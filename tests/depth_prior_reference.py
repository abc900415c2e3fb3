"""Twins of gsplat_amd/depth_priors.py for the tests: make_depth_scale.py's get_scales and cameras.py's map preparation written
a second time, with the two cv2 calls replaced by the rules DESIGN.md 4.8.4 states, plus a float64 form of each.

  scales_twin(..., wide=False)   the fit in the script's dtypes.  The medians come from a SORT (middle element, or the two
                                 middle ones added and halved in the sequence's own dtype) where the module calls np.median;
                                 the sample splits rint(32 x) by floor division and remainder where the module shifts and masks
  scales_twin(..., wide=True)    the same terms |inv - t_colmap| (float64) and |mono - t_mono| (float32 differences), summed
                                 EXACTLY (math.fsum) and divided in float64: the form the device's fixed-order float64 sums are
                                 held to
  prepare_twin                   the camera's map in float32, coordinate by coordinate
  prepare_twin64                 the same rule with every product and sum in float64 (the float32 quantities the rule itself
                                 names - the fraction fx, float32(scale), float32(offset) - keep their float32 values)
"""
import math

import numpy as np

from gsplat_amd import io as gio

F32 = np.float32


def sample_twin(mono_map, x, y, coord_bits=5):
    h, w = mono_map.shape
    out = np.empty(x.shape, dtype=np.float32)
    for k in range(x.shape[0]):
        cell, frac = [], []
        for v in (x[k], y[k]):
            v = F32(v)
            if coord_bits is None:
                c = math.floor(float(v))
                f = v - F32(c)
            else:
                q = 1 << coord_bits
                i = int(np.rint(v * F32(q)))          # half-to-even
                c, f = i // q, F32(i % q) / F32(q)
            cell.append(c)
            frac.append(F32(f))
        (cx, cy), (fx, fy) = cell, frac
        x0, x1 = min(max(cx, 0), w - 1), min(max(cx + 1, 0), w - 1)
        y0, y1 = min(max(cy, 0), h - 1), min(max(cy + 1, 0), h - 1)
        gx, gy = F32(1) - fx, F32(1) - fy
        acc = F32(gy * gx) * mono_map[y0, x0]
        acc = F32(acc + F32(gy * fx) * mono_map[y0, x1])
        acc = F32(acc + F32(fy * gx) * mono_map[y1, x0])
        acc = F32(acc + F32(fy * fx) * mono_map[y1, x1])
        out[k] = acc
    return out


def _middle(sorted_values):
    n = sorted_values.shape[0]
    if n % 2:
        return sorted_values[n // 2]
    a, b = sorted_values[n // 2 - 1], sorted_values[n // 2]
    return (a + b) / sorted_values.dtype.type(2)


def scales_twin(image, cam, table, mono, coord_bits=5, wide=False):
    """-> dict(scale, offset, n_valid, t_colmap, s_colmap, t_mono, s_mono, range, abs_c, abs_m); abs_* = the sums of the
    deviations' terms (what the summation bound scales with).  Where the gate fails the four statistics are 0."""
    ids = np.asarray(image.point3D_ids, dtype=np.int64)
    keep = (ids >= 0) & (ids < table.shape[0])
    zero = dict(scale=0, offset=0, n_valid=0, t_colmap=0.0, s_colmap=0.0, t_mono=0.0, s_mono=0.0, range=0.0, abs_c=0.0, abs_m=0.0)
    if not keep.any():
        return zero
    R = gio.qvec2rotmat(image.qvec)
    P = table[ids[keep]]
    xy = np.asarray(image.xys, dtype=np.float64)[keep]
    field = np.asarray(mono).astype(np.float32) / F32(65536)
    with np.errstate(all="ignore"):
        z = P[:, 0] * R[2, 0]
        z = z + P[:, 1] * R[2, 1]
        z = z + P[:, 2] * R[2, 2]
        z = z + float(image.tvec[2])
        inv = 1.0 / z
        s = field.shape[0] / int(cam.height)
        m = (xy * s).astype(np.float32)
        wlim, hlim = F32(int(cam.width) * s), F32(int(cam.height) * s)     # the Python float meets a float32 array: float32
        ok = (m[:, 0] >= 0) & (m[:, 1] >= 0) & (m[:, 0] < wlim) & (m[:, 1] < hlim) & (inv > 0)
        spread = inv.max() - inv.min()
    n = int(ok.sum())
    zero.update(n_valid=n, range=float(spread))
    if not (n > 10 and spread > 1e-3):
        return zero
    inv, m = inv[ok], m[ok]
    sampled = sample_twin(field, m[:, 0], m[:, 1], coord_bits)
    with np.errstate(all="ignore"):
        t_c = _middle(np.sort(inv))
        t_m = _middle(np.sort(sampled))
        dev_c, dev_m = np.abs(inv - t_c), np.abs(sampled - t_m)
        if wide:
            finite = np.isfinite(dev_c).all()
            s_c = np.float64(math.fsum(dev_c.tolist()) if finite else dev_c.sum()) / np.float64(n)
            s_m = np.float64(math.fsum(dev_m.astype(np.float64).tolist())) / np.float64(n)
        else:
            s_c, s_m = np.mean(dev_c), np.mean(dev_m)
        scale = s_c / s_m
        offset = t_c - t_m * scale
    return dict(scale=float(scale), offset=float(offset), n_valid=n, t_colmap=float(t_c), s_colmap=float(s_c), t_mono=float(t_m),
                s_mono=float(s_m), range=float(spread), abs_c=float(dev_c.sum()), abs_m=float(dev_m.astype(np.float64).sum()))


# ------------------------------------------------------------------------------------------------ the camera's map
def _coord(d, n_in, n_out):
    f = F32((d + 0.5) * (n_in / n_out) - 0.5)
    s = math.floor(float(f))
    f = F32(f - F32(s))
    if s < 0:
        s, f = 0, F32(0)
    if s >= n_in - 1:
        s, f = n_in - 1, F32(0)
    return s, min(s + 1, n_in - 1), f


def _prepare(src, size, entry, divisor, dt):
    src = np.asarray(src)
    H, W = src.shape
    W2, H2 = size
    S = (src.astype(np.float32) / F32(divisor)).astype(dt)     # (exact for 65536 and 512)
    if (H2, W2) == (H, W):
        out = S.copy()
    else:
        xs = [_coord(d, W, W2) for d in range(W2)]
        ys = [_coord(d, H, H2) for d in range(H2)]
        rows = np.empty((H, W2), dtype=dt)
        for d, (x0, x1, f) in enumerate(xs):
            a1 = dt(f)
            a0 = dt(F32(1) - f) if dt is F32 else dt(1) - a1
            rows[:, d] = a0 * S[:, x0] + a1 * S[:, x1]
        out = np.empty((H2, W2), dtype=dt)
        for d, (y0, y1, f) in enumerate(ys):
            b1 = dt(f)
            b0 = dt(F32(1) - f) if dt is F32 else dt(1) - b1
            out[d] = b0 * rows[y0] + b1 * rows[y1]
    out[out < 0] = 0
    reliable = True
    if entry is not None:
        if entry["scale"] < 0.2 * entry["med_scale"] or entry["scale"] > 5 * entry["med_scale"]:
            reliable = False
        if entry["scale"] > 0:
            out = out * dt(F32(entry["scale"])) + dt(F32(entry["offset"]))
    mask = np.full((1, H2, W2), 1.0 if reliable else 0.0, dtype=np.float32)
    return out[None].astype(dt), mask, reliable


def prepare_twin(src, size, entry=None, divisor=65536.0):
    return _prepare(src, size, entry, divisor, F32)


def prepare_twin64(src, size, entry=None, divisor=65536.0):
    return _prepare(src, size, entry, divisor, np.float64)

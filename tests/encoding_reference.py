"""Torch restatement of DNGaussian's grid and SH encoders (gridencoder/src/gridencoder.cu, shencoder/src/shencoder.cu),
independent of the HIP code: the arbiter of tests/test_encoding_cpu.py and tests/test_gpu_encoding.py.

Grid: the level geometry, corner selection and hash use fp32 arithmetic exactly as the reference states them (scale =
exp2(l * S) * H - 1 from the fp32 product l * S, pos = x * scale + 0.5 / 0, its floor and fraction in fp32, uint32
hashing); interpolation and every sum run in float64 with torch autograd, which also gives the embedding and input
gradients.  The input gradient flows through the fraction with d(frac)/dx = scale (smoothstep: its derivative too):
frac = fp32 fraction + (x - fp32(x)) * scale, which is the fp32 fraction itself for fp32 inputs.
The left corner's factor under smoothstep is s(1 - p), which is 1 - s(p) exactly (s(p) = p^2 (3 - 2 p)) and keeps its
relative accuracy next to a cell face, where 1 - s(p) cancels: float64's 1 - s(p) is itself 1e-5 off such a factor.

SH: the general Cartesian real-SH formula with the r^2 -> 1 substitution and the reference's sign (band 1 is
(-C1 y, C1 z, -C1 x), the Condon-Shortley phase (-1)^m), evaluated as written for non-unit inputs too:
    Y_l^0  = K_l^0 Pi_l^0(z)
    Y_l^m  = (-1)^m sqrt(2) K_l^m Pi_l^m(z) A_m(x, y),   Y_l^-m = (-1)^m sqrt(2) K_l^m Pi_l^m(z) B_m(x, y)   (m > 0)
    Pi_l^m(z) = sum_k (-1)^k 2^-l C(l,k) C(2l-2k,l) (l-2k)!/(l-2k-m)! z^(l-2k-m)
    A_m = sum_p C(m,p) x^p y^(m-p) cos((m-p) pi/2),   B_m = sum_p C(m,p) x^p y^(m-p) sin((m-p) pi/2)
output index l^2 + l + m.  This gives shencoder.cu's polynomials for degrees 1..8 term for term."""
import math

import numpy as np
import torch

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037)
U32 = 0xFFFFFFFF


def grid_offsets(D, L, per_level_scale, H, log2_hashmap_size, align_corners):
    """gridencoder/grid.py: min(2^log2_hashmap_size, (res or res+1)^D) per level, up to a multiple of 8, float64."""
    offsets, offset = [], 0
    for i in range(L):
        res = int(np.ceil(H * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (res if align_corners else res + 1) ** D)
        offsets.append(offset)
        offset += int(np.ceil(n / 8) * 8)
    offsets.append(offset)
    return offsets


def per_level_scale_of(L, H, per_level_scale=2.0, desired_resolution=None):
    if desired_resolution is not None:
        return float(np.exp2(np.log2(desired_resolution / H) / (L - 1)))
    return per_level_scale


def level_geometry(L, per_level_scale, H):
    """[(scale, resolution)] per level: S = log2(per_level_scale) as fp32, the fp32 product l * S, exp2 rounded once to
    fp32, * H - 1 in fp32; resolution = ceil(scale) + 1."""
    S = np.float32(np.log2(per_level_scale))
    out = []
    for l in range(L):
        ls = np.float32(np.float32(l) * S)
        e = np.float32(np.exp2(np.float64(ls)))
        sc = np.float32(np.float32(e * np.float32(H)) - np.float32(1.0))
        out.append((sc, int(np.ceil(sc)) + 1))
    return out


def _slot(cell, D, gridtype, align_corners, hsize, res):
    """cell: int64 [B, D] -> slot in [0, hsize) (uint32 arithmetic, as the reference's get_grid_index)."""
    stride, index = 1, torch.zeros_like(cell[:, 0])
    d = 0
    while d < D and stride <= hsize:
        index = (index + cell[:, d] * stride) & U32
        stride = (stride * (res if align_corners else res + 1)) & U32
        d += 1
    if gridtype == 0 and stride > hsize:
        index = torch.zeros_like(cell[:, 0])
        for d in range(D):
            index = index ^ ((cell[:, d] * PRIMES[d]) & U32)
    return index % hsize


def grid_encode_ref(inputs, embeddings, offsets, per_level_scale, H, gridtype=0, align_corners=False, interpolation=0,
                    fp32_cells=True, dtype=torch.float64):
    """inputs [B,D] in [0,1] (fp32 or fp64, may require grad), embeddings [n_slots,C] (any float, may require grad)
    -> float64 [B, L*C].  fp32_cells=False places the points in float64 throughout (for gradcheck, whose float64
    perturbations are below the fp32 rounding of the position).  dtype=torch.float32 forms every product and sum
    (smoothstep, corner weights, the interpolation and, through autograd, both gradients) in fp32 instead: one fp32
    order among many, the yardstick of tests/encoding_cases.py's measured bars; the result is then fp32."""
    x32 = inputs.detach().float()
    xg = inputs.to(dtype)
    emb = embeddings.to(dtype)
    B, D = x32.shape
    L = len(offsets) - 1
    oob = ((x32 < 0) | (x32 > 1)).any(dim=1)
    xs = torch.where(oob[:, None], torch.zeros_like(x32), x32)
    outs = []
    for l, (sc, res) in enumerate(level_geometry(L, per_level_scale, H)):
        pos = xs * torch.tensor(sc, dtype=torch.float32) + torch.tensor(0.0 if align_corners else 0.5, dtype=torch.float32)
        if not fp32_cells:
            pos = torch.where(oob[:, None], torch.zeros_like(xg), xg) * float(sc) + (0.0 if align_corners else 0.5)
        fl = torch.floor(pos.detach())
        cell = fl.long()
        if fp32_cells:
            frac = (pos - fl).to(dtype) + (xg - xs.to(dtype)) * float(sc)  # (zero for fp32 inputs; carries d/dx = scale)
        else:
            frac = pos - fl
        cfrac = 1.0 - frac
        if interpolation == 1:
            frac, cfrac = frac * frac * (3.0 - 2.0 * frac), cfrac * cfrac * (3.0 - 2.0 * cfrac)
        base, hsize = offsets[l], offsets[l + 1] - offsets[l]
        acc = 0.0
        for k in range(1 << D):
            bits = torch.tensor([(k >> d) & 1 for d in range(D)], dtype=torch.int64, device=cell.device)
            w = torch.ones((B,), dtype=dtype, device=cell.device)
            for d in range(D):
                w = w * (frac[:, d] if (k >> d) & 1 else cfrac[:, d])
            rows = base + _slot(cell + bits, D, gridtype, align_corners, hsize, res)
            acc = acc + w[:, None] * emb[rows]
        outs.append(torch.where(oob[:, None], torch.zeros_like(acc), acc))
    return torch.cat(outs, dim=1)


# ---- spherical harmonics ----
def _pi_coeffs(l, m):
    """[(coefficient, power of z)] of Pi_l^m with r^2 -> 1."""
    out = []
    for k in range((l - m) // 2 + 1):
        c = (-1) ** k * 2.0 ** -l * math.comb(l, k) * math.comb(2 * l - 2 * k, l) \
            * math.factorial(l - 2 * k) / math.factorial(l - 2 * k - m)
        out.append((c, l - 2 * k - m))
    return out


def sh_encode_ref(inputs, degree, dtype=torch.float64):
    """inputs [B,3] (any float, may require grad) -> float64 [B, degree^2]; dtype=torch.float32: the same statements with
    every product and sum in fp32 (the yardstick of the per-column bars of tests/encoding_cases.py)."""
    v = inputs.to(dtype)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = [None] * (degree * degree)
    for l in range(degree):
        for m in range(l + 1):
            K = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            pi = sum(c * z ** p for c, p in _pi_coeffs(l, m))
            if m == 0:
                out[l * l + l] = K * pi * torch.ones_like(x)
                continue
            A = sum(math.comb(m, p) * x ** p * y ** (m - p) * round(math.cos((m - p) * math.pi / 2)) for p in range(m + 1))
            Bm = sum(math.comb(m, p) * x ** p * y ** (m - p) * round(math.sin((m - p) * math.pi / 2)) for p in range(m + 1))
            s = (-1) ** m * math.sqrt(2.0) * K
            out[l * l + l + m] = s * pi * A
            out[l * l + l - m] = s * pi * Bm
    return torch.stack(out, dim=1)

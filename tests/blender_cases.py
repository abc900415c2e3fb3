"""Constructed inputs for the Blender kernels (csrc/gs_dng_blender.hip), shared by tests/test_blender_cpu.py (which proves the
table) and tests/test_gpu_blender_kernels.py (which holds the kernels to it).  Everything is float32 on the CPU, built from
fixed seeds."""
import torch

import blender_reference as br

IMAGE_SIZES = ((1, 1), (3, 5), (17, 64), (65, 257))
IMAGE_KINDS = ("mixed", "white", "none")
RULE_P = (1, 63, 64, 65, 255, 256, 257, 1023)
BG_THR = 254 / 255
WHITE_THR = 253 / 255
SH_FORMS = tuple((M, d) for M, top in ((1, 0), (4, 1), (9, 2), (16, 3)) for d in range(top + 1))   # (M, active degree)
SH_MARGIN = 1e-4      # every SH row's float64 minimum colour is farther than this from WHITE_THR: a condition on the INPUTS
INF = torch.tensor(float("inf"))
DENORMAL = 2.0 ** -140   # an fp32 denormal, exactly
SPECIAL_OPACITIES = (-30.0, -0.0, 0.0, 20.0, DENORMAL, float("-inf"), float("nan"))


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def around(thr):
    """float32(thr) and its two neighbours -> (below, at, above) as Python floats"""
    t = f32(thr)
    return float(torch.nextafter(t, -INF)), float(t), float(torch.nextafter(t, INF))


def edge_pixels(H, W):
    """where "mixed" images carry their constructed pixels: name -> flat pixel index (those that fit H W pixels)"""
    n = H * W
    spots = {"at": 0, "above": n // 3 + 1, "below": n // 2 + 1, "nan": (2 * n) // 3 + 1, "nan_white": n - 1}
    out, used = {}, set()
    for name, i in spots.items():
        if i < n and i not in used:
            out[name] = i
            used.add(i)
    return out


def image(H, W, kind="mixed", thr=BG_THR, seed=0):
    """gt [3,H,W].  "mixed": about a third of the pixels white (every channel above the threshold), the others with at least one
    channel below it, and the pixels of edge_pixels: channel minimum at float32(thr) (unmasked), at its upper neighbour
    (masked), at its lower one (unmasked), a NaN channel beside two white ones (unmasked), and all three NaN (unmasked).
    "white": every pixel above the threshold; "none": no pixel."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    below, at, above = around(thr)
    white = above + (1.0 - above) * torch.rand((3, H, W), generator=g)
    white = torch.maximum(white, f32(above))
    if kind == "white":
        return white.contiguous()
    other = white.clone()
    ch = torch.randint(0, 3, (H, W), generator=g)
    low = 0.99 * thr * torch.rand((H, W), generator=g)
    for c in range(3):
        other[c] = torch.where(ch == c, low, other[c])
    if kind == "none":
        return other.contiguous()
    is_white = torch.rand((H, W), generator=g) < 1 / 3
    gt = torch.where(is_white[None], white, other).contiguous()
    flat = gt.view(3, -1)
    for k, (name, i) in enumerate(edge_pixels(H, W).items()):
        flat[:, i] = 1.0
        c = k % 3
        if name == "nan":
            flat[c, i] = float("nan")
        elif name == "nan_white":
            flat[:, i] = float("nan")
        else:
            flat[c, i] = dict(at=at, above=above, below=below)[name]
    return gt


def mono_image(H, W, seed=0):
    """a mono depth map as stored: [H,W] in [0, 255]"""
    g = torch.Generator().manual_seed(31 * H + W + seed)
    return (torch.rand((H, W), generator=g) * 255.0).contiguous()


def rule_rows(P, thr=WHITE_THR, seed=0):
    """colour [P,3], stat [P,1] (all non-zero), opacity_raw [P,1]: half of the rows white; rows 0, 7, 14 (those below P) have
    their channel minimum at the lower neighbour of float32(thr), at float32(thr) and at its upper neighbour; rows 3, 8, 13, ...
    (those below P) are white and carry SPECIAL_OPACITIES; one row has a NaN channel beside two white ones."""
    g = torch.Generator().manual_seed(500 + P + seed)
    below, at, above = around(thr)
    u = torch.rand((P, 3), generator=g)
    white = torch.maximum(above + (1.0 - above) * u, f32(above))
    other = white.clone()
    other[torch.arange(P), torch.randint(0, 3, (P,), generator=g)] = 0.99 * thr * torch.rand((P,), generator=g)
    colour = torch.where((torch.arange(P) % 2 == 1)[:, None], white, other)
    stat = 1e-4 + torch.rand((P, 1), generator=g) * 1e-3
    opacity = torch.randn((P, 1), generator=g) * 3.0
    for i, v in enumerate((below, at, above)):
        if 7 * i < P:
            colour[7 * i] = 1.0
            colour[7 * i, i % 3] = v
    for k, v in enumerate(SPECIAL_OPACITIES):
        if 3 + 5 * k < P:
            colour[3 + 5 * k] = white[3 + 5 * k]
            opacity[3 + 5 * k, 0] = v
    if P > 40:
        colour[40] = 1.0
        colour[40, 1] = float("nan")
    return colour.contiguous(), stat.contiguous(), opacity.contiguous()


def sh_rows(P, M, thr=WHITE_THR, seed=0):
    """xyz [P,3], features [P,M,3] (every coefficient non-zero, the inactive ones included), campos [3], stat [P,1],
    opacity_raw [P,1], centre (the row that sits on the camera centre, or None when P == 1): about half of the rows white at
    degree 0.  The dc coefficients are nudged until, at EVERY active degree M allows, every row's float64 minimum colour is
    farther than SH_MARGIN from float32(thr)."""
    g = torch.Generator().manual_seed(9000 + 17 * P + M + seed)
    campos = torch.tensor([0.3, -1.7, 2.1], dtype=torch.float32)
    xyz = (torch.randn((P, 3), generator=g) * 1.5).contiguous()
    level = torch.where(torch.arange(P) % 2 == 1, 0.995 + 0.2 * torch.rand((P,), generator=g), -0.3 + 1.3 * torch.rand((P,), generator=g))
    features = torch.randn((P, M, 3), generator=g) * 0.02
    features = torch.where(features.abs() < 1e-3, torch.full_like(features, 1e-3), features)
    features[:, 0, :] = ((level[:, None] + 0.01 * torch.rand((P, 3), generator=g)) - 0.5) / br.C0
    centre = None
    if P > 1:
        centre = P // 2
        xyz[centre] = campos
    top = {1: 0, 4: 1, 9: 2, 16: 3}[M]
    t = float(f32(thr))
    for _ in range(64):
        bad = torch.zeros((P,), dtype=torch.bool)
        for d in range(top + 1):
            mn = br.sh_colour64(xyz, features, d, campos).min(-1).values
            bad |= (mn - t).abs() <= 2 * SH_MARGIN
        if not bool(bad.any()):
            break
        features[bad, 0, :] += 0.004
    stat = 1e-4 + torch.rand((P, 1), generator=g) * 1e-3
    opacity = torch.randn((P, 1), generator=g) * 3.0
    return xyz, features.contiguous(), campos, stat.contiguous(), opacity.contiguous(), centre

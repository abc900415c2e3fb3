"""Constructed scenes for the blend kernels (csrc/gs_render_fwd_wave.hip, gs_render_bwd_wave.hip, gs_blend.h).

The kernels blend four pixels per lane (one per 8x8 quadrant of a 16x16 tile), consume a tile's list in 64-entry
batches with the next batch prefetched, leave the batch loop on a wave-uniform flag and keep "done" in the sign of T.
Random scenes put nothing on those edges on purpose.  The scenes here do: list ends, saturation stops and last
contributors at entry 63 / 64 / 65 / 127 / ... of a tile, quadrants of a lane that disagree, tiles of which only a part
lies inside the image, the alpha rules (0.99 clamp, 1/255 skip) and depth ties.

Every Gaussian is screen-aligned in front of ONE camera at (4, 0, 0) looking down -x, whose axes are world axes (camera
x = world y, y = -z, z = -x): a Gaussian is given by its wanted pixel centre, pixel sigma(s) and view depth and becomes
`means3D` + `cov3D_precomp` + `colors_precomp` + `opacities`, and - where its footprint is axis-aligned - also `scales` +
identity `rotations` (`Case.scene_sr`).  View depths rise strictly in list order (DZ apart) except where a case asks
for a tie.  Pixel centres and variances are chosen on a lattice (integer or half-integer centres, a few fixed
variances), so that the squared distances a pixel can have to a centre are known numbers and alpha = 1/255 falls
between two of them: the margin condition below is met by construction, not by luck.

THE MARGIN CONDITION (`margins`, asserted per case by tests/test_blend_cases_cpu.py).  In the float64 dense model
(tests/dense_reference.py), for every (pixel, entry) pair:
  * |alpha - 1/255| > MARGIN / 255 wherever the entry lies in the pixel's tile rectangle;
  * |T (1 - alpha) - 1e-4| > MARGIN * 1e-4 at every saturation test the pixel performs before (and when) it stops;
  * |opacity exp(power) - 0.99| > 1e-3 on every pair in the rectangle (clamp meant to act: the opacity-1 Gaussians on
    their centre pixel, raw = 1; meant not to act: everything else).
Where a case needs `power <= 0` to hold at |power| ~ 0 (the opacity-1 Gaussians sit ON a pixel centre), it holds in fp32
as in float64 because the conic is positive definite with a cross term that is zero up to the projection's off-axis part:
tests/test_blend_cases_cpu.py asserts b^2 < 1e-6 a c on the fp32 conic of every axis-aligned case (b^2 < a c on the other).
MARGIN = 1e-3 relative: about 15x the worst fp32 error of a 1 300-factor transmittance product (1 300 x 2^-24 = 8e-5).
With it no fp32 implementation can take a skip or stop decision the other way on these scenes, so the GPU tests
(tests/test_gpu_blend_cases.py) exempt no pixel from anything.

Size: every case is at most 64x64 with at most ~1 300 Gaussians, which dense_reference.render evaluates as N pixels x
G Gaussians in float64 with autograd: 240 N G bytes, 80 MB for the 1 025-entry list on its 16x16 image (the largest
case here), 1.3 GB at the allowance's corner.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from gsplat_amd import synthetic

MARGIN = 1e-3
EYE = (4.0, 0.0, 0.0)
FOVX = 0.9
Z0, DZ = 3.0, 1e-3          # view depth of entry i (0-based, list order): Z0 + i DZ
SZ = 0.01                   # thickness along the view axis (world units)
WIDE = 200.3                # pixel sigma of a "wide" Gaussian: alpha varies by < 1 % across a 40-pixel image
FILL = 0.006                # opacity of a wide filler entry: above 1/255 by half, 130 of them leave T = 0.46
KILL = 0.8                  # opacity of a wide killer: five leave T = 3.2e-4, the sixth's test gives 6.4e-5 < 1e-4
VAR_BLOB = 1.3              # pixel variance (incl. the 0.3 dilation) of a narrow blob / stripe: alpha / opacity =
#                             .68 / .21 / .031 / .0021 at distance 1 / 2 / 3 / 4: with opacity <= 0.97 distance 4 is skipped


Case = namedtuple("Case", "name W H scene scene_sr cam bg tile_len meta")
# tile_len: [tiles] expected list length per tile on the reference's lists (from the construction)
# meta: dict; "stop": {tile: 1-based entry at which the whole tile is saturated}, "group": which section of the issue


class Builder:
    def __init__(self, W, H, bg=(0.1, 0.2, 0.3)):
        self.W, self.H = W, H
        self.cam = synthetic.look_at_camera(EYE, W, H, FoVx=FOVX)
        self.fx = W / (2.0 * self.cam.tanfovx)
        self.fy = H / (2.0 * self.cam.tanfovy)
        self.c2w = self.cam.world_view_transform[:3, :3].double().numpy()   # columns: camera axes in the world
        a = np.abs(self.c2w)
        assert np.array_equal(a, np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])), "camera axes must be world axes"
        self.eye = np.asarray(EYE)
        self.bg = torch.tensor(bg)
        self.rows = []       # (mean[3], cov6[6], scales[3] or None, colour[3], opacity, (cx, cy, a, b, c))
        self.next = 0
        self.rng = np.random.RandomState(1234)
        self.gx, self.gy = (W + 15) // 16, (H + 15) // 16

    def add(self, cx, cy, var_x, opacity, var_y=None, theta=None, colour=None, tie=False, visible=True):
        """One Gaussian centred on pixel coordinates (cx, cy) with total pixel variances var_x, var_y (the 0.3 the
        rasterizer adds included) along its axes, the first axis rotated by theta in the image plane (None: axis-aligned,
        so that scales + identity rotation describe it too).  tie: same view depth, bit for bit, as the entry before."""
        var_y = var_x if var_y is None else var_y
        if not tie:
            self.depth = Z0 + self.next * DZ
            self.next += 1
        z = float(np.float32(self.depth)) if visible else -1.0
        zz = abs(z)
        xc = zz * self.cam.tanfovx * ((2.0 * cx + 1.0) / self.W - 1.0)
        yc = zz * self.cam.tanfovy * ((2.0 * cy + 1.0) / self.H - 1.0)
        mean = self.eye + self.c2w @ np.array([xc, yc, z])
        s1, s2 = math.sqrt(var_x - 0.3) * zz / self.fx, math.sqrt(var_y - 0.3) * zz / self.fy
        if theta is None:
            Sc = np.diag([s1 * s1, s2 * s2, SZ * SZ])
            scales = np.abs(self.c2w) @ np.array([s1, s2, SZ])
            a, b, c = var_x, 0.0, var_y
        else:
            R = np.array([[math.cos(theta), -math.sin(theta), 0], [math.sin(theta), math.cos(theta), 0], [0, 0, 1.0]])
            Sc = R @ np.diag([s1 * s1, s2 * s2, SZ * SZ]) @ R.T
            scales = None
            C2 = R[:2, :2] @ np.diag([var_x - 0.3, var_y - 0.3]) @ R[:2, :2].T
            a, b, c = C2[0, 0] + 0.3, C2[0, 1], C2[1, 1] + 0.3
        Sw = self.c2w @ Sc @ self.c2w.T
        cov6 = [Sw[0, 0], Sw[0, 1], Sw[0, 2], Sw[1, 1], Sw[1, 2], Sw[2, 2]]
        if colour is None:
            colour = self.rng.uniform(0.05, 1.0, size=3)
        self.rows.append((mean, cov6, scales, np.asarray(colour, dtype=np.float64), float(opacity), (cx, cy, a, b, c), visible))
        return len(self.rows)

    # ---- the recurring patterns -----------------------------------------------------------------------------------
    def centre(self):
        return (self.W - 1) / 2.0, (self.H - 1) / 2.0

    def wide(self, opacity, n=1, colour=None):
        cx, cy = self.centre()
        for _ in range(n):
            self.add(cx + self.rng.randint(-2, 3), cy + self.rng.randint(-2, 3), WIDE * WIDE, opacity, colour=colour)

    def trailers(self, n=130):
        """entries behind a stop: half opaque, colours up to 20 - one of them blended by mistake shows at once; 0.5 deeper
        than the stop, beyond the margin (5 % + 0.02) of a depth-limited list"""
        self.next += 500
        for _ in range(n):
            self.wide(0.5, colour=self.rng.uniform(5.0, 20.0, size=3))

    def stop_all_at(self, k):
        """the whole image saturates at entry k (1-based, counted from this call's first entry): k - 6 fillers, five
        killers that are blended (T = 3.2e-4 x fillers), a sixth whose test gives < 1e-4"""
        assert k >= 7
        self.wide(FILL, k - 6)
        self.wide(KILL, 6)

    # ---- expected lists ------------------------------------------------------------------------------------------
    def tile_len(self):
        """per tile, how many Gaussians' rectangles hold it: forward.cu's radius / getRect rules applied to the WANTED
        pixel centre and covariance (not to a projection), with the rounding steps required to be clear of an integer"""
        n = np.zeros((self.gy, self.gx), dtype=np.int64)
        for (_, _, _, _, _, (cx, cy, a, b, c), visible) in self.rows:
            if not visible:
                continue
            mid, det = 0.5 * (a + c), a * c - b * b
            lam = mid + math.sqrt(max(0.1, mid * mid - det))
            r3 = 3.0 * math.sqrt(lam)
            assert abs(r3 - round(r3)) > 1e-3, "radius %.6f too close to an integer" % r3
            rad = math.ceil(r3)
            lim = []
            for v, g in ((cx - rad, self.gx), (cy - rad, self.gy), (cx + rad + 15, self.gx), (cy + rad + 15, self.gy)):
                q = v / 16.0
                # (truncation towards zero and the clamp make 0 and everything beyond the grid harmless)
                assert abs(q - round(q)) > 1e-4 or not 1 <= round(q) <= g, "rectangle edge %.6f on a tile border" % q
                lim.append(int(min(max(math.trunc(q), 0), g)))
            n[lim[1]:lim[3], lim[0]:lim[2]] += 1
        return n.reshape(-1)

    def case(self, name, **meta):
        P = len(self.rows)
        f32 = torch.float32
        means = torch.tensor(np.stack([r[0] for r in self.rows]), dtype=f32)
        cov = torch.tensor(np.array([r[1] for r in self.rows]), dtype=f32)
        col = torch.tensor(np.stack([r[3] for r in self.rows]), dtype=f32)
        op = torch.tensor([[r[4]] for r in self.rows], dtype=f32)
        scene = dict(means3D=means, opacities=op, colors_precomp=col, cov3D_precomp=cov, sh_degree=0)
        scene_sr = None
        if all(r[2] is not None for r in self.rows):
            scene_sr = dict(means3D=means, opacities=op, colors_precomp=col, sh_degree=0,
                            scales=torch.tensor(np.stack([r[2] for r in self.rows]), dtype=f32),
                            rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]] * P, dtype=f32))
        assert P <= 1300 and self.W <= 64 and self.H <= 64
        return Case(name, self.W, self.H, scene, scene_sr, self.cam, self.bg, self.tile_len(), meta)


# ---- the cases ----------------------------------------------------------------------------------------------------
LIST_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
STOPS = (63, 64, 65, 127, 128, 129)
PARTIAL_SIZES = ((17, 17), (24, 40), (9, 33), (40, 24))


def _len(n):
    """one tile, n low-opacity entries: nothing saturates (T_final >= exp(-6) = 2.5e-3), every entry reaches every
    pixel, entry n is every pixel's last contributor"""
    b = Builder(16, 16)
    if n == 0:
        b.add(8, 8, 4.0, 0.5, visible=False)      # behind the camera: the tile's list is empty
    b.wide(max(FILL, min(0.3, 6.0 / max(n, 1))), n)
    return b.case("len_%d" % n, group="length", n=n)


def _stop_all(k):
    b = Builder(16, 16)
    b.stop_all_at(k)
    b.trailers()
    return b.case("stop_all_%d" % k, group="stop", stop={0: k})


def _stripes(b, x0, y0, repeats=3):
    """narrow stripes (opacity 0.97, VAR_BLOB across) along the rows y0 + 1, 4, 7, 10, 13 and then along the columns
    x0 + 1, 4, ...: every pixel of rows y0 .. y0 + 14 and of columns x0 .. x0 + 14 lies within 1 of a stripe's axis and takes
    alpha >= 0.66 from it `repeats` times; row y0 + 15 and column x0 + 15 lie at distance 2 (alpha 0.21)"""
    for c in (1, 4, 7, 10, 13):
        for _ in range(repeats):
            b.add(b.centre()[0], y0 + c, WIDE * WIDE, 0.97, var_y=VAR_BLOB)
    for c in (1, 4, 7, 10, 13):
        for _ in range(repeats):
            b.add(x0 + c, b.centre()[1], VAR_BLOB, 0.97, var_y=WIDE * WIDE)


def _stop_last(k):
    """all pixels but (15, 15) are dead after 34 entries (four wide killers, then stripes that spare the last row and
    column crossing); the corner pixel lives on at T ~ 4e-4 through the fillers and dies at entry k"""
    b = Builder(16, 16)
    b.wide(KILL, 4)
    _stripes(b, 0, 0)
    assert b.next == 34
    b.wide(FILL, k - 1 - b.next)
    b.wide(KILL, 1)
    assert b.next == k
    b.trailers()
    return b.case("stop_last_%d" % k, group="stop", stop={0: k}, last_pixel=(15, 15))


def _quad_early():
    """quadrant 0 (x, y < 8) saturates inside the first batch (four wide killers, then blobs on a 3 x 3 lattice inside
    it), the other three run to the end of the 200-entry list"""
    b = Builder(16, 16)
    b.wide(KILL, 4)
    for _ in range(5):
        for cy in (1.0, 3.5, 6.0):
            for cx in (1.0, 3.5, 6.0):
                b.add(cx, cy, VAR_BLOB, 0.95)
    b.wide(0.0045, 200 - b.next)
    return b.case("quad_early_sat", group="quadrant", early=0, n=200)


def _quad_only(q):
    """100 narrow blobs inside quadrant q; the other three quadrants receive nothing (distance >= 4: alpha < 1/255)"""
    b = Builder(16, 16)
    ox, oy = (q & 1) * 8, (q >> 1) * 8
    for i in range(100):
        b.add(ox + 3.0 + 0.5 * (i % 4), oy + 3.0 + 0.5 * ((i // 4) % 4), VAR_BLOB, 0.05)
    return b.case("quad_only_%d" % q, group="quadrant", only=q)


def _quad_four_batches():
    """batch b (entries 64 b + 1 .. 64 b + 64) lies inside quadrant b: the four pixels of a lane have their last
    contributors in four different batches"""
    b = Builder(16, 16)
    for q in range(4):
        ox, oy = (q & 1) * 8, (q >> 1) * 8
        for i in range(64):
            b.add(ox + 3.0 + 0.5 * (i % 4), oy + 3.0 + 0.5 * ((i // 4) % 4), VAR_BLOB, 0.05)
    return b.case("quad_four_batches", group="quadrant")


def _partial(W, H, kind):
    """tiles cut by the image border, each holding the whole list (wide Gaussians): 257 entries that never saturate, or a
    stop of every tile at entry 128 with 130 entries behind it"""
    b = Builder(W, H)
    if kind == "len":
        b.wide(0.02, 257)
        return b.case("partial_%dx%d_len257" % (W, H), group="partial", n=257)
    b.stop_all_at(128)
    b.trailers()
    return b.case("partial_%dx%d_stop128" % (W, H), group="partial", stop={t: 128 for t in range(b.gx * b.gy)})


def _partial_inside_stop():
    """9x33: three tiles of which columns 9 .. 15 lie outside the image.  Killers centred on column 2 (variance 8 across,
    wide along y) reach the inside columns (alpha 0.10 on column 8, which dies last, at entry INSIDE_STOP) and NOT columns
    12 .. 15: a kernel that let outside pixels live would never see these tiles stop."""
    b = Builder(9, 33)
    for _ in range(INSIDE_STOP):
        b.add(2, 16, 8.0, 0.97, var_y=WIDE * WIDE)
    b.trailers()
    return b.case("partial_9x33_inside_stop", group="partial", stop={0: INSIDE_STOP, 1: INSIDE_STOP, 2: INSIDE_STOP},
                  outside_alive=(12, 16))


INSIDE_STOP = 86    # 0.8978^85 = 1.05e-4 is the last test above 1e-4 on column 8 (margin 5 %), the 86th gives 9.4e-5


def _opaque(pos):
    """opacity 1.0 centred on pixel (5, 9) as entry `pos` of 130: alpha is clamped to 0.99 there (raw 1.0) and nowhere else
    (variance 4: raw <= 0.88 one pixel away)"""
    b = Builder(16, 16)
    b.wide(FILL, pos - 1)
    b.add(5, 9, 4.0, 1.0)
    b.wide(FILL, 130 - pos)
    return b.case("opaque_entry_%d" % pos, group="alpha", clamp=(pos, 5, 9))


def _subthreshold():
    """entries 62 .. 66 and the last two lie in the tile's rectangle and reach no pixel of it (a blob 2.9 pixels left of
    the image at opacity 0.05: alpha <= 0.002): they count in the numbering and are nobody's last contributor"""
    b = Builder(16, 16)
    b.wide(0.02, 61)
    for i in range(5):
        b.add(-2.9, 3.0 + 2 * i, VAR_BLOB, 0.05)
    b.wide(0.02, 64)
    for i in range(2):
        b.add(-2.9, 5.0 + 4 * i, VAR_BLOB, 0.05)
    return b.case("alpha_subthreshold", group="alpha", skipped=(62, 63, 64, 65, 66, 131, 132))


def _low_opacity():
    """wide Gaussians of opacity 0.002 < 1/255 as entries 1, 64, 65 and last (CULL's L2 < 0 branch; the culled lists
    drop them altogether)"""
    b = Builder(16, 16)
    b.wide(0.002, 1)
    b.wide(0.02, 62)
    b.wide(0.002, 2)
    b.wide(0.02, 64)
    b.wide(0.002, 1)
    return b.case("alpha_low_opacity", group="alpha", skipped=(1, 64, 65, 130))


def _diagonal():
    """32x32, four tiles.  An ellipse of variances 150 x 4 along the anti-diagonal, centred at (19.5, 19.5) in tile
    (1, 1): its long axis runs into tiles (1, 0) and (0, 1), and across the corner it reaches tile (0, 0) at exactly one
    pixel, (15, 15) (alpha 0.0057; its neighbours 0.0017).  No list rule may drop it from tile 0."""
    b = Builder(32, 32)
    b.wide(0.02, 3)
    b.add(19.5, 19.5, 150.0, 0.9, var_y=4.0, theta=-math.pi / 4, colour=(3.0, 0.2, 2.0))
    b.wide(0.02, 3)
    return b.case("alpha_diagonal_corner", group="alpha", corner_pixel=(15, 15), ellipse=4)


def _ties(run):
    """`run` Gaussians at one view depth, bit for bit, between ordinary entries (the 70-run straddles entry 64): they
    blend in index order, and with alpha 0.03 .. 0.14 and random colours any other order moves the image by ~ 1e-3"""
    b = Builder(16, 16)
    b.wide(0.02, 30 if run > 3 else 10)
    for i in range(run):
        b.add(4.0 + (i % 5) * 2, 4.0 + ((i // 5) % 5) * 2, 9.0 if i % 2 else WIDE * WIDE, 0.03 + 0.12 * ((i * 7) % 10) / 10.0,
              tie=i > 0)
    b.wide(0.02, 10)
    return b.case("ties_%d" % run, group="ties", run=run)


def _table():
    t = [(lambda n=n: _len(n), "len_%d" % n) for n in LIST_LENGTHS]
    t += [(lambda k=k: _stop_all(k), "stop_all_%d" % k) for k in STOPS]
    t += [(lambda k=k: _stop_last(k), "stop_last_%d" % k) for k in STOPS]
    t += [(_quad_early, "quad_early_sat")] + [(lambda q=q: _quad_only(q), "quad_only_%d" % q) for q in range(4)]
    t += [(_quad_four_batches, "quad_four_batches")]
    for W, H in PARTIAL_SIZES:
        t += [(lambda W=W, H=H: _partial(W, H, "len"), "partial_%dx%d_len257" % (W, H)),
              (lambda W=W, H=H: _partial(W, H, "stop"), "partial_%dx%d_stop128" % (W, H))]
    t += [(_partial_inside_stop, "partial_9x33_inside_stop")]
    t += [(lambda p=p: _opaque(p), "opaque_entry_%d" % p) for p in (1, 64, 65)]
    t += [(_subthreshold, "alpha_subthreshold"), (_low_opacity, "alpha_low_opacity"), (_diagonal, "alpha_diagonal_corner")]
    t += [(lambda r=r: _ties(r), "ties_%d" % r) for r in (3, 70)]
    return t


TABLE = _table()                      # [(constructor, name)]: CPU and GPU tests parametrize over NAMES
NAMES = [name for _, name in TABLE]
NO_SCALES_ROTATIONS = ("alpha_diagonal_corner",)   # cases whose scene_sr is None
_BUILT = {}


def build(name):
    if name not in _BUILT:
        c = dict((n, f) for f, n in TABLE)[name]()
        assert c.name == name
        _BUILT[name] = c
    return _BUILT[name]


def cotangents(case):
    g = torch.Generator().manual_seed(1000 + NAMES.index(case.name))
    return torch.randn((3, case.H, case.W), generator=g), torch.randn((1, case.H, case.W), generator=g) * 0.3


_DENSE = {}


def dense(case, which="scene"):
    """-> (outputs incl. `detail`, gradients) of the float64 model with this case's cotangents; cached per process"""
    key = (case.name, which)
    if key not in _DENSE:
        import dense_reference
        sc = getattr(case, which)
        leaves, d = {}, {}
        for k, v in sc.items():
            if torch.is_tensor(v):
                leaves[k] = v.double().clone().requires_grad_(True)
                d[k] = leaves[k]
            else:
                d[k] = v
        P = sc["means3D"].shape[0]
        d["ndc_probe"] = leaves["ndc_probe"] = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
        out = dense_reference.render(d, case.cam, case.bg, False, detail=True)
        dc, di = cotangents(case)
        ((out["color"] * dc.double()).sum() + (out["invdepth"] * di.double()).sum()).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        _DENSE[key] = ({k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, grads)
    return _DENSE[key]


def margins(detail):
    """the margin condition's three distances, each as (smallest margin found / the margin required): all must be > 1"""
    r, t = detail["in_rect"], detail["tested"]
    alpha = detail["raw"].clamp(max=0.99)
    big = torch.tensor(float("inf"), dtype=torch.float64)
    m_alpha = torch.where(r & (detail["power"] <= 0), (alpha - 1.0 / 255.0).abs(), big).min() if r.any() else big
    m_T = torch.where(t, (detail["test_T"] - 1e-4).abs(), big).min() if t.any() else big
    m_clamp = torch.where(r, (detail["raw"] - 0.99).abs(), big).min() if r.any() else big
    return dict(alpha=float(m_alpha) / (MARGIN / 255.0), T=float(m_T) / (MARGIN * 1e-4), clamp=float(m_clamp) / 1e-3)

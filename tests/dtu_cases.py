"""Constructed inputs for the DTU kernels (csrc/gs_dng_dtu.hip), shared by tests/test_dtu_cpu.py (which proves the table) and
tests/test_gpu_dtu_kernels.py (which holds the kernels to it).  Everything is float32 on the CPU, built from fixed seeds."""
import torch

MASK_SIZES = ((1, 1), (49, 3), (50, 64), (51, 65), (130, 130), (300, 400))
FILL_SIZES = ((1, 1), (7, 5), (64, 64), (63, 257), (300, 400))
MASK_KINDS = ("none", "all_but_one", "all", "half")
RULE_P = (1, 63, 64, 65, 257, 1000)
THRESHOLDS = (15 / 255, 20 / 255, 30 / 255, 240 / 255)
INF = torch.tensor(float("inf"))


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def around(thr):
    """float32(thr) and its two neighbours -> (below, at, above) as Python floats"""
    t = f32(thr)
    return float(torch.nextafter(t, -INF)), float(t), float(torch.nextafter(t, INF))


def run_specs(H):
    """(start row, length) of the constructed dark runs that fit H rows: 48 / 49 / 50 / 51 rows starting at row 0, starting
    mid-column, and ending at the last row"""
    out = []
    for L in (48, 49, 50, 51):
        for start in (0, H // 3, H - L):
            if start >= 0 and start + L <= H and (start, L) not in out:
                out.append((start, L))
    return out


def mask_image(H, W, thr, kind="runs", seed=0):
    """gt [3,H,W].  "runs": bright everywhere but for the constructed dark runs (one spec per column, the specs cycling over
    the first two thirds of the columns), columns of random dark speckle behind them, and a last column that is dark top to
    bottom but for three rows whose channel maximum is float32(thr) (not dark) / its lower neighbour (dark) / its upper one
    (not dark).  "dark" / "bright": every pixel on one side."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    bright = 0.5 + 0.5 * torch.rand((3, H, W), generator=g)
    dark = 0.9 * thr * torch.rand((3, H, W), generator=g)
    if kind == "dark":
        return dark
    if kind == "bright":
        return bright
    is_dark = torch.zeros((H, W), dtype=torch.bool)
    specs = run_specs(H)
    n_run_cols = (2 * W) // 3
    for x in range(n_run_cols):
        if specs:
            s, L = specs[x % len(specs)]
            is_dark[s:s + L, x] = True
    for x in range(n_run_cols, W):
        is_dark[:, x] = torch.rand((H,), generator=g) < 0.97
    gt = torch.where(is_dark[None], dark, bright)
    if W >= 2:
        x = W - 1
        gt[:, :, x] = dark[:, :, x]
        below, at, above = around(thr)
        for k, v in enumerate((at, below, above)):
            y = (H // 4) * (k + 1)
            if 0 < y < H:
                gt[:, y, x] = 0.5 * v      # the other two channels stay under the maximum
                gt[k % 3, y, x] = v
    return gt.contiguous()


def fill_mask(H, W, kind, seed=0):
    g = torch.Generator().manual_seed(77 * H + W + seed)
    n = H * W
    if kind == "none":
        m = torch.zeros((n,), dtype=torch.bool)
    elif kind == "all":
        m = torch.ones((n,), dtype=torch.bool)
    elif kind == "all_but_one":
        m = torch.ones((n,), dtype=torch.bool)
        m[(2 * n) // 3] = False
    else:
        m = torch.rand((n,), generator=g) < 0.5
    return m.reshape(1, H, W)


def fill_image(H, W, seed=0):
    """non-negative, of the size of a depth or of 255 - mono"""
    g = torch.Generator().manual_seed(31 * H + W + seed)
    return (torch.rand((1, H, W), generator=g) * 200.0).contiguous()


def alpha_image(H, W, seed=0):
    g = torch.Generator().manual_seed(13 * H + W + seed)
    a = torch.rand((1, H, W), generator=g)
    a.view(-1)[3::7] = 0.0     # pixels nothing was blended into
    return a.contiguous()


def rule_rows(P, black_thr=20 / 255, white_thr=240 / 255, seed=0):
    """colour [P,3], stat [P,1], opacity_raw [P,1]: a third of the rows dark, a third bright, the rest in between; the first
    rows sit on the thresholds: max_c at float32(black_thr) and its neighbours, min_c at float32(white_thr) and its neighbours"""
    g = torch.Generator().manual_seed(500 + P + seed)
    u = torch.rand((P, 3), generator=g)
    cls = torch.arange(P) % 3
    colour = torch.where(cls[:, None] == 0, u * black_thr * 0.99, torch.where(cls[:, None] == 1, white_thr + (1 - white_thr) * u, u))
    edge = []
    for v in around(black_thr):
        edge.append((v, 0.5 * v, 0.25 * v))           # max_c = v
    for v in around(white_thr):
        edge.append((v, 0.5 + 0.5 * v, 1.0))          # min_c = v
    for i, row in enumerate(edge):
        if i < P:
            colour[(7 * i) % P] = torch.tensor(row, dtype=torch.float32).roll(i % 3)
    stat = torch.rand((P, 1), generator=g) * 1e-3
    opacity = torch.randn((P, 1), generator=g)
    return colour.contiguous(), stat.contiguous(), opacity.contiguous()


RULE_FORMS = (   # (black, white) of dng_reg.colour_rule
    ((20 / 255, 10, True), (240 / 255, 2, True)),
    ((20 / 255, 10, True), (240 / 255, 2, False)),
    ((20 / 255, 10, False), None),
    (None, (240 / 255, 2, True)),
    (None, None),
    ((0.6, 10, True), (0.4, 2, False)),   # thresholds that overlap: a row both rules fire on is divided twice, black first
)


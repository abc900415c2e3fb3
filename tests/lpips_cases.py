"""Seeded weights and the case tables of the LPIPS tests (test_lpips_cpu.py, test_gpu_lpips.py, golden/make_golden_lpips.py,
tools/lpips_timing.py).  No run here has seen the real weight files: VGG16 and the lin layers are filled from a seed, in the
real files' shapes and key names."""
import numpy as np
import torch

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision vgg16().features
CONV_SHAPE = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
              (512, 512), (512, 512), (512, 512))
PAIRS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512))   # the eight distinct ones
BLOCK_CONVS = (2, 2, 3, 3, 3)
TAP_CHANNELS = (64, 128, 256, 512, 512)
WEIGHT_SEED = 20240607


def make_state_dicts(seed=WEIGHT_SEED, signed_lin=False, renamed=False):
    """-> (vgg_sd, lin_sd) of fp32 CPU tensors.  Convolutions N(0, 2 / (9 Cin)) (He: activations keep their scale through
    thirteen layers), biases N(0, 0.05^2), lin weights uniform [0, 1) - the real ones are non-negative - or, signed_lin,
    uniform [-0.5, 0.5).  renamed: the lin keys as the reference's get_state_dict leaves them ({k}.1.weight)."""
    rng = np.random.default_rng(seed)
    vgg = {}
    for i, (cin, cout) in zip(CONV_INDEX, CONV_SHAPE):
        vgg["features.%d.weight" % i] = torch.from_numpy(
            (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
        vgg["features.%d.bias" % i] = torch.from_numpy((rng.standard_normal((cout,)) * 0.05).astype(np.float32))
    lin = {}
    for k, c in enumerate(TAP_CHANNELS):
        v = rng.random((1, c, 1, 1)) - (0.5 if signed_lin else 0.0)
        lin[("%d.1.weight" if renamed else "lin%d.model.1.weight") % k] = torch.from_numpy(v.astype(np.float32))
    return vgg, lin


# ---- whole-call cases: (name, H, W, image seed).  16 x 16 is the minimum (the fifth tap is 1 x 1); the others put an odd
# height or width in front of every one of the four pools (pool_sizes below; test_lpips_cpu proves it)
WHOLE_CASES = (("min_16x16", 16, 16, 1), ("17x19", 17, 19, 2), ("35x50", 35, 50, 3), ("48x64", 48, 64, 4), ("75x100", 75, 100, 5))


def whole_images(H, W, seed):
    """-> (render, gt) uint8 [H,W,3]: a smooth random ground truth and a render that is the ground truth plus noise (LPIPS of
    a few hundredths, the range a sparse-view model leaves)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9), rng.uniform(0, 6.28)
            gt[:, :, c] += rng.uniform(0.1, 0.3) * np.sin(fy * yy + fx * xx + ph)
        gt[:, :, c] += 0.5 + 0.08 * rng.standard_normal((H, W))
    render = gt + 0.1 * rng.standard_normal((H, W, 3))
    to_u8 = lambda a: np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)   # noqa: E731
    return to_u8(render), to_u8(gt)


def planar(u8):
    """to_tensor: uint8 [H,W,3] -> fp32 [3,H,W] = byte / 255"""
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).to(torch.float32).div(255.0).contiguous()


def pool_sizes(H, W):
    """the (h, w) entering each of the four pools"""
    out = []
    for _ in range(4):
        out.append((H, W))
        H, W = H // 2, W // 2
    return out


# ---- convolution, exact: integer data whose every partial sum is an integer below 2^24 whatever the order
CONV_SIZES = ((1, 1), (1, 37), (37, 1), (16, 16), (33, 31), (64, 65))   # below, at and off the 32-column / 4- and 8-row tiles
INT_X_MAX, INT_W_MAX, INT_B_MAX = 3, 2, 8


def int_conv_case(cin, cout, H, W, seed):
    """x in {0..3} [2,cin,H,W], w in {-2..2}, integer b in {-8..8}"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, INT_X_MAX + 1, (2, cin, H, W)).astype(np.float32))
    w = torch.from_numpy(rng.integers(-INT_W_MAX, INT_W_MAX + 1, (cout, cin, 3, 3)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-INT_B_MAX, INT_B_MAX + 1, (cout,)).astype(np.float32))
    return x, w, b


def int_conv_bound(cin):
    """the largest |partial sum| any order of summation can meet"""
    return 9 * cin * INT_X_MAX * INT_W_MAX + INT_B_MAX


def large_tile_size(cout):
    """The kernel has two tile shapes: 8 x 32 pixels x 64 channels when that grid has at least 256 workgroups, else 4 x 32
    pixels x 32 channels.  CONV_SIZES reach the first only for Cout = 512 (64 x 65), so every pair is also run at the smallest
    (H, 33) that selects it for N = 2: two column tiles, the second one pixel wide, and a one-row last tile."""
    tiles_y = 128 // (2 * (cout // 64))
    return (8 * (tiles_y - 1) + 1, 33)


def conv_workgroups_large(N, cout, H, W):
    return N * ((W + 31) // 32) * ((H + 7) // 8) * (cout // 64)


# ---- convolution, random data: a size on the small tile shape and the pair's large_tile_size
RANDOM_CONV_SMALL = (9, 35)


def random_conv_case(cin, cout, H, W, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(np.maximum(rng.standard_normal((2, cin, H, W)), 0).astype(np.float32))   # (post-ReLU-like)
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal((cout,)) * 0.05).astype(np.float32))
    return x, w, b


# ---- pool: (H, W) of the input, odd and even, down to a 1 x 1 output
POOL_SIZES = ((2, 2), (3, 3), (2, 5), (7, 4), (16, 16), (33, 31), (5, 64))

# ---- distance: (C, H, W)
DIST_SHAPES = ((64, 1, 1), (512, 1, 1), (64, 23, 31), (512, 23, 31))


def dist_case(C, H, W, seed, signed_lin=False, zero_pixel=False):
    """features like a tap's: non-negative, about a third of them zero.  zero_pixel: pixel (0, 0) of fx is all zero."""
    rng = np.random.default_rng(seed)
    fx = np.maximum(rng.standard_normal((C, H, W)) + 0.4, 0).astype(np.float32)
    fy = np.maximum(fx + 0.2 * rng.standard_normal((C, H, W)), 0).astype(np.float32)
    if zero_pixel:
        fx[:, 0, 0] = 0.0
    lin = (rng.random((C,)) - (0.5 if signed_lin else 0.0)).astype(np.float32)
    return torch.from_numpy(fx), torch.from_numpy(fy), torch.from_numpy(lin)

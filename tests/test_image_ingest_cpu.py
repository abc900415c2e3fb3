"""Image ingest on the host (gsplat_amd/imageio.py: resize_alpha_u8, ingest_image and their unit rules) - the arbiter of the
device path (tests/test_gpu_image_ingest.py).  No Pillow here: tests/golden/pil_resize_alpha.npz carries its bytes."""
import os

import numpy as np
import pytest
import torch

import image_ingest_cases as cases
from gsplat_amd import imageio
from gsplat_amd import io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_resize_alpha.npz")
CASES = cases.fixture_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def all_pairs():
    """uint8 [256,256,2]: [a, c] = (c, a) - every colour byte against every alpha byte"""
    c, a = np.meshgrid(np.arange(256), np.arange(256))
    return np.stack([c, a], axis=2).astype(np.uint8)


def test_fixture_covers_what_it_should(golden):
    keys = [c[0] for c in CASES]
    assert len(set(keys)) == len(keys) == 34
    assert sorted(k[:-4] for k in golden.files if k.endswith("_crc")) == sorted(keys)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert any(W2 % 2 == 1 and C == 2 for _, _, _, (H2, W2), C in CASES), "an LA row that is no whole number of words"
    assert any((H, W) == (H2, W2) for _, _, (H, W), (H2, W2), _ in CASES)


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_numpy_path_equals_pillows_recorded_bytes(golden, key):
    _, make, (H, W), (H2, W2), C = next(c for c in CASES if c[0] == key)
    a = make()
    assert cases.crc(a) == int(golden[key + "_crc"]), "the seeded input is not the generator's"
    want = cases.expected(golden, key, a)
    got = imageio.resize_alpha_u8(a, (W2, H2))
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (H2, W2, C)
    assert np.array_equal(got, want), int((got != want).sum())
    t = imageio.resize_alpha_u8(torch.from_numpy(a), (W2, H2))
    assert torch.is_tensor(t) and not t.is_cuda and np.array_equal(t.numpy(), want)
    if (H, W) == (H2, W2):
        assert got is not a and not np.shares_memory(got, a), "the same size is a copy"


def test_premultiply_and_unpremultiply_over_every_pair():
    px = all_pairs()
    pre = imageio.premultiply_u8(px)
    un = imageio.unpremultiply_u8(px)
    assert np.array_equal(pre[:, :, 1], px[:, :, 1]) and np.array_equal(un[:, :, 1], px[:, :, 1]), "alpha is unchanged"
    for a in range(256):
        for c in range(256):
            t = c * a + 128
            assert pre[a, c, 0] == ((t >> 8) + t) >> 8, (c, a)
            assert un[a, c, 0] == (c if a in (0, 255) else min(255, (255 * c) // a)), (c, a)
    rgba = np.repeat(px[:, :, :1], 3, axis=2)
    rgba = np.concatenate((rgba, px[:, :, 1:]), axis=2)
    assert np.array_equal(imageio.premultiply_u8(rgba)[:, :, 2], pre[:, :, 0])
    assert np.array_equal(imageio.unpremultiply_u8(rgba)[:, :, 1], un[:, :, 0])


@pytest.mark.parametrize("white", [False, True])
def test_composite_over_every_pair_is_io_composite_rgba(white):
    px = all_pairs()
    rgba = np.concatenate((np.repeat(px[:, :, :1], 3, axis=2), px[:, :, 1:]), axis=2)
    q = imageio.composite_u8_numpy(rgba, white)
    want = gio.composite_rgba(rgba, white)
    assert q.dtype == np.uint8 and q.shape == (256, 256, 3)
    assert np.array_equal(np.transpose(q.astype(np.float32) / np.float32(255), (2, 0, 1)), want)
    image, mask = imageio.ingest_image(rgba, (256, 256), white_background=white)
    assert np.array_equal(image, want) and image.dtype == np.float32
    assert np.array_equal(mask, np.ones((1, 256, 256), dtype=np.float32)), "a composited image has no alpha mask"


def test_ingest_image_is_resize_then_byte_over_255_and_the_cameras_mask():
    rgba = cases.seeded(37, 53, 4, 11)
    rgb = np.ascontiguousarray(rgba[:, :, :3])
    W2, H2 = 26, 19
    r4 = imageio.resize_alpha_u8_numpy(rgba, (W2, H2))
    image, mask = imageio.ingest_image(rgba, (W2, H2))
    planes = r4.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(image, planes[:3]) and np.array_equal(mask, planes[3:4])
    assert image.flags["C_CONTIGUOUS"] and image.shape == (3, H2, W2) and mask.shape == (1, H2, W2)
    for is_test_view in (False, True):
        for is_test_dataset in (False, True):
            kw = dict(train_test_exp=True, is_test_view=is_test_view, is_test_dataset=is_test_dataset)
            _, m = imageio.ingest_image(rgba, (W2, H2), **kw)
            assert np.array_equal(m, gio.camera_alpha_mask(planes, **kw).numpy())
            i3, m3 = imageio.ingest_image(rgb, (W2, H2), **kw)
            want3 = imageio.resize_u8_numpy(rgb, (W2, H2)).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            assert np.array_equal(i3, want3) and np.array_equal(m3, gio.camera_alpha_mask(want3, **kw).numpy())
    _, m = imageio.ingest_image(rgba, (W2, H2), train_test_exp=False, is_test_view=True)
    assert np.array_equal(m, planes[3:4]), "without train_test_exp no half is zeroed"
    # a CPU tensor gives CPU tensors; the same size keeps the bytes
    ti, tm = imageio.ingest_image(torch.from_numpy(rgba), (53, 37))
    assert torch.is_tensor(ti) and np.array_equal(ti.numpy(), rgba[:, :, :3].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    assert np.array_equal(tm.numpy()[0], rgba[:, :, 3].astype(np.float32) / np.float32(255))
    # NeRF-synthetic: the composite happens at the source size, then the image is resized as RGB; an RGB file gets alpha 255
    for white in (False, True):
        image, mask = imageio.ingest_image(rgba, (W2, H2), white_background=white)
        comp = imageio.composite_u8_numpy(rgba, white)
        assert np.array_equal(image, imageio.resize_u8_numpy(comp, (W2, H2)).transpose(2, 0, 1).astype(np.float32) / np.float32(255))
        assert float(mask.min()) == 1.0
        i3, _ = imageio.ingest_image(rgb, (53, 37), white_background=white)
        opaque = np.concatenate((rgb, np.full((37, 53, 1), 255, dtype=np.uint8)), axis=2)
        assert np.array_equal(i3, gio.composite_rgba(opaque, white))


def test_refusals():
    with pytest.raises(ValueError, match="C in 3/4"):
        imageio.ingest_image(np.zeros((4, 4, 2), dtype=np.uint8), (2, 2))
    with pytest.raises(ValueError, match="C in 2/4"):
        imageio.resize_alpha_u8(np.zeros((4, 4, 3), dtype=np.uint8), (2, 2))
    with pytest.raises(ValueError, match="uint8 only"):
        imageio.ingest_image(np.zeros((4, 4, 3), dtype=np.float32), (2, 2))
    with pytest.raises(ValueError, match=">= 1"):
        imageio.resize_alpha_u8(np.zeros((4, 4, 4), dtype=np.uint8), (0, 2))
    with pytest.raises(ValueError, match="premultiplies"):   # resize_u8 keeps refusing alpha: that is resize_alpha_u8's
        imageio.resize_u8(np.zeros((4, 4, 4), dtype=np.uint8), (2, 2))

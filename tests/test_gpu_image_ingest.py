"""Image ingest on the device (csrc/gs_image_ingest.hip, gsplat_amd/imageio.py): everything is exact.

Resize of LA / RGBA: every case of tests/golden/pil_resize_alpha.npz - Pillow's recorded bytes - with torch.equal.  The planar
image is bitwise byte / 255, the alpha mask the alpha byte / 255 (or ones), both half-masks as io.camera_alpha_mask zeroes them.
The composite equals the host path (numpy float64, which tests/test_image_ingest_cpu.py holds to io.composite_rgba) over all
65 536 (colour, alpha) pairs and both backgrounds.  Every output and the scratch - of exactly gs_image_ingest_tmp_bytes - sit
between guard patterns.  No Pillow here."""
import os

import numpy as np
import pytest
import torch

import image_ingest_cases as cases
from gsplat_amd import imageio
from gsplat_amd import io as gio

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_resize_alpha.npz")
E_NULL, E_SHAPE = -1, -2
CASES = cases.fixture_cases()
GUARD, PAD = 0xA5, 256
COMPOSITE, WHITE, ZERO_LEFT, ZERO_RIGHT = 1, 2, 4, 8
ORDER = ("inp", "H", "W", "C", "H2", "W2", "xb", "xc", "kx", "yb", "yc", "ky", "flags", "tmp", "tmp_bytes", "out", "image", "alpha")


def raw_ingest(hip, src, H2, W2, flags=0, u8=True, planes=True, override=None):
    """gs_image_ingest itself, outputs and scratch between guards, scratch of exactly gs_image_ingest_tmp_bytes
    -> (status, bytes or None, image or None, alpha or None, guards intact?, nothing written at all?)"""
    H, W, C = src.shape
    Ce = 3 if flags & COMPOSITE else C
    api = hip.api
    nb = int(api.raw("image_ingest_tmp_bytes")(H, W, C, H2, W2, flags))
    n_px = H2 * W2
    obuf = torch.full((PAD + n_px * Ce + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    tbuf = torch.full((PAD + nb + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    ibuf = torch.full((64 + 3 * n_px + 64,), -7.0, dtype=torch.float32, device=DEV)
    abuf = torch.full((64 + n_px + 64,), -7.0, dtype=torch.float32, device=DEV)
    xb, xc = imageio._tables_on(DEV, W, W2) if W2 != W else (None, None)
    yb, yc = imageio._tables_on(DEV, H, H2) if H2 != H else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = dict(inp=src.data_ptr(), H=H, W=W, C=C, H2=H2, W2=W2, xb=ptr(xb), xc=ptr(xc), kx=0 if xc is None else xc.shape[1],
                yb=ptr(yb), yc=ptr(yc), ky=0 if yc is None else yc.shape[1], flags=flags, tmp=(tbuf.data_ptr() + PAD) if nb else None,
                tmp_bytes=nb, out=(obuf.data_ptr() + PAD) if u8 else None, image=(ibuf.data_ptr() + 256) if planes else None,
                alpha=(abuf.data_ptr() + 256) if planes else None)
    args.update(override or {})
    rc = api.raw("image_ingest")(*[args[k] for k in ORDER], None)
    torch.cuda.synchronize()
    intact = (bool((obuf[:PAD] == GUARD).all()) and bool((obuf[PAD + n_px * Ce:] == GUARD).all())
              and bool((tbuf[:PAD] == GUARD).all()) and bool((tbuf[PAD + nb:] == GUARD).all())
              and bool((ibuf[:64] == -7.0).all()) and bool((ibuf[64 + 3 * n_px:] == -7.0).all())
              and bool((abuf[:64] == -7.0).all()) and bool((abuf[64 + n_px:] == -7.0).all()))
    untouched = all(bool((b == v).all()) for b, v in ((obuf, GUARD), (tbuf, GUARD), (ibuf, -7.0), (abuf, -7.0)))
    return (rc, obuf[PAD:PAD + n_px * Ce].reshape(H2, W2, Ce) if u8 else None, ibuf[64:64 + 3 * n_px].reshape(3, H2, W2) if planes else None,
            abuf[64:64 + n_px].reshape(1, H2, W2) if planes else None, intact, untouched)


def planes_of(u8):
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).to(torch.float32).div(255).contiguous()


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_alpha_resize_equals_pillows_recorded_bytes(hip, key):
    z = np.load(GOLDEN)
    _, make, (H, W), (H2, W2), C = next(c for c in CASES if c[0] == key)
    a = make()
    assert cases.crc(a) == int(z[key + "_crc"]), "the seeded input is not the generator's"
    want = torch.from_numpy(cases.expected(z, key, a))
    src = torch.from_numpy(a).to(DEV)
    rc, got, image, alpha, intact, _ = raw_ingest(hip, src, H2, W2, planes=C == 4)
    assert rc == 0 and intact, "a guard byte around an output or the scratch was written"
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    if C == 4:
        p = planes_of(want.numpy())
        assert torch.equal(image.cpu(), p[:3]), "the planar image is not byte / 255"
        assert torch.equal(alpha.cpu(), p[3:4]), "the alpha mask is not alpha byte / 255"
        # without the bytes, and with one half of the mask zeroed each way
        for flags, kw in ((ZERO_LEFT, dict(is_test_dataset=True)), (ZERO_RIGHT, dict(is_test_dataset=False))):
            rc, none, image, alpha, intact, _ = raw_ingest(hip, src, H2, W2, flags=flags, u8=False)
            assert rc == 0 and intact and none is None and torch.equal(image.cpu(), p[:3])
            assert torch.equal(alpha.cpu(), gio.camera_alpha_mask(p, train_test_exp=True, is_test_view=True, **kw))
        gi, ga = imageio.ingest_image(src, (W2, H2))
        hi, ha = imageio.ingest_image(a, (W2, H2))
        assert gi.is_cuda and np.array_equal(gi.cpu().numpy(), hi) and np.array_equal(ga.cpu().numpy(), ha)
    out = imageio.resize_alpha_u8(src, (W2, H2))
    assert out.is_cuda and out.dtype == torch.uint8 and torch.equal(out.cpu(), want)


RGB_SIZES = (((53, 37), (26, 19)), ((16, 16), (40, 31)), ((37, 53), (37, 26)), ((53, 26), (19, 26)), ((21, 17), (21, 17)), ((1, 1), (3, 3)))


@pytest.mark.parametrize("size", RGB_SIZES)
def test_rgb_is_the_resize_with_a_mask_of_ones(hip, size):
    (H, W), (H2, W2) = size
    a = np.ascontiguousarray(cases.seeded(H, W, 4, 500 + H + W)[:, :, :3])
    want = imageio.resize_u8_numpy(a, (W2, H2))   # (tests/test_image_files_cpu.py holds it to Pillow's bytes)
    p = planes_of(want)
    src = torch.from_numpy(a).to(DEV)
    rc, got, image, alpha, intact, _ = raw_ingest(hip, src, H2, W2)
    assert rc == 0 and intact and torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(image.cpu(), p)
    assert torch.equal(alpha.cpu(), torch.ones(1, H2, W2))
    for is_test_dataset in (False, True):
        kw = dict(train_test_exp=True, is_test_view=True, is_test_dataset=is_test_dataset)
        gi, ga = imageio.ingest_image(src, (W2, H2), **kw)
        assert torch.equal(gi.cpu(), p) and torch.equal(ga.cpu(), gio.camera_alpha_mask(p, **kw))


@pytest.mark.parametrize("white", [False, True])
def test_composite_over_every_pair_and_through_every_pass(hip, white):
    c, a = np.meshgrid(np.arange(256), np.arange(256))
    rgba = np.stack([c, (c + 85) & 255, 255 - c, a], axis=2).astype(np.uint8)
    flags = COMPOSITE | (WHITE if white else 0)
    want = imageio.composite_u8_numpy(rgba, white)
    assert np.array_equal(planes_of(want).numpy(), gio.composite_rgba(rgba, white))
    src = torch.from_numpy(rgba).to(DEV)
    rc, got, image, alpha, intact, _ = raw_ingest(hip, src, 256, 256, flags=flags)
    assert rc == 0 and intact and torch.equal(got.cpu(), torch.from_numpy(want)), "the composite's bytes"
    assert torch.equal(image.cpu(), planes_of(want)) and torch.equal(alpha.cpu(), torch.ones(1, 256, 256))
    noisy = cases.seeded(53, 37, 4, 77)
    nsrc = torch.from_numpy(noisy).to(DEV)
    for H2, W2 in ((26, 19), (53, 19), (26, 37), (80, 50)):   # both passes, either one, up
        hi, ha = imageio.ingest_image(noisy, (W2, H2), white_background=white)
        rc, got, image, alpha, intact, _ = raw_ingest(hip, nsrc, H2, W2, flags=flags)
        assert rc == 0 and intact and np.array_equal(image.cpu().numpy(), hi) and np.array_equal(alpha.cpu().numpy(), ha)
        assert torch.equal(got.cpu(), torch.from_numpy(imageio.resize_u8_numpy(imageio.composite_u8_numpy(noisy, white), (W2, H2))))
        gi, ga = imageio.ingest_image(nsrc, (W2, H2), white_background=white)
        assert np.array_equal(gi.cpu().numpy(), hi) and np.array_equal(ga.cpu().numpy(), ha)
    rgb = np.ascontiguousarray(noisy[:, :, :3])   # an RGB file of a NeRF-synthetic scene: alpha 255
    gi, _ = imageio.ingest_image(torch.from_numpy(rgb).to(DEV), (19, 26), white_background=white)
    assert np.array_equal(gi.cpu().numpy(), imageio.ingest_image(rgb, (19, 26), white_background=white)[0])


def test_from_an_unaligned_source(hip):
    """Word loads only when the pixels are word-aligned: a source 1 byte off, for RGBA (both passes, each alone) and LA"""
    for C in (4, 2):
        for (H, W), (H2, W2) in (((37, 26), (9, 8)), ((37, 26), (9, 26)), ((37, 26), (37, 8)), ((37, 26), (37, 26))):
            a = cases.seeded(H, W, C, 900 + C)
            buf = torch.zeros(H * W * C + 8, dtype=torch.uint8, device=DEV)
            src = buf[1:1 + H * W * C].reshape(H, W, C)
            src.copy_(torch.from_numpy(a))
            assert src.data_ptr() % 4 == 1
            rc, got, _, _, intact, _ = raw_ingest(hip, src, H2, W2, planes=False)
            assert rc == 0 and intact and torch.equal(got.cpu(), torch.from_numpy(imageio.resize_alpha_u8_numpy(a, (W2, H2)))), (C, H2, W2)


def test_status_codes(hip):
    src = torch.from_numpy(cases.seeded(37, 64, 4, 1)).to(DEV)
    nb = int(hip.api.raw("image_ingest_tmp_bytes")(37, 64, 4, 9, 16, 0))
    assert 37 * 16 * 4 <= nb < 37 * 16 * 4 + 256
    assert int(hip.api.raw("image_ingest_tmp_bytes")(37, 64, 4, 9, 16, COMPOSITE)) < nb, "the intermediate of a composite is RGB"
    assert int(hip.api.raw("image_ingest_tmp_bytes")(37, 64, 4, 37, 16, 0)) == 0
    for override in (dict(inp=None), dict(out=None, image=None, alpha=None), dict(xb=None), dict(xc=None), dict(yb=None),
                     dict(yc=None), dict(tmp=None)):
        rc, _, _, _, _, untouched = raw_ingest(hip, src, 9, 16, override=override)
        assert rc == E_NULL and untouched, override
    for override in (dict(C=1), dict(C=5), dict(C=0), dict(H=0), dict(W=-1), dict(H2=0), dict(W2=0), dict(kx=0), dict(ky=-3),
                     dict(tmp_bytes=nb - 1), dict(tmp_bytes=0), dict(flags=16), dict(flags=WHITE), dict(C=3, flags=COMPOSITE),
                     dict(C=2), dict(C=2, image=None), dict(C=2, alpha=None)):
        rc, _, _, _, _, untouched = raw_ingest(hip, src, 9, 16, override=override)
        assert rc == E_SHAPE and untouched, override
    # a skipped pass needs neither its tables nor scratch; each output is optional on its own
    rc, got, _, _, intact, _ = raw_ingest(hip, src, 37, 16, planes=False, override=dict(yb=None, yc=None, tmp=None, tmp_bytes=0))
    want = imageio.resize_alpha_u8_numpy(src.cpu().numpy(), (16, 37))
    assert rc == 0 and intact and torch.equal(got.cpu(), torch.from_numpy(want))
    rc, _, image, alpha, intact, _ = raw_ingest(hip, src, 9, 16, u8=False, override=dict(image=None))
    assert rc == 0 and intact and bool((image == -7.0).all())
    assert torch.equal(alpha.cpu(), planes_of(imageio.resize_alpha_u8_numpy(src.cpu().numpy(), (16, 9)))[3:4])
    with pytest.raises(ValueError, match="premultiplies"):
        imageio.resize_u8(src, (2, 2))


def test_a_table_that_leaves_the_source_reads_nothing(hip):
    """Runs that leave the source axis give 0 for their samples and touch nothing else (the kernels check each run)"""
    a = cases.seeded(13, 29, 4, 3)
    a[:, :, 3] = 255   # (opaque: premultiply and un-premultiply are the identity, so a zeroed pixel is 0, 0, 0, 0)
    src = torch.from_numpy(a).to(DEV)
    want = torch.from_numpy(imageio.resize_alpha_u8_numpy(a, (7, 13)))
    want[:, 2] = 0
    want[:, 4] = 0
    xb, xc = (t.clone() for t in imageio._tables_on(DEV, 29, 7))
    xb[2, 0] = 29                # starts beyond the row
    xb[4, 1] = xc.shape[1] + 1   # longer than the table row
    rc, got, _, _, intact, _ = raw_ingest(hip, src, 13, 7, planes=False, override=dict(xb=xb.data_ptr(), xc=xc.data_ptr()))
    assert rc == 0 and intact and torch.equal(got.cpu(), want)
    yb, yc = (t.clone() for t in imageio._tables_on(DEV, 13, 5))
    yb[1, 0] = -1
    yb[3, 0] = 12                # its run would end beyond the last row
    want = torch.from_numpy(imageio.resize_alpha_u8_numpy(a, (29, 5)))
    want[1] = 0
    want[3] = 0
    rc, got, _, _, intact, _ = raw_ingest(hip, src, 5, 29, planes=False, override=dict(yb=yb.data_ptr(), yc=yc.data_ptr()))
    assert rc == 0 and intact and torch.equal(got.cpu(), want)

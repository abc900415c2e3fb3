"""read_png16 / write_png16 (gsplat_amd/imageio.py) against tests/golden/png16/ - files written by Pillow, or built with every
row forced to one filter type, and what Pillow decoded from each (tests/golden/make_golden_png16.py; no Pillow needed here).

Pillow decodes 16-bit grey files to uint16: those must be equal.  A 16-bit RGB file it reduces to the high byte of every sample:
read_png16 >> 8 must be that, and read_png16 itself the uint16 samples the file was built from (decoded.npz's <name>_src)."""
import os
import struct
import zlib

import numpy as np
import pytest

from gsplat_amd import imageio

WHERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png16")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(WHERE, "decoded.npz"))


@pytest.mark.parametrize("name", ["pil_1x1.png", "pil_5x6.png", "pil_1x7.png", "pil_13x9_wide.png"])
def test_pillow_written_grey_files_decode_to_pillows_array(z, name):
    got = imageio.read_png16(os.path.join(WHERE, name))
    assert got.dtype == np.uint16 and got.ndim == 2
    assert np.array_equal(got, z[name])
    if name == "pil_13x9_wide.png":
        assert got.shape == (13, 9) and (got >= 256).all() and ((got & 255) != 0).all()


@pytest.mark.parametrize("ft", range(5))
def test_every_row_filter_at_16_bits_grey(z, ft):
    name = "f%d_L.png" % ft
    raw = zlib.decompress(imageio._png_parse(os.path.join(WHERE, name), "test")[1])
    assert set(raw[::1 + 6 * 2]) == {ft}, "the file's rows carry filter type %d" % ft
    got = imageio.read_png16(os.path.join(WHERE, name))
    assert got.dtype == np.uint16 and got.shape == (7, 6)
    assert np.array_equal(got, z[name])


@pytest.mark.parametrize("ft", range(5))
def test_every_row_filter_at_16_bits_rgb(z, ft):
    name = "f%d_RGB.png" % ft
    got = imageio.read_png16(os.path.join(WHERE, name))
    assert got.dtype == np.uint16 and got.shape == (7, 6, 3)
    assert z[name].dtype == np.uint8 and np.array_equal((got >> 8).astype(np.uint8), z[name])   # Pillow's high bytes
    assert np.array_equal(got, z[name + "_src"])


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (4, 3, 1), (2, 3, 2), (5, 4, 3), (3, 2, 4)])
def test_write_then_read_round_trips(tmp_path, shape):
    rng = np.random.default_rng(len(shape) * 100 + shape[0])
    a = rng.integers(0, 65536, size=shape).astype(np.uint16)
    a.flat[0], a.flat[-1] = 0x0102, 0xFFFE          # (both bytes distinct: the byte order shows)
    path = str(tmp_path / "a.png")
    imageio.write_png16(path, a)
    got = imageio.read_png16(path)
    want = a[:, :, 0] if (a.ndim == 3 and a.shape[2] == 1) else a     # one channel comes back [H,W]
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    with open(path, "rb") as fp:
        head = fp.read(33)
    assert struct.unpack(">IIBBBBB", head[16:29])[2] == 16
    with pytest.raises(ValueError, match="8-bit files only"):       # read_png keeps refusing it
        imageio.read_png(path)
    with pytest.raises(ValueError, match="uint16 only"):
        imageio.write_png16(path, a.astype(np.uint8))


def test_an_8_bit_file_keeps_its_byte_values(z, tmp_path):
    got = imageio.read_png16(os.path.join(WHERE, "grey8.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, z["grey8.png"].astype(np.uint16)) and int(got.max()) <= 255
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    imageio.write_png(str(tmp_path / "c.png"), rgb)
    got = imageio.read_png16(str(tmp_path / "c.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, rgb.astype(np.uint16))


def test_palette_interlaced_and_low_bit_depths_are_refused(tmp_path):
    with pytest.raises(ValueError, match="palette"):
        imageio.read_png16(os.path.join(WHERE, "refuse_palette.png"))
    a = np.arange(12, dtype=np.uint16).reshape(3, 4)
    data = imageio.png16_bytes(a)
    ihdr = bytearray(data[16:29])

    def with_header(h):
        body = bytes(h)
        return data[:12] + b"IHDR" + body + struct.pack(">I", zlib.crc32(b"IHDR" + body) & 0xFFFFFFFF) + data[33:]

    ihdr[12] = 1
    (tmp_path / "i.png").write_bytes(with_header(ihdr))
    with pytest.raises(ValueError, match="interlaced"):
        imageio.read_png16(str(tmp_path / "i.png"))
    ihdr[12], ihdr[8] = 0, 4
    (tmp_path / "b.png").write_bytes(with_header(ihdr))
    with pytest.raises(ValueError, match="bits per sample"):
        imageio.read_png16(str(tmp_path / "b.png"))
    (tmp_path / "n.png").write_bytes(b"not a png")
    with pytest.raises(ValueError, match="not a PNG"):
        imageio.read_png16(str(tmp_path / "n.png"))

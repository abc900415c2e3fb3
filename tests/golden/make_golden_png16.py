"""Generator of tests/golden/png16/ (run by hand where Pillow is installed; the tests only read what it wrote).

Files of at most 13 x 9 pixels and png16/decoded.npz with what Pillow decodes from each:
  pil_1x1.png, pil_5x6.png, pil_1x7.png   16-bit grey, written by Pillow (height x width; its adaptive row filter)
  pil_13x9_wide.png                       16-bit grey, 13 rows x 9 columns, every sample >= 256 with a non-zero low byte: a
                                          reader that swaps or drops a byte cannot pass
  f<t>_L.png, f<t>_RGB.png                every row forced to filter type t = 0..4 at 16 bits - Pillow's writer has no such
                                          switch, so the rows are filtered here as the PNG specification defines them, on BYTES,
                                          the "left" byte one whole pixel (2 C bytes) back - then decoded by Pillow
  grey8.png                               8-bit grey, written by Pillow: read_png16 returns its bytes' values as uint16
  refuse_palette.png                      written by Pillow (the interlaced file is made in the test)
decoded.npz holds per file <name> = Pillow's array.  Pillow decodes 16-bit grey to uint16 ("I;16").  A 16-bit RGB file it
reduces to 8 bits per sample, the HIGH byte of each: for those files <name> is that uint8 array and <name>_src the uint16
samples the file was built from; this script asserts the one is the other's high byte, and a wrong "left" distance corrupts
high bytes as it does low ones.
"""
import os
import struct
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
COLOUR_TYPE = {1: 0, 3: 2}


def filtered_rows16(a, ft):
    """The rows of a uint16 [H,W,C] image under filter type ft, each with its type byte; bpp = 2 C"""
    H, W, C = a.shape
    bpp = 2 * C
    rows = np.ascontiguousarray(a.astype(">u2")).view(np.uint8).reshape(H, W * bpp).astype(np.int64)
    left = np.zeros_like(rows)
    left[:, bpp:] = rows[:, :-bpp]
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    ul = np.zeros_like(rows)
    ul[1:, bpp:] = rows[:-1, :-bpp]
    if ft == 0:
        pred = np.zeros_like(rows)
    elif ft == 1:
        pred = left
    elif ft == 2:
        pred = up
    elif ft == 3:
        pred = (left + up) // 2
    else:
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    body = ((rows - pred) & 255).astype(np.uint8)
    return b"".join(bytes([ft]) + body[y].tobytes() for y in range(H))


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def main():
    where = os.path.join(HERE, "png16")
    os.makedirs(where, exist_ok=True)
    rng = np.random.default_rng(16)
    decoded = {}

    def pillow(name):
        return np.asarray(Image.open(os.path.join(where, name)))

    for H, W in ((1, 1), (5, 6), (1, 7)):
        y, x = np.mgrid[0:H, 0:W]
        a = ((2100 * x + 777 * y + rng.integers(0, 300, size=(H, W))) & 65535).astype(np.uint16)
        name = "pil_%dx%d.png" % (H, W)
        Image.fromarray(a).save(os.path.join(where, name))
        decoded[name] = pillow(name)
        assert decoded[name].dtype == np.uint16 and np.array_equal(decoded[name], a), name
    a = (rng.integers(1, 256, size=(13, 9)) * 256 + rng.integers(1, 256, size=(13, 9))).astype(np.uint16)
    assert (a >= 256).all() and ((a & 255) != 0).all()
    Image.fromarray(a).save(os.path.join(where, "pil_13x9_wide.png"))
    decoded["pil_13x9_wide.png"] = pillow("pil_13x9_wide.png")
    assert np.array_equal(decoded["pil_13x9_wide.png"], a)

    for C, mode in ((1, "L"), (3, "RGB")):
        for ft in range(5):
            b = rng.integers(0, 65536, size=(7, 6, C)).astype(np.uint16)
            data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 7, 16, COLOUR_TYPE[C], 0, 0, 0))
                    + chunk(b"IDAT", zlib.compress(filtered_rows16(b, ft), 9)) + chunk(b"IEND", b""))
            name = "f%d_%s.png" % (ft, mode)
            with open(os.path.join(where, name), "wb") as fp:
                fp.write(data)
            got = pillow(name)
            decoded[name] = got
            if got.dtype == np.uint16:
                assert np.array_equal(got.reshape(b.shape), b), name     # Pillow undoes the filter written here
            else:
                assert got.dtype == np.uint8 and np.array_equal(got.reshape(b.shape), (b >> 8).astype(np.uint8)), name
                decoded[name + "_src"] = b

    g = rng.integers(0, 256, size=(4, 5), dtype=np.uint8)
    Image.fromarray(g, "L").save(os.path.join(where, "grey8.png"))
    decoded["grey8.png"] = pillow("grey8.png")
    assert np.array_equal(decoded["grey8.png"], g)
    Image.fromarray(g, "L").convert("P").save(os.path.join(where, "refuse_palette.png"))
    np.savez_compressed(os.path.join(where, "decoded.npz"), **decoded)
    total = sum(os.path.getsize(os.path.join(where, f)) for f in os.listdir(where))
    print("wrote png16/: %d files, %.1f KB; uint8 decodes: %s"
          % (len(os.listdir(where)), total / 1024.0, sorted(k for k, v in decoded.items() if v.dtype == np.uint8)))


if __name__ == "__main__":
    main()

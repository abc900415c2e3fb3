"""Generator of tests/golden/pil_resize_alpha.npz (run by hand where Pillow is installed; the tests only read what it wrote).

Per case of tests/image_ingest_cases.py::fixture_cases (modes LA and RGBA):
  <key>_crc   CRC32 of the input (the tests regenerate the input and check it)
  <key>_out   Pillow's Image.resize((W2, H2)) bytes, [H2,W2,C] - or, for the same-size case, nothing: Pillow returns a copy
              before it converts to the premultiplied mode, which this script asserts, so the expected output is the input
It also asserts, case by case, that gsplat_amd.imageio.resize_alpha_u8_numpy gives Pillow's bytes and that the per-channel
resize WITHOUT the premultiplied rule does not (on the cases whose alpha varies): the rule is what the fixture pins."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import image_ingest_cases as cases  # noqa: E402
from gsplat_amd import imageio  # noqa: E402

MODES = {2: "LA", 4: "RGBA"}


def main():
    out, naive_differs = {}, 0
    for key, make, (H, W), (H2, W2), C in cases.fixture_cases():
        a = make()
        got = np.asarray(Image.fromarray(a, MODES[C]).resize((W2, H2))).reshape(H2, W2, C)
        assert np.array_equal(imageio.resize_alpha_u8_numpy(a, (W2, H2)), got), key
        out[key + "_crc"] = np.array(cases.crc(a), dtype=np.uint32)
        if (H, W) == (H2, W2):
            assert np.array_equal(got, a), key
        else:
            out[key + "_out"] = got
            naive_differs += int((imageio.resize_u8_numpy(a, (W2, H2)) != got).sum() > 0)
    assert naive_differs > 10, "the premultiplied rule is not exercised"
    path = os.path.join(HERE, "pil_resize_alpha.npz")
    np.savez_compressed(path, **out)
    print("wrote pil_resize_alpha.npz: %.1f KB, %d cases, %d of them differ from the per-channel resize"
          % (os.path.getsize(path) / 1024.0, len(out) // 2 + 1, naive_differs))


if __name__ == "__main__":
    main()

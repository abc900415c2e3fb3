"""Generator of tests/golden/eval_metrics.npz (run by hand, never by the suite):

    python tests/golden/make_golden_eval.py /path/to/LGDWT-GS/utils/image_utils.py /path/to/gaussian-splatting/utils/loss_utils.py

It loads the reference's own image_utils.py (psnr, mse) and loss_utils.py (ssim, l1_loss) from the given paths and EXECUTES
them on the CPU, in float32 as the evaluation scripts do, on seeded image pairs (tests/eval_reference.py: seeded_pair,
seeded_mask - the file keeps the seeds and a checksum of what they gave, not the images).  The pixel transforms in front of
them are the stated ones (clamp; save_image's byte and to_tensor's division; metrics_dtu.py's blend and `mask == 1.`
selection, with the grey mask repeated over three channels as that script reads it).  Only numbers are kept: per case the
reference's float32 mse / psnr / ssim / l1 / count, the float64 restatement's, and the distance between the two - the
margin the GPU test adds to its own bars when it compares against the reference's values."""
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_reference as restatement  # noqa: E402

# key: (H, W, seed, spread beyond [0,1], clamp, quantise, masked)
CASES = {
    "plain_37x53": (37, 53, 21, 0.0, False, False, False),
    "quantise_37x53": (37, 53, 21, 0.0, False, True, False),
    "clamp_64x96": (64, 96, 22, 0.25, True, False, False),
    "clamp_quantise_64x96": (64, 96, 22, 0.25, True, True, False),
    "mask_quantise_64x96": (64, 96, 23, 0.0, False, True, True),
    "mask_clamp_quantise_37x53": (37, 53, 24, 0.25, True, True, True),
}
MASK_SEED = 31
METRICS = ("mse", "psnr", "ssim", "l1", "count")


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def png_round_trip_note():
    """The stated quantisation against a real in-memory PNG, as far as this machine's libraries go."""
    x = restatement.seeded_pair(3, 37, 53, 21, 0.25)[0]
    q = restatement.to_bytes(x)
    try:
        from PIL import Image
    except ImportError:
        return "PIL not importable: the quantisation formula was not checked against a PNG round trip"
    buf = io.BytesIO()
    Image.fromarray(q.permute(1, 2, 0).numpy()).save(buf, format="PNG")
    back = torch.from_numpy(np.array(Image.open(io.BytesIO(buf.getvalue())))).permute(2, 0, 1)
    assert torch.equal(back, q)
    assert torch.equal(back.float().div(255), restatement.transform(x, quantise=True))
    try:
        import torchvision  # noqa: F401
    except ImportError:
        return ("torchvision not importable: save_image / to_tensor themselves were not run; the bytes of the stated formula "
                "survive a PIL in-memory PNG round trip unchanged and their float32 / 255 equals the restatement's")
    import torchvision.transforms.functional as tf
    from torchvision.utils import save_image
    buf = io.BytesIO()
    save_image(x, buf, format="png")
    assert torch.equal(tf.to_tensor(Image.open(io.BytesIO(buf.getvalue()))), restatement.transform(x, quantise=True))
    return "quantisation formula checked against torchvision save_image -> PIL PNG -> to_tensor: identical"


def main():
    iu, lu = load(sys.argv[1], "ref_image_utils"), load(sys.argv[2], "ref_loss_utils")
    out, cases = {}, []
    for key, (H, W, seed, spread, clamp, quantise, masked) in CASES.items():
        render, gt = restatement.seeded_pair(3, H, W, seed, spread)
        mask = restatement.seeded_mask(H, W, MASK_SEED) if masked else None
        r = restatement.transform(render, None, clamp, quantise)[None]
        g = restatement.transform(gt, None, clamp, quantise)[None]
        if masked:
            m3 = mask[None, None].repeat(1, 3, 1, 1)
            mask_bin = (m3 == 1.)
            r = r * m3 + (1 - m3)
            g = g * m3 + (1 - m3)
            ra, ga = r[mask_bin][None, ...], g[mask_bin][None, ...]
            count = float(mask_bin.sum())
        else:
            ra, ga, count = r, g, float(r.numel())
        ref = {"mse": float(iu.mse(ra, ga)), "psnr": float(iu.psnr(ra, ga)), "ssim": float(lu.ssim(r, g)),
               "l1": float(lu.l1_loss(r, g)), "count": count}
        mine = restatement.metrics(render, gt, mask, clamp, quantise)
        out[key + "_ref"] = np.array([ref[k] for k in METRICS], dtype=np.float64)
        out[key + "_f64"] = np.array([mine[k] for k in METRICS], dtype=np.float64)
        out[key + "_dist"] = np.abs(out[key + "_ref"] - out[key + "_f64"])
        out[key + "_checksum"] = np.array([float(render.double().sum()), float(gt.double().sum()),
                                           float(mask.double().sum()) if masked else 0.0])
        cases.append({"key": key, "H": H, "W": W, "seed": seed, "spread": spread, "clamp": clamp, "quantise": quantise,
                      "masked": masked, "mask_seed": MASK_SEED})
        print(key, "ref", out[key + "_ref"], "dist", out[key + "_dist"])
    out["cases"] = np.array(json.dumps(cases))
    out["metrics"] = np.array(json.dumps(METRICS))
    out["notes"] = np.array(png_round_trip_note())
    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(str(out["notes"]))
    print("wrote %s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()

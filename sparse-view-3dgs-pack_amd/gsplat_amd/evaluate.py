"""Test-set evaluation over libgsplat_hip.so (csrc/gs_eval.hip): PSNR, SSIM and L1 of a render against its ground truth
from one pass over the two images, in the forms the reference's evaluation computes them.

  metrics.py (render.py's PNGs read back)     image_metrics(render, gt, quantise=True)          LGDWT-GS/metrics.py:31-32,70-83
  training_report (clamped tensors)           image_metrics(render, gt, clamp=True)             DNGaussian/train_llff.py:298-302
  metrics_dtu.py (white outside the mask)     image_metrics(render, gt, mask=m, quantise=True)  DNGaussian/metrics_dtu.py:40-46,93-95

The pixel transform runs in this order on both images: clamp to [0, 1], the 8-bit round trip of torchvision's save_image /
to_tensor, the blend to white under the mask.  Divergences from the reference, all raised or documented: one view per call
(the reference-named psnr / ssim loop over a batch), fp32 CUDA(HIP) tensors only, at most 4 channels, the DTU mask is ONE
[H,W] plane broadcast over the channels (the reference's is a 3-channel image; DTU's masks are grey).  The gaps this list
used to name are closed beside this file: LPIPS (on request, below), Image.resize and the PNG files in gsplat_amd/imageio.py, the evaluation from
those files in gsplat_amd/render_set.py (evaluate_dir resizes to the mask's size as metrics_dtu.py:37-39 does; the functions
HERE still take images that already have the mask's size), and SSIM_sk here, on request:

  ssim_sk=True    skimage.metrics.structural_similarity(channel_axis=2, data_range=1.0) of the transformed pair
                  (DNGaussian/metrics.py:81, metrics_dtu.py:94), csrc/gs_eval_files.hip: word 5 of a view's row, "ssim_sk" of
                  image_metrics, "SSIM_sk" (the mean only, metrics.py:93-99) of Evaluator.result().  float64 throughout, where
                  skimage runs float32 on the reference's arrays: 2e-10 to 8e-7 apart on the tests' cases.  skimage is not a dependency and the
                  definition is taken from its documented algorithm.  Images below 7 x 7 raise.
  lpips=weights   lpips(render, gt, net_type='vgg') of the transformed pair (metrics.py:74,85, metrics_dtu.py:98),
                  csrc/gs_lpips.hip through gsplat_amd/lpips.py: word 6 of a view's row, "lpips" of image_metrics, "LPIPS" of
                  Evaluator.result() (the mean and the per-view entry, metrics.py:83-86).  `weights` is a
                  lpips.LpipsWeights from the user's two files; nothing is fetched.  Images below 16 x 16 or of fewer than
                  three channels raise.

Nothing here synchronises with the host: a view's numbers are float64 words in device memory, and Evaluator.result() is the
one read-back of a whole test set."""

import torch

from ._lib import hip_api, stream_of
from .io import write_results_json  # noqa: F401  (the evaluation's files: results.json, per_view.json)

CLAMP, QUANTISE, MASK_DTU = 1, 2, 4  # GS_EVAL_CLAMP, GS_EVAL_QUANTISE, GS_EVAL_MASK_DTU
WORDS = 8                            # GS_EVAL_WORDS: mse, psnr, ssim, l1, count, 3 reserved
C1, C2 = 0.01 ** 2, 0.03 ** 2        # utils/loss_utils.py (_ssim)
_MSE, _PSNR, _SSIM, _L1, _COUNT, _SSIM_SK, _LPIPS = range(7)   # (words 5 and 6 are reserved = 0 unless ssim_sk / lpips are asked for)
SK_WIN = 7                           # skimage's default win_size: smaller images raise there


def _image(t, what):
    """[C,H,W] or [1,C,H,W] -> contiguous [C,H,W]"""
    if not torch.is_tensor(t):
        raise ValueError("%s: expected a tensor, got %s" % (what, type(t).__name__))
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError("%s: batch 1 only (got batch %d) - call it once per view" % (what, t.shape[0]))
        t = t[0]
    if t.dim() != 3:
        raise ValueError("%s: expected a [C,H,W] or [1,C,H,W] image, got shape %s" % (what, tuple(t.shape)))
    if not t.is_cuda:
        raise ValueError("%s: CUDA(HIP) tensors only - there is no CPU path" % what)
    if t.dtype != torch.float32:
        raise ValueError("%s: fp32 only (got %s)" % (what, t.dtype))
    return t.contiguous()


def _check(render, gt, mask):
    render, gt = _image(render, "render"), _image(gt, "gt")
    if render.shape != gt.shape:
        raise ValueError("render %s and gt %s differ in shape" % (tuple(render.shape), tuple(gt.shape)))
    if gt.device != render.device:
        raise ValueError("render and gt live on different devices")
    Cn, H, W = (int(x) for x in render.shape)
    if Cn > 4 or min(Cn, H, W) < 1:
        raise ValueError("1 to 4 channels of at least one pixel (got %s)" % (tuple(render.shape),))
    if mask is not None:
        if not torch.is_tensor(mask) or not mask.is_cuda or mask.dtype != torch.float32 or mask.device != render.device:
            raise ValueError("mask: an fp32 CUDA(HIP) tensor on the images' device")
        if mask.numel() != H * W or tuple(mask.shape[-2:]) != (H, W):
            raise ValueError("mask: one [H,W] plane of the images' size (got %s for %dx%d)" % (tuple(mask.shape), H, W))
        mask = mask.reshape(H, W).contiguous()
    return render, gt, mask, Cn, H, W


def _flags(mask, clamp, quantise):
    return (CLAMP if clamp else 0) | (QUANTISE if quantise else 0) | (MASK_DTU if mask is not None else 0)


def _launch(render, gt, mask, Cn, H, W, flags, tmp, row, quantised):
    hip_api().call("eval_metrics", render.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), Cn, H, W,
                   int(flags), C1, C2, tmp.data_ptr(), tmp.numel(), row.data_ptr(),
                   None if quantised is None else quantised.data_ptr(), stream_of(render))


def _tmp(device, Cn, H, W):
    return torch.empty((int(hip_api().raw("eval_tmp_bytes")(Cn, H, W)),), dtype=torch.uint8, device=device)


def _sk_check(H, W):
    if H < SK_WIN or W < SK_WIN:
        raise ValueError("ssim_sk: images of at least %d x %d (got %d x %d) - skimage raises there too" % (SK_WIN, SK_WIN, H, W))


def _sk_tmp(device, Cn, H, W):
    return torch.empty((int(hip_api().raw("eval_ssim_sk_tmp_bytes")(Cn, H, W)),), dtype=torch.uint8, device=device)


def _launch_sk(render, gt, mask, Cn, H, W, flags, tmp, out):
    """out (one float64 word in device memory) <- SSIM_sk of the transformed pair; on the stream of _launch, after it"""
    hip_api().call("eval_ssim_sk", render.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), Cn, H, W,
                   int(flags), tmp.data_ptr(), tmp.numel(), out.data_ptr(), stream_of(render))


def _launch_lpips(render, gt, mask, Cn, H, W, flags, weights, tmp, taps, word):
    """word (one float64 word of a row) <- LPIPS of the transformed pair; taps: six float64 words of device scratch (the five
    per-tap terms and their sum, copied into `word` on the device)"""
    from . import lpips as _lpips
    _lpips.launch(render, gt, mask, Cn, H, W, flags, weights, tmp, taps)
    word.copy_(taps[5:6])


def _lpips_setup(weights, Cn, H, W, device):
    from . import lpips as _lpips
    if not isinstance(weights, _lpips.LpipsWeights):
        raise ValueError("lpips: LpipsWeights (gsplat_amd.lpips) expected, got %s" % type(weights).__name__)
    _lpips.check_size(Cn, H, W)
    return torch.empty((_lpips.tmp_bytes(H, W),), dtype=torch.uint8, device=device)


def image_metrics(render, gt, mask=None, clamp=False, quantise=False, return_bytes=False, ssim_sk=False, lpips=None):
    """-> {"mse", "psnr", "ssim", "l1", "count"}: 0-d float64 device tensors (views of one row), plus "bytes" - the uint8
    [H,W,C] image torchvision's save_image would write for `render` - when return_bytes, plus "ssim_sk" (skimage's
    structural_similarity of the same transformed pair) when ssim_sk, plus "lpips" (LPIPS-VGG of the same transformed pair,
    the bits of lpips.lpips_vgg) when lpips = the LpipsWeights.  Identical images give psnr = +inf; an empty mask gives
    mse = psnr = NaN, as in the reference."""
    render, gt, mask, Cn, H, W = _check(render, gt, mask)
    if ssim_sk:
        _sk_check(H, W)
    dev = render.device
    lp_tmp = _lpips_setup(lpips, Cn, H, W, dev) if lpips is not None else None
    row = torch.empty((WORDS,), dtype=torch.float64, device=dev)
    q = torch.empty((H, W, Cn), dtype=torch.uint8, device=dev) if return_bytes else None
    _launch(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), _tmp(dev, Cn, H, W), row, q)
    out = {"mse": row[_MSE], "psnr": row[_PSNR], "ssim": row[_SSIM], "l1": row[_L1], "count": row[_COUNT]}
    if ssim_sk:
        _launch_sk(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), _sk_tmp(dev, Cn, H, W), row[_SSIM_SK:_SSIM_SK + 1])
        out["ssim_sk"] = row[_SSIM_SK]
    if lpips is not None:
        _launch_lpips(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), lpips, lp_tmp,
                      torch.empty((6,), dtype=torch.float64, device=dev), row[_LPIPS:_LPIPS + 1])
        out["lpips"] = row[_LPIPS]
    if return_bytes:
        out["bytes"] = q
    return out


def _views(img1, img2):
    if img1.dim() == 3:
        img1, img2 = img1[None], img2[None]
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError("expected two [B,C,H,W] (or [C,H,W]) images of one shape, got %s and %s"
                         % (tuple(img1.shape), tuple(img2.shape)))
    return img1, img2


def psnr(img1, img2):
    """utils/image_utils.py:17-19: [B,1] (float32, as the reference's), one kernel pass per view."""
    img1, img2 = _views(img1, img2)
    return torch.stack([image_metrics(a, b)["psnr"] for a, b in zip(img1, img2)]).to(torch.float32)[:, None]


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py ssim with its defaults: a scalar (float32), the mean over the whole batch.  No gradient: this is
    the evaluation's SSIM (the training loss is fused_ssim / lgdwt_loss)."""
    if window_size != 11 or not size_average:
        raise ValueError("ssim: window_size 11 and size_average=True only")
    img1, img2 = _views(img1, img2)
    return torch.stack([image_metrics(a, b)["ssim"] for a, b in zip(img1, img2)]).mean().to(torch.float32)


class Evaluator:
    """The [n_views, 8] float64 device table of a test set and the scratch of its one image size.  add() writes a row with two
    launches (four with ssim_sk, which fills word 5 of the row; with lpips = the LpipsWeights the LPIPS launches follow and
    fill word 6) and no host wait; result() is the one read-back."""
    FILL = float("nan")   # rows no view was added to
    ssim_sk = False       # (a table filled by hand, as the tests do, reports what the defaults report)
    lpips = None

    def __init__(self, n_views, C, H, W, device, ssim_sk=False, lpips=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("Evaluator: CUDA(HIP) device only - there is no CPU path")
        if n_views < 1 or not 1 <= C <= 4 or H < 1 or W < 1:
            raise ValueError("Evaluator: n_views >= 1, 1..4 channels, H, W >= 1 (got %r)" % ((n_views, C, H, W),))
        self.shape = (int(C), int(H), int(W))
        self.table = torch.full((int(n_views), WORDS), self.FILL, dtype=torch.float64, device=device)
        self.tmp = _tmp(device, *self.shape)   # (views are added on one stream: the launches of two views never overlap)
        self.ssim_sk = bool(ssim_sk)
        if self.ssim_sk:
            _sk_check(int(H), int(W))
            self.sk_tmp = _sk_tmp(device, *self.shape)
        self.lpips = lpips
        if lpips is not None:
            self.lp_tmp = _lpips_setup(lpips, int(C), int(H), int(W), device)
            self.lp_taps = torch.full((int(n_views), 6), self.FILL, dtype=torch.float64, device=device)   # per-tap terms, sum

    def add(self, i, render, gt, mask=None, clamp=False, quantise=False):
        """Row i <- the metrics of this view."""
        if not 0 <= int(i) < self.table.shape[0]:
            raise ValueError("Evaluator.add: view %d outside 0..%d" % (i, self.table.shape[0] - 1))
        render, gt, mask, Cn, H, W = _check(render, gt, mask)
        if (Cn, H, W) != self.shape or render.device != self.table.device:
            raise ValueError("Evaluator.add: view is %s on %s, the table was built for %s on %s"
                             % ((Cn, H, W), render.device, self.shape, self.table.device))
        _launch(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), self.tmp, self.table[int(i)], None)
        if self.ssim_sk:
            _launch_sk(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), self.sk_tmp,
                       self.table[int(i), _SSIM_SK:_SSIM_SK + 1])
        if self.lpips is not None:
            _launch_lpips(render, gt, mask, Cn, H, W, _flags(mask, clamp, quantise), self.lpips, self.lp_tmp,
                          self.lp_taps[int(i)], self.table[int(i), _LPIPS:_LPIPS + 1])

    def result(self, names=None):
        """The one read-back -> {"SSIM", "PSNR", "L1", "per_view": {"SSIM": {name: v}, "PSNR": {...}, "L1": {...}}}.  The means
        are plain means of the per-view values (metrics.py:76-83: torch.tensor(psnrs).mean()).  An Evaluator built with
        ssim_sk adds "SSIM_sk": the mean only, no per-view entry, as DNGaussian/metrics.py:93-99 stores it; one built with lpips
        adds "LPIPS", the mean and the per-view entry (metrics.py:83-86)."""
        table = self.table.cpu()
        n = table.shape[0]
        names = ["%05d.png" % i for i in range(n)] if names is None else list(names)   # render.py:45 names its files so
        if len(names) != n:
            raise ValueError("%d names for %d views" % (len(names), n))
        out, per = {}, {}
        cols = (("SSIM", _SSIM), ("PSNR", _PSNR), ("L1", _L1)) + ((("LPIPS", _LPIPS),) if self.lpips is not None else ())
        for key, col in cols:
            vals = [float(v) for v in table[:, col]]
            out[key] = sum(vals) / n
            per[key] = dict(zip(names, vals))
        if self.ssim_sk:
            out["SSIM_sk"] = sum(float(v) for v in table[:, _SSIM_SK]) / n
        out["per_view"] = per
        return out


def evaluate_views(model, cameras, gts, Rasterizer, Settings, bg, names=None, quantise=True, clamp=True, masks=None,
                   camera_keys=None, lpips=None):
    """Render every camera of a test set and score it against its ground truth -> Evaluator.result(names).
    The renders go through trainer.render (the plain forward: no exposure, no clamp - the metric kernel clamps), under
    no_grad.  No metric is read back between views; the rasterizer's own wait for a view's instance count is all the host
    waits for.  camera_keys: one key per camera for the backend's per-camera state (GaussianRasterizer.camera_key; depth
    limits stay off), default ("evaluate", i).  lpips: the LpipsWeights, for the "LPIPS" entries (Evaluator)."""
    from .trainer import render
    if len(cameras) != len(gts) or len(cameras) == 0:
        raise ValueError("evaluate_views: %d cameras and %d ground-truth images" % (len(cameras), len(gts)))
    if masks is not None and len(masks) != len(cameras):
        raise ValueError("evaluate_views: %d masks for %d cameras" % (len(masks), len(cameras)))
    ev = None
    with torch.no_grad():
        for i, (cam, gt) in enumerate(zip(cameras, gts)):
            key = ("evaluate", i) if camera_keys is None else camera_keys[i]
            img = render(cam, model, Rasterizer, Settings, bg, filter_as_indices=None, clamp=False, camera_key=key)["render"]
            if ev is None:
                ev = Evaluator(len(cameras), img.shape[0], img.shape[1], img.shape[2], img.device, lpips=lpips)
            ev.add(i, img, gt, mask=None if masks is None else masks[i], clamp=clamp, quantise=quantise)
    return ev.result(names)

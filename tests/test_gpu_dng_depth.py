"""DNGaussian's depth-normalisation losses on the MI355X (csrc/gs_depth_norm.hip through the dng_loss package) against
the float64 restatement (tests/dng_depth_reference.py).

Per case:
(a) mask: the HIP mask may differ from the float64 mask only where ||d64| - margin| <= tau, tau = 4 x the largest
    |d32 - d64| of the RESTATEMENT run in fp32 and fp64 on that input (never a figure of the code under test); the
    differing share is capped at 1e-4 of the elements, and the same cap is asserted on the restatement's own
    fp32-against-fp64 flips first.
(b) values: loss and input gradient against the float64 restatement with the HIP mask imposed - loss within
    1e-5 max(1, |loss|), gradient within 1e-4 of the tensor's largest entry.  No element is exempt.
(c) two runs give the same bits (loss, mask, gradient).
(d) an incoming dL/dloss scales the gradient: exactly for a power of two, within (b)'s bar otherwise.
(e) the fused node: masks identical to the separate nodes', gradient = their weighted sum within (b)'s bar.
The measured distances go to profiles/dng_depth_parity.json (or to the file DNG_DEPTH_PARITY_OUT names)."""
import json
import os

import numpy as np
import pytest
import torch

import dng_depth_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"fixture": None, "378x504": (378, 504), "300x400": (300, 400), "400x400": (400, 400), "1080x1920": (1080, 1920)}
PATCHES = (5, 8, 16, 17, 53)
MARGINS = (0.00025, 0.001, 0.01, 0.2)
FORMS = ("mse", "mse_global", "l1", "l1_global")
LOSS_BAR, GRAD_BAR, FLIP_CAP = 1e-5, 1e-4, 1e-4
PARITY = {}
_inputs_cache = {}


def inputs(size):
    """(depth, target) float64 CPU [1,1,H,W], the same numbers as their float32 form."""
    if size not in _inputs_cache:
        if SIZES[size] is None:
            z = np.load(os.path.join(ROOT, "tests", "golden", "dng_depth.npz"))
            _inputs_cache[size] = (torch.from_numpy(z["depth"]).double(), torch.from_numpy(z["mono"]).double())
        else:
            _inputs_cache[size] = ref.scene(*SIZES[size], seed=sum(SIZES[size]))
    return _inputs_cache[size]


def hip_fn(name):
    import dng_loss
    return getattr(dng_loss, "patch_norm_%s" % name.replace("mse", "mse_loss").replace("l1", "l1_loss"))


def run_hip(name, depth, mono, p, margin, upstream=None):
    dev = torch.device("cuda:0")
    x = depth.float().to(dev).requires_grad_(True)
    loss, mask = hip_fn(name)(x, mono.float().to(dev), p, margin, return_mask=True)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(upstream, device=dev))
    return loss.detach().cpu(), mask.cpu(), x.grad.cpu()


def _record(key, **kw):
    PARITY[key] = kw
    try:
        out = os.environ.get("DNG_DEPTH_PARITY_OUT") or os.path.join(ROOT, "profiles", "dng_depth_parity.json")
        json.dump(PARITY, open(out, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _cases():
    out = []
    for i, size in enumerate(SIZES):
        for j, p in enumerate(PATCHES):
            if SIZES[size] is None and p > 64:
                continue
            for k, name in enumerate(FORMS):
                out.append(pytest.param(size, p, name, MARGINS[(i + j + k) % 4],
                                        id="%s-p%d-%s-m%g" % (size, p, name, MARGINS[(i + j + k) % 4])))
    return out


def test_cases_cover_every_margin_with_every_patch_size_and_form():
    seen_p, seen_f = set(), set()
    for c in _cases():
        _, p, name, margin = c.values
        seen_p.add((p, margin))
        seen_f.add((name, margin))
    assert seen_p == {(p, m) for p in PATCHES for m in MARGINS}
    assert seen_f == {(f, m) for f in FORMS for m in MARGINS}


@pytest.mark.parametrize("size,p,name,margin", _cases())
def test_patch_loss_against_the_restatement(hip, size, p, name, margin):
    depth, mono = inputs(size)
    glob, l1 = ref.FORMS[name]
    # the restatement on its own: fp64, and fp32 for what single precision moves
    _, mask64, d64 = ref.patch_norm_loss(depth, mono, p, margin, glob, l1, return_all=True)
    _, mask32, d32 = ref.patch_norm_loss(depth.float(), mono.float(), p, margin, glob, l1, return_all=True)
    n = mask64.numel()
    tau = 4.0 * float((d32.double() - d64).abs().max())
    own_flips = int((mask32 != mask64).sum())
    assert own_flips <= FLIP_CAP * n, "the restatement itself flips %d of %d: not an input of the stated kind" % (own_flips, n)

    loss, mask, grad = run_hip(name, depth, mono, p, margin)
    # (a) the mask
    assert mask.shape == mask64.shape and mask.dtype == torch.bool
    diff = mask != mask64
    band = (d64.abs() - margin).abs() <= tau
    flips = int(diff.sum())
    outside = int((diff & ~band).sum())
    print("mask: %d of %d differ, %d outside the band tau=%.3e (restatement fp32: %d)" % (flips, n, outside, tau, own_flips))
    assert outside == 0
    assert flips <= FLIP_CAP * n
    # (b) values, with the HIP mask imposed
    x = depth.clone().requires_grad_(True)
    want = ref.patch_norm_loss(x, mono, p, margin, glob, l1, mask=mask)
    want.backward()
    want = float(want.detach())
    loss_err = abs(float(loss) - want) / max(1.0, abs(want))
    grad_err = float((grad.double() - x.grad).abs().max()) / float(x.grad.abs().max())
    print("loss %.9g (want %.9g) err %.2e; grad rel err %.2e" % (float(loss), want, loss_err, grad_err))
    _record("%s p=%d %s margin=%g" % (size, p, name, margin), loss_err=loss_err, grad_err=grad_err, mask_flips=flips,
            restatement_fp32_flips=own_flips, tau=tau, elements=n, masked=int(mask.sum()))
    assert loss_err <= LOSS_BAR
    assert grad_err <= GRAD_BAR
    assert grad.shape == depth.shape
    # (c) the same bits twice
    loss2, mask2, grad2 = run_hip(name, depth, mono, p, margin)
    assert torch.equal(loss, loss2) and torch.equal(mask, mask2) and torch.equal(grad, grad2)
    # (d) the incoming gradient
    _, _, quarter = run_hip(name, depth, mono, p, margin, upstream=0.25)
    assert torch.equal(quarter, 0.25 * grad)
    _, _, scaled = run_hip(name, depth, mono, p, margin, upstream=-3.5)
    assert float((scaled.double() + 3.5 * x.grad).abs().max()) <= GRAD_BAR * 3.5 * float(x.grad.abs().max())


def test_empty_mask_is_nan_with_a_zero_gradient(hip):
    depth, mono = inputs("fixture")
    loss, mask, grad = run_hip("mse", depth, mono, 8, 1e9)
    assert bool(torch.isnan(loss)) and not bool(mask.any())
    assert float(grad.abs().max()) == 0.0 and not bool(torch.isnan(grad).any())


def test_patch_sizes_at_the_edges(hip):
    """p = 2, a patch wider than a workgroup, and the one-patch image."""
    depth, mono = inputs("300x400")
    for p in (2, 3, 129, 257, 300):
        x = depth.clone().requires_grad_(True)
        loss, mask, grad = run_hip("mse", depth, mono, p, 0.01)
        want = ref.patch_norm_loss(x, mono, p, 0.01, mask=mask)
        want.backward()
        assert abs(float(loss) - float(want.detach())) <= LOSS_BAR * max(1.0, abs(float(want.detach()))), p
        assert float((grad.double() - x.grad).abs().max()) <= GRAD_BAR * float(x.grad.abs().max()), p
        mask64 = ref.patch_norm_loss(depth, mono, p, 0.01, return_all=True)[1]
        assert int((mask != mask64).sum()) <= FLIP_CAP * mask.numel(), p


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("guide", ["mono", "rgb"])
def test_smoothness_against_the_restatement(hip, size, guide):
    import dng_loss
    dev = torch.device("cuda:0")
    depth, mono = inputs(size)
    if guide == "rgb":
        g = torch.Generator().manual_seed(5)
        img = torch.rand((1, 3) + tuple(depth.shape[2:]), generator=g).double()
    else:
        img = mono
    x = depth.clone().requires_grad_(True)
    want = ref.loss_depth_smoothness(x, img)
    want.backward()
    outs = []
    for _ in range(2):
        xh = depth.float().to(dev).requires_grad_(True)
        loss = dng_loss.loss_depth_smoothness(xh, img.float().to(dev))
        loss.backward()
        outs.append((loss.detach().cpu(), xh.grad.cpu()))
    loss, grad = outs[0]
    loss_err = abs(float(loss) - float(want.detach())) / max(1.0, abs(float(want.detach())))
    grad_err = float((grad.double() - x.grad).abs().max()) / float(x.grad.abs().max())
    print("smoothness %.9g (want %.9g) err %.2e; grad rel err %.2e" % (float(loss), float(want.detach()), loss_err, grad_err))
    _record("%s smoothness %s" % (size, guide), loss_err=loss_err, grad_err=grad_err)
    assert loss_err <= LOSS_BAR and grad_err <= GRAD_BAR
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("p_local,p_global,margin,w_smooth", [(5, 16, 0.01, 0.1), (17, 8, 0.00025, 0.0), (53, 5, 0.2, 0.1),
                                                              (8, 8, 0.001, 0.1)])
def test_fused_node_is_the_sum_of_its_parts(hip, size, p_local, p_global, margin, w_smooth):
    import dng_loss
    dev = torch.device("cuda:0")
    depth, mono = inputs(size)
    t = mono.float().to(dev)
    w_local, w_global = 0.1, 1.0
    # the separate nodes, as a training script calls them: three losses pending, one backward
    xs = depth.float().to(dev).requires_grad_(True)
    l_loc, m_loc = dng_loss.patch_norm_mse_loss(xs, t, p_local, margin, return_mask=True)
    total = w_local * l_loc
    l_s = None
    if w_smooth:
        l_s = dng_loss.loss_depth_smoothness(xs, t)
        total = total + w_smooth * l_s
    l_glob, m_glob = dng_loss.patch_norm_mse_loss_global(xs, t, p_global, margin, return_mask=True)
    total = total + w_global * l_glob
    total.backward()
    # the fused node, twice
    outs = []
    for _ in range(2):
        xf = depth.float().to(dev).requires_grad_(True)
        f_total, parts, f_loc, f_glob = dng_loss.depth_regulariser(xf, t, p_local, p_global, margin, w_local, w_global,
                                                                   w_smooth, return_parts=True)
        f_total.backward()
        outs.append((f_total.detach().cpu(), parts.cpu(), f_loc.cpu(), f_glob.cpu(), xf.grad.cpu()))
    f_total, parts, f_loc, f_glob, f_grad = outs[0]
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.equal(f_loc, m_loc.cpu()) and torch.equal(f_glob, m_glob.cpu())
    assert float(parts[1]) == float(l_loc) and float(parts[2]) == float(l_glob)
    if w_smooth:
        assert float(parts[3]) == float(l_s)
    assert float(parts[0]) == float(f_total)
    assert abs(float(f_total) - float(total)) <= LOSS_BAR * max(1.0, abs(float(total)))
    sep = xs.grad.cpu()
    sum_err = float((f_grad - sep).abs().max()) / float(sep.abs().max())
    # and against the restatement with the HIP masks imposed
    x = depth.clone().requires_grad_(True)
    want = ref.depth_regulariser(x, mono, p_local, p_global, margin, w_local, w_global, w_smooth, mask_local=f_loc,
                                 mask_global=f_glob)
    want.backward()
    loss_err = abs(float(f_total) - float(want.detach())) / max(1.0, abs(float(want.detach())))
    grad_err = float((f_grad.double() - x.grad).abs().max()) / float(x.grad.abs().max())
    print("fused: vs separate nodes %.2e; vs restatement loss %.2e grad %.2e" % (sum_err, loss_err, grad_err))
    _record("%s fused p=(%d,%d) margin=%g w_smooth=%g" % (size, p_local, p_global, margin, w_smooth), loss_err=loss_err,
            grad_err=grad_err, grad_vs_separate_nodes=sum_err)
    assert sum_err <= GRAD_BAR and loss_err <= LOSS_BAR and grad_err <= GRAD_BAR


def test_forward_only_and_three_dim_inputs(hip):
    """No gradient wanted: the loss alone; a [1,H,W] depth (what a renderer returns) gets a [1,H,W] gradient."""
    import dng_loss
    dev = torch.device("cuda:0")
    depth, mono = inputs("fixture")
    x, t = depth.float().to(dev), mono.float().to(dev)
    with torch.no_grad():
        a = dng_loss.patch_norm_l1_loss(x, t, 8, 0.01)
    x3 = x[0].clone().requires_grad_(True)
    b = dng_loss.patch_norm_l1_loss(x3, t[0], 8, 0.01)
    b.backward()
    assert float(a) == float(b) and x3.grad.shape == x3.shape

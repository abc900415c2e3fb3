"""Test oracle: DNGaussian's depth-normalisation losses restated in plain torch, in the dtype of their inputs (the tests
run them in float64, and in float32 to measure what single precision alone moves).  Written from the semantics, not
from the reference's text: patches are cut with reshape / permute, not unfold.

    patches        non-overlapping p x p, stride p, remainder rows / columns dropped, row-major patch order,
                   elements row-major inside a patch: [L, p*p]
    n(x)           (x - patch mean) / (s + 1e-2 std_all); std_all = unbiased std of all L p^2 patch elements (with
                   gradient); s = the patch's unbiased std (with gradient), or in the global form the unbiased std of the
                   whole uncropped image, detached
    d, mask        d = n(input) - n(target), mask = |d| > margin (strict)
    loss           mean over the mask of d^2 (mse) or |d| (l1); NaN on an empty mask, with a zero gradient

Every patch loss takes an optional imposed `mask` ([L, p*p] bool): with one given the threshold is not evaluated and
that mask selects the elements."""
import torch


def patches(x, p):
    """[1,1,H,W] -> [L, p*p]."""
    assert x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 1
    H, W = x.shape[2], x.shape[3]
    ny, nx = H // p, W // p
    v = x[0, 0, :ny * p, :nx * p].reshape(ny, p, nx, p).permute(0, 2, 1, 3)
    return v.reshape(ny * nx, p * p)


def normalised(x, p, global_form, image_std=None):
    """image_std: the global form's detached whole-image std as a given constant (a finite-difference check has to hold it
    fixed, since it is no function of the input as far as the gradient is concerned)."""
    P = patches(x, p)
    mean = P.mean(dim=1, keepdim=True)
    n = P.shape[1]
    if global_form:
        s = x.reshape(-1).std(unbiased=True).detach() if image_std is None else image_std
    else:
        s = ((P - mean) ** 2).sum(dim=1, keepdim=True).div(n - 1).sqrt()
    flat = P.reshape(-1)
    std_all = ((flat - flat.mean()) ** 2).sum().div(flat.numel() - 1).sqrt()
    return (P - mean) / (s + 1e-2 * std_all)


def normalised_difference(input, target, p, global_form, input_std=None):
    return normalised(input, p, global_form, input_std) - normalised(target, p, global_form)


def patch_norm_loss(input, target, p, margin, global_form=False, l1=False, mask=None, return_all=False, input_std=None):
    """-> loss, or (loss, mask, d) with return_all."""
    d = normalised_difference(input, target, p, global_form, input_std)
    if mask is None:
        mask = d.detach().abs() > margin
    sel = d[mask]
    loss = (sel.abs() if l1 else sel ** 2).mean()
    return (loss, mask, d) if return_all else loss


def patch_norm_mse_loss(input, target, patch_size, margin, return_mask=False, mask=None):
    loss, m, _ = patch_norm_loss(input, target, patch_size, margin, False, False, mask, True)
    return (loss, m) if return_mask else loss


def patch_norm_mse_loss_global(input, target, patch_size, margin, return_mask=False, mask=None):
    loss, m, _ = patch_norm_loss(input, target, patch_size, margin, True, False, mask, True)
    return (loss, m) if return_mask else loss


def patch_norm_l1_loss(input, target, patch_size, margin, return_mask=False, mask=None):
    loss, m, _ = patch_norm_loss(input, target, patch_size, margin, False, True, mask, True)
    return (loss, m) if return_mask else loss


def patch_norm_l1_loss_global(input, target, patch_size, margin, return_mask=False, mask=None):
    loss, m, _ = patch_norm_loss(input, target, patch_size, margin, True, True, mask, True)
    return (loss, m) if return_mask else loss


FORMS = {"mse": (False, False), "mse_global": (True, False), "l1": (False, True), "l1_global": (True, True)}


def loss_depth_smoothness(depth, img):
    """Edge-aware first-order smoothness: |dx depth|, |dy depth| weighted by exp(-mean_c |dx img|), over the weights' sum."""
    wx = torch.exp(-(img[..., :, 1:] - img[..., :, :-1]).abs().mean(dim=1, keepdim=True))
    wy = torch.exp(-(img[..., 1:, :] - img[..., :-1, :]).abs().mean(dim=1, keepdim=True))
    gx = (depth[..., :, 1:] - depth[..., :, :-1]).abs()
    gy = (depth[..., 1:, :] - depth[..., :-1, :]).abs()
    return ((gx * wx).sum() + (gy * wy).sum()) / (wx.sum() + wy.sum())


def depth_regulariser(depth, mono, p_local, p_global, margin, w_local=0.1, w_global=1.0, w_smooth=0.0, mask_local=None,
                      mask_global=None):
    """The reference scripts' call: w_local * mse(p_local) + w_smooth * smoothness + w_global * mse_global(p_global)."""
    total = w_local * patch_norm_mse_loss(depth, mono, p_local, margin, mask=mask_local)
    if w_smooth != 0.0:
        total = total + w_smooth * loss_depth_smoothness(depth, mono)
    return total + w_global * patch_norm_mse_loss_global(depth, mono, p_global, margin, mask=mask_global)


def scene(H, W, seed, dtype=torch.float64):
    """A depth / target pair of the kind the losses meet: a smooth field plus a step plus noise; depth around 3 +- 1.5,
    target (255 - mono depth) around 120 +- 60, correlated with the depth but not a function of it."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H, dtype=torch.float64)[:, None]
    x = torch.linspace(0, 1, W, dtype=torch.float64)[None, :]
    ph = torch.rand((4,), generator=g, dtype=torch.float64) * 6.28
    base = (torch.sin(3.1 * x + ph[0]) * torch.cos(2.3 * y + ph[1]) + 0.5 * torch.sin(7.0 * (x + y) + ph[2]))
    step = ((x + 0.5 * y) > 0.8).double()
    other = torch.cos(4.3 * x - 2.9 * y + ph[3])
    depth = 3.0 + 0.8 * base + 0.9 * step + 0.15 * torch.randn((H, W), generator=g, dtype=torch.float64)
    mono = 120.0 + 30.0 * base + 40.0 * step + 14.0 * other + 4.0 * torch.randn((H, W), generator=g, dtype=torch.float64)
    # through float32, so that the fp32 and fp64 runs start from the same numbers
    return depth.float().to(dtype)[None, None], mono.float().to(dtype)[None, None]

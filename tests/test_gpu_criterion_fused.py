"""The LGDWT criterion without its clamped image (gs_lgdwt_fused_fwd) and with its gradient from one kernel (gs_lgdwt_fused_bwd)
against the kernel sequence they replace: sums, SSIM maps, SSIM partials and gradient bit for bit, and the whole FusedLGDWTLoss
either way, to the bit."""
import pytest
import torch

from gsplat_amd import losses
from gsplat_amd.losses import LGDWTCriterion, LossOps

pytestmark = pytest.mark.gpu

C1, C2 = 0.01 ** 2, 0.03 ** 2
SHAPES = [(1080, 1920, 128), (256, 384, 64), (260, 392, 128)]
SWITCHES = [(True, True), (True, False), (False, True), (False, False)]   # (dwt, patch)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _inputs(C, H, W, ps, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand((C, H, W), generator=g)
    raw = gt + 0.2 * torch.randn((C, H, W), generator=g)       # an un-clamped render: values outside [0, 1]
    mask = (torch.rand(((H // ps) * (W // ps),), generator=g) < 0.4).to(torch.uint8)
    mask[0] = 1
    return raw.cuda(), gt.cuda(), mask.cuda()


def _sequence_fwd(api, raw, gt, ps, mask):
    """gs_l1_dwt2_patch_fwd_clamp_p + gs_ssim_fwd_partials, as FusedLGDWTLoss ran them: (img, rows of 12, ssim partials, maps)"""
    C, H, W = raw.shape
    img = torch.empty_like(raw)
    rows = torch.empty((int(api.raw("dwt_partials_count")(C, H, W)) * 12,), device="cuda")
    api.call("l1_dwt2_patch_fwd_clamp_p", raw.data_ptr(), gt.data_ptr(), C, H, W, ps, mask.data_ptr() if ps else None,
             rows.data_ptr(), img.data_ptr(), _st())
    n = int(api.raw("ssim_partials_count")(1, C, H, W))
    part = torch.empty((n,), device="cuda")
    d = [torch.empty_like(raw) for _ in range(3)]
    api.call("ssim_fwd_partials", img.data_ptr(), gt.data_ptr(), 1, C, H, W, C1, C2, part.data_ptr(), *[x.data_ptr() for x in d],
             _st())
    return img, rows, part, d


def _fused_fwd(api, raw, gt, ps, mask):
    C, H, W = raw.shape
    rows = torch.empty((int(api.raw("dwt_partials_count")(C, H, W)) * 12,), device="cuda")
    part = torch.empty((int(api.raw("ssim_partials_count")(1, C, H, W)),), device="cuda")
    d = [torch.empty_like(raw) for _ in range(3)]
    api.call("lgdwt_fused_fwd", raw.data_ptr(), gt.data_ptr(), C, H, W, C1, C2, ps, mask.data_ptr() if ps else None,
             rows.data_ptr(), part.data_ptr(), *[x.data_ptr() for x in d], _st())
    return rows, part, d


@pytest.mark.parametrize("H,W,ps", SHAPES)
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("patch", [True, False])
def test_fused_forward_equals_the_sequence(hip, H, W, ps, C, patch):
    api = hip.api
    raw, gt, mask = _inputs(C, H, W, ps, H + W + C)
    pps = ps if patch else 0
    _, ref_rows, ref_part, ref_d = _sequence_fwd(api, raw, gt, pps, mask)
    rows, part, d = _fused_fwd(api, raw, gt, pps, mask)
    torch.cuda.synchronize()
    assert torch.equal(rows, ref_rows), "rows of 12 sums"
    assert torch.equal(part, ref_part), "SSIM partials"
    for k in range(3):
        assert torch.equal(d[k], ref_d[k]), "derivative map %d" % k
    if patch:
        assert float(ref_rows.view(-1, 12)[:, 9:].sum(0).min()) > 0, "no selected patch contributed"


@pytest.mark.parametrize("H,W,ps", SHAPES)
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("dwt,patch", SWITCHES)
@pytest.mark.parametrize("clamp_mask", [True, False])
def test_fused_backward_equals_the_sequence(hip, H, W, ps, C, dwt, patch, clamp_mask):
    api = hip.api
    raw, gt, mask = _inputs(C, H, W, ps, 7 * H + W + C)
    pps = ps if patch else 0
    img, _, _, d = _sequence_fwd(api, raw, gt, pps, mask)
    g = torch.Generator().manual_seed(H + C)
    coef = (torch.rand((16,), generator=g) / (C * H * W)).cuda()   # out[8..23]: c_l1, c_ssim, c_band x8, c_patch x3
    coef[1] = -coef[1] * 50
    if not dwt:
        coef[2:10] = 0
    st = _st()
    ref = torch.empty_like(raw)
    if patch:
        api.call("l1_dwt2_patch_bwd", img.data_ptr(), gt.data_ptr(), C, H, W, ps, mask.data_ptr(), coef.data_ptr(),
                 coef[2:].data_ptr(), coef[10:].data_ptr(), ref.data_ptr(), 0, st)
    elif dwt:
        api.call("l1_dwt2_bwd", img.data_ptr(), gt.data_ptr(), C, H, W, coef.data_ptr(), coef[2:].data_ptr(), ref.data_ptr(), 0, st)
    else:
        api.call("l1_bwd_dev", img.data_ptr(), gt.data_ptr(), img.numel(), coef.data_ptr(), ref.data_ptr(), 0, st)
    api.call("ssim_bwd_uniform", img.data_ptr(), gt.data_ptr(), 1, C, H, W, coef[1:].data_ptr(), *[x.data_ptr() for x in d],
             ref.data_ptr(), 1, raw.data_ptr() if clamp_mask else None, st)
    out = torch.full_like(raw, float("nan"))       # every pixel must be written
    flags = 1 | (2 if dwt else 0) | (4 if clamp_mask else 0)
    api.call("lgdwt_fused_bwd", raw.data_ptr(), gt.data_ptr(), C, H, W, flags, pps, mask.data_ptr() if patch else None,
             coef.data_ptr(), *[x.data_ptr() for x in d], out.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


class _Spy:
    """The product api with a log of the entry points called through it."""

    def __init__(self, api):
        self._api, self.calls = api, []

    def __getattr__(self, name):
        return getattr(self._api, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._api.call(name, *args)


def _criterion_run(api, raw, gt, dwt, patch, ps, steps=2):
    crit = LGDWTCriterion(LossOps(api), dwt_enable=dwt, patch_dwt_enable=patch, patch_size=ps)
    res = []
    for _ in range(steps):
        r = raw.clone().requires_grad_(True)
        loss, parts = crit.fused_call(r, gt)
        loss.backward()
        res.append((loss.detach().clone(), parts["dwt_scale"].detach().clone(), r.grad.clone()))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("H,W,ps,C", [(1080, 1920, 128, 3), (256, 384, 64, 1), (260, 392, 128, 3)])
@pytest.mark.parametrize("dwt,patch", SWITCHES)
def test_criterion_fused_vs_sequence(hip, monkeypatch, H, W, ps, C, dwt, patch):
    raw, gt, _ = _inputs(C, H, W, ps, 3 * H + C)
    spy = _Spy(hip.api)
    fused = _criterion_run(spy, raw, gt, dwt, patch, ps)
    # the one-kernel gradient everywhere but beside the separate patch kernels (patch term without the DWT term); no clamped
    # image where the sums come from the folded DWT kernel
    assert ("lgdwt_fused_bwd" in spy.calls) == (dwt or not patch)
    assert ("lgdwt_fused_fwd" in spy.calls) == dwt and ("ssim_fwd_partials" in spy.calls) == (not dwt)
    again = _criterion_run(hip.api, raw, gt, dwt, patch, ps)
    monkeypatch.setattr(losses, "FUSED_PASSES", False)
    spy = _Spy(hip.api)
    seq = _criterion_run(spy, raw, gt, dwt, patch, ps)
    assert "lgdwt_fused_fwd" not in spy.calls and "lgdwt_fused_bwd" not in spy.calls and "ssim_fwd_partials" in spy.calls
    for (lf, sf, gf), (la, sa, ga), (ls, ss, gs) in zip(fused, again, seq):
        if patch and not dwt:
            # the sequence's separate patch kernels (gs_patch_dwt_fwd) add their sums with float atomics: equal to rounding only
            for a, b in ((lf, ls), (la, ls), (sf, ss)):
                assert abs(float(a) - float(b)) <= 1e-5 * abs(float(b)), (float(a), float(b))
            for gg in (gf, ga):
                assert float((gg - gs).abs().max()) <= 1e-5 * float(gs.abs().max())
            continue
        assert torch.equal(lf, la) and torch.equal(sf, sa) and torch.equal(gf, ga), "two fused runs differ"
        assert torch.equal(lf, ls) and torch.equal(sf, ss), (float(lf), float(ls), float(sf), float(ss))
        assert torch.equal(gf, gs), float((gf - gs).abs().max())


def test_ineligible_shape_keeps_the_sequence(hip):
    """131 x 260 (H not a multiple of 4) with the DWT term: the old kernels, and the same bits as with the switch off."""
    raw, gt, _ = _inputs(3, 131, 260, 64, 5)
    spy = _Spy(hip.api)
    res = _criterion_run(spy, raw, gt, True, True, 64, steps=1)
    assert "lgdwt_fused_fwd" not in spy.calls and "lgdwt_fused_bwd" not in spy.calls
    assert "ssim_fwd_partials" in spy.calls and "ssim_bwd_uniform" in spy.calls
    assert torch.isfinite(res[0][2]).all()

"""gs_lgdwt_fused_fwd in its one-launch form (lgdwt_fwd_kernel: the DWT / L1 / patch workgroups and the SSIM tiles in one grid)
against the two launches it replaces (GS_LGDWT_FWD_SPLIT=1): rows of 12 sums, SSIM partials and the three derivative maps as
bit patterns, no tolerance - the bodies, the per-workgroup rows and the order of additions are the same by construction.  The
switch is read once per process, so each arm runs in a child process of its own (this file as a program); the stage timers
count the launches: one under ssim_fwd in the default form, one each under dwt2_l1_fwd and ssim_fwd under the escape."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
C1, C2 = 0.01 ** 2, 0.03 ** 2
SIZES = [(1080, 1920, 128), (64, 64, 32), (260, 392, 64)]   # (H, W, patch size where a mask is given)
CASES = [(C, H, W, ps if patch else 0) for H, W, ps in SIZES for C in (1, 3) for patch in (False, True)]
OUTPUTS = ("dwt_partials", "ssim_partials", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")


def _key(C, H, W, ps):
    return "%d-%dx%d-ps%d" % (C, H, W, ps)


def _inputs(C, H, W, ps, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand((C, H, W), generator=g)
    raw = gt + 0.2 * torch.randn((C, H, W), generator=g)       # an un-clamped render: values outside [0, 1]
    mask = None
    if ps:
        mask = (torch.rand(((H // ps) * (W // ps),), generator=g) < 0.4).to(torch.uint8)
        mask[0] = 1
        mask = mask.cuda()
    return raw.cuda(), gt.cuda(), mask


def _nan_filled(n):
    """n floats of a quiet-NaN pattern with a payload: an element the kernels leave alone shows in the comparison"""
    return torch.full((n,), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)


def _child(out_path):
    sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
    from gsplat_amd import hip_backend
    from gsplat_amd.capi import read_profile
    api = hip_backend().api
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for C, H, W, ps in CASES:
        raw, gt, mask = _inputs(C, H, W, ps, 11 * H + W + 5 * C + ps)
        bufs = [_nan_filled(int(api.raw("dwt_partials_count")(C, H, W)) * 12),
                _nan_filled(int(api.raw("ssim_partials_count")(1, C, H, W)))] + [_nan_filled(C * H * W) for _ in range(3)]
        api.call("profile_reset")
        api.call("profile_enable", 1)
        api.call("lgdwt_fused_fwd", raw.data_ptr(), gt.data_ptr(), C, H, W, C1, C2, ps, mask.data_ptr() if ps else None,
                 *[b.data_ptr() for b in bufs], st)
        api.call("profile_enable", 0)
        torch.cuda.synchronize()
        prof = read_profile(api)
        entry = {k: b.view(torch.int32).cpu() for k, b in zip(OUTPUTS, bufs)}
        entry["launches"] = {k: int(v[1]) for k, v in prof.items()}
        res[_key(C, H, W, ps)] = entry
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """{arm: {case: outputs as int32, launches per stage}} from one child process per arm"""
    d = tmp_path_factory.mktemp("one_launch")
    out = {}
    for arm, split in (("one", "0"), ("split", "1")):
        f = str(d / (arm + ".pt"))
        env = dict(os.environ, GS_LGDWT_FWD_SPLIT=split)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), f], env=env, capture_output=True, text=True, cwd=ROOT,
                           timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        out[arm] = torch.load(f)
    return out


@pytest.mark.parametrize("C,H,W,ps", CASES)
def test_one_launch_equals_the_two_launches(arms, C, H, W, ps):
    one, split = arms["one"][_key(C, H, W, ps)], arms["split"][_key(C, H, W, ps)]
    for k in OUTPUTS:
        for name, arm in (("one launch", one), ("two launches", split)):
            assert not torch.isnan(arm[k].view(torch.float32)).any(), "%s: %s has elements nobody wrote" % (name, k)
        assert torch.equal(one[k], split[k]), k
    if ps:
        assert float(one["dwt_partials"].view(torch.float32).view(-1, 12)[:, 9:].sum(0).min()) > 0, "no selected patch contributed"


@pytest.mark.parametrize("C,H,W,ps", CASES)
def test_launch_counts(arms, C, H, W, ps):
    one, split = arms["one"][_key(C, H, W, ps)]["launches"], arms["split"][_key(C, H, W, ps)]["launches"]
    assert one == {"ssim_fwd": 1}, one
    assert split == {"dwt2_l1_fwd": 1, "ssim_fwd": 1}, split


if __name__ == "__main__":
    _child(sys.argv[1])

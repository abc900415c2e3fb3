"""The device form of densify / split / prune, held to the host path on the CPU (no GPU needed).

tests/densify_reference.py restates the device plan in torch: per-SOURCE-row flags from five fp32 thresholds, then the
destination table in reference order.  Here the model that table describes is compared with what
GaussianModelLite.densify_and_prune (host path, the arbiter) builds - which proves that a clone's prune decision is its
source survivor's and that the N samples of a split row share one decision -, the fp32-threshold rule is pinned on the host
path, and every input of tests/test_gpu_densify_device.py is shown to be decisive (margin condition)."""
import os
import re

import pytest
import torch

import densify_reference as dr
from gsplat_amd.trainer import GaussianModelLite, TrainOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("densify_tmp_bytes", "densify_plan", "densify_emit", "morton_codes", "densify_gather")


def plan_of(m, N, screen):
    thr = dr.thresholds(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, m.percent_dense, N)
    flags = dr.plan_flags(m.params["scaling"].detach(), m.params["opacity"].detach(), m.xyz_gradient_accum, m.denom, thr,
                          bool(screen))
    return flags, dr.destination_table(flags, N)


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dr.SIZES)
def test_the_table_applied_to_a_model_is_the_host_path(oracle, P, with_nir):
    seen = set()
    for seed in dr.SEEDS:
        for N in dr.NS:
            for screen in dr.SCREENS:
                m = dr.build_model(oracle.api, "cpu", P, seed, with_nir=with_nir)
                flags, (src, kind, noise_row, counts) = plan_of(m, N, screen)
                ns = counts[2]
                noise = torch.randn((ns * N, 3), generator=torch.Generator().manual_seed(77)) if ns else None
                want_p, want_a, want_b = dr.apply_table(m, src, kind, noise_row, noise, N)
                got_counts = m.densify_and_prune(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, screen, None,
                                                 generator=torch.Generator().manual_seed(77), N=N)
                assert got_counts == dr.returned_counts(counts, P, N)
                assert m.P == int(src.numel()) == counts[0] + counts[1] + N * counts[3]
                p, a, b = dr.snapshot(m)
                sam = kind == dr.SAMPLE
                for n, _ in m.fields:
                    if n in ("xyz", "scaling"):
                        # copies are exact; the samples' two computed fields get the last-bit bar tests/test_densify_cpu.py grants
                        assert torch.equal(dr.bits(p[n][~sam]), dr.bits(want_p[n][~sam])), n
                        assert torch.allclose(p[n][sam], want_p[n][sam], rtol=2e-6, atol=1e-6), n
                    else:
                        assert torch.equal(dr.bits(p[n]), dr.bits(want_p[n])), n
                    assert torch.equal(dr.bits(a[n]), dr.bits(want_a[n])) and torch.equal(dr.bits(b[n]), dr.bits(want_b[n])), n
                seen.add((counts[1] > 0, ns > 0, got_counts[2] > 0))
    if P >= 70:
        assert (True, True, True) in seen   # clones, splits and prunes all happened


def test_block_edges_and_constructed_statistics_on_the_host_path(oracle):
    """Selected rows on the first and last row of every 256-row block but one, which has none; denom = 0, 0 / 0 and negative
    statistics; and the fp32-threshold rule: g == float32(max_grad) is selected, the next fp32 below is not."""
    P = 1031
    for N, screen in ((2, None), (3, 20)):
        m = dr.build_model(oracle.api, "cpu", P, 7)
        flags, _ = plan_of(m, N, screen)
        d = {}
        m.densify_and_prune(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, screen, None, generator=torch.Generator().manual_seed(1),
                            N=N, decisions=d)
        clone, split = d["clone"], d["split"]
        assert torch.equal(clone, (flags & dr.CLONE) != 0) and torch.equal(split, (flags & dr.SPLIT) != 0)
        sel = clone | split
        for b in range((P + 255) // 256):
            lo, hi = b * 256, min(b * 256 + 255, P - 1)
            if b == dr.EMPTY_BLOCK:
                assert not bool(sel[lo:hi + 1].any())
            else:
                assert bool(sel[lo]) and bool(sel[hi]), b
        assert bool(sel[dr.ROW_INF]) and not bool(sel[dr.ROW_NAN])                    # x / 0 = inf, 0 / 0 -> 0
        assert bool(clone[dr.ROW_NEG_SMALL]) and not bool(sel[dr.ROW_NEG_LARGE])      # clone on |g|, split on g
        assert bool(clone[dr.ROW_EXACT]) and not bool(sel[dr.ROW_BELOW])
        assert float(d["g"][dr.ROW_EXACT]) == float(dr.f32(dr.MAX_GRAD)) > float(d["g"][dr.ROW_BELOW])


def gpu_inputs(api):
    """Every (model, min_opacity) tests/test_gpu_densify_device.py builds with densify_reference.build_model - built here on the
    CPU from the same recipe.  Its two trainer-based tests densify TRAINED models, which cannot be rebuilt here: they assert
    the same condition on the GPU model in front of every densification."""
    for P in dr.SIZES:
        for seed in dr.SEEDS:
            for nir in (False, True):
                for so in (False, True):
                    for pd in (None, 1e9):
                        yield dr.build_model(api, "cpu", P, seed, with_nir=nir, spatial_order=so, percent_dense=pd), dr.MIN_OPACITY
            yield dr.build_model(api, "cpu", P, seed, overrides=False), 1e-9    # nothing pruned
            yield dr.build_model(api, "cpu", P, seed, overrides=False), dr.MIN_OPACITY
            yield dr.build_model(api, "cpu", P, seed, spatial_order=True, overrides=False), dr.MIN_OPACITY
            yield dr.build_model(api, "cpu", P, seed, spatial_order=True, overrides=False, percent_dense=1e9), dr.MIN_OPACITY
            yield dr.build_model(api, "cpu", P, seed), 2.0                      # every row pruned


def test_every_gpu_input_is_decisive(oracle):
    """Margin condition, 0 rows left out: the float64 decision values lie more than 1e-5 relative (about 100 fp32 ulps) from
    their thresholds, so no last-bit difference between torch's exp / sigmoid and the kernel's can flip a decision."""
    worst = float("inf")
    for m, min_opacity in gpu_inputs(oracle.api):
        for N in dr.NS:
            worst = min(worst, dr.smallest_margin(m, dr.EXTENT, N, min_opacity))
    print("smallest relative margin %.3e" % worst)
    assert worst > 1e-5


def test_the_new_entry_points_are_declared_everywhere():
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert name in PROTOTYPES and name in DEVICE_ONLY, name
        assert re.search(r"\bgs_%s\s*\(" % name, header), name
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)
    assert TrainOptions().densify_on_device is False
    assert TrainOptions(densify_on_device=True).densify_on_device is True


def test_on_device_on_a_cpu_model_raises(oracle):
    m = dr.build_model(oracle.api, "cpu", 70, 3)
    before = m.flat.clone()
    with pytest.raises(RuntimeError, match="no fallback"):
        m.densify_and_prune(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, None, None, on_device=True)
    with pytest.raises(RuntimeError, match="no fallback"):   # (the parity instrument does not excuse it)
        m.densify_and_prune(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, None, None, decisions={}, on_device=True)
    assert m.P == 70 and torch.equal(m.flat, before)
    plain = GaussianModelLite(dr._scene(70, 3), torch.device("cpu"))   # torch Adam: no flat state either
    with pytest.raises(RuntimeError, match="no fallback"):
        plain.densify_and_prune(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, None, None, on_device=True)

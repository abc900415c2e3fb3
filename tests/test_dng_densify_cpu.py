"""DNGaussian's densification rule, mask prunes and opacity resets on GaussianModelLite's host path, held bit for bit to the
restatement of the reference's sequence in tests/dng_densify_reference.py (no GPU needed); the torch restatement of the device
form held to the host path, which proves that the gated plan is still a per-SOURCE-row decision; and the margin condition on
every input tests/test_gpu_dng_densify.py uses."""
import os
import re

import pytest
import torch

import dng_densify_reference as dg
import densify_reference as dr
from gsplat_amd.knn import dist2
from gsplat_amd.trainer import GaussianModelLite, TrainOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("densify_plan_gated", "prune_tmp_bytes", "prune_plan", "prune_emit")


def assert_model_is(m, ref, what=""):
    """Parameters, both moments and the three statistics, bit for bit."""
    got, want = dg.snapshot(m), ref.state()
    assert m.P == ref.P, (what, m.P, ref.P)
    for part_got, part_want in zip(got, want):
        for n, _ in m.fields:
            assert part_got[n].shape == part_want[n].shape, (what, n)
            assert torch.equal(dg.bits(part_got[n]), dg.bits(part_want[n])), (what, n)
    for a, b in zip(dg.statistics(m), (ref.xyz_gradient_accum, ref.denom, ref.max_radii2D)):
        assert a.shape == b.shape and torch.equal(dg.bits(a), dg.bits(b)), (what, "statistics")


def max_dists(oracle, m, kind):
    """None, a float and a tensor [P,1]: around the median 3-NN distance, so that some rows go and most stay."""
    if kind == "none":
        return None
    d = torch.sqrt(dist2(oracle.api, m.params["xyz"].detach()))
    mid = float(d.median()) * 1.5
    if kind == "float":
        return mid
    g = torch.Generator().manual_seed(m.P)
    return (mid * (0.5 + torch.rand((m.P, 1), generator=g))).float()


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dg.SIZES)
def test_prune_points_is_the_reference_indexing(oracle, P, with_nir):
    for name, mask in dg.mask_patterns(P).items():
        for spatial_order in (False, True):
            m = dg.build_model(oracle.api, "cpu", P, 7, with_nir=with_nir, spatial_order=spatial_order)
            ref = dg.Reference.of(m)
            steps, generation = dict(m.optimizer.seg_steps), m.generation
            before, ptr = m.flat.clone(), m.flat.data_ptr()
            m.optimizer.dormant_flags()
            form = mask if name != "alternating" else mask.to(torch.uint8)[:, None]   # (uint8 and [P,1] are masks too)
            n = m.prune_points(form)
            ref.prune_points(mask)
            assert n == int(mask.sum()), name
            assert_model_is(m, ref, name)
            assert m.optimizer.seg_steps == steps
            if n == 0:      # nothing goes: the buffers are left alone
                assert m.generation == generation and m.flat.data_ptr() == ptr and torch.equal(m.flat, before)
            else:
                assert all(p.grad is None for p in m.params.values()) and not m.optimizer._dormant_valid
                assert m.spatial_order == spatial_order
    m = dg.build_model(oracle.api, "cpu", P, 7)
    for bad in (torch.zeros(P + 1, dtype=torch.bool), torch.zeros((P, 2), dtype=torch.bool), torch.zeros((1, P, 1), dtype=torch.bool)):
        with pytest.raises(ValueError):
            m.prune_points(bad)
    with pytest.raises(ValueError):
        m.prune_points(torch.zeros(P))    # a float mask is none
    assert m.P == P


def test_a_pruned_spatially_ordered_model_stays_ordered(oracle):
    from gsplat_amd import synthetic
    m = dg.build_model(oracle.api, "cpu", 1031, 5, spatial_order=True)
    xyz = m.params["xyz"].detach().clone()
    assert torch.equal(xyz, xyz[synthetic.morton_order(xyz)])
    mask = dg.mask_patterns(1031)["random_50pct"]
    m.prune_points(mask)
    # a subsequence of ordered rows: nothing is re-sorted (the Morton box of the smaller set may differ; the order does not)
    assert m.spatial_order and torch.equal(m.params["xyz"].detach(), xyz[~mask])


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dg.SIZES)
def test_densify_and_prune_dng_is_the_reference_sequence(oracle, P, with_nir):
    knn = lambda x: dist2(oracle.api, x)   # noqa: E731
    seen = set()
    for seed in dg.SEEDS:
        for N in dg.NS:
            for kind in ("none", "float", "tensor"):
                m = dg.build_model(oracle.api, "cpu", P, seed, with_nir=with_nir)
                ref = dg.Reference.of(m)
                md = max_dists(oracle, m, kind)
                steps = dict(m.optimizer.seg_steps)
                got = m.densify_and_prune_dng(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, 20, dg.OPA_THRESH, md,
                                              generator=torch.Generator().manual_seed(77), N=N)
                want = ref.densify_and_prune(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, 20, dg.OPA_THRESH, md, knn=knn,
                                             generator=torch.Generator().manual_seed(77), N=N)
                assert got == want, (seed, N, kind)
                assert_model_is(m, ref, (seed, N, kind))
                for t in dg.statistics(m):       # zeroed at the new size
                    assert t.shape[0] == m.P and float(t.abs().sum()) == 0
                assert m.optimizer.seg_steps == steps and all(p.grad is None for p in m.params.values())
                seen.add((got[0] > 0, got[1] > 0, got[2] > 0, got[3] > 0))
    if P >= 70:
        assert any(s[0] for s in seen) and any(s[1] and s[2] and s[3] for s in seen)


@pytest.mark.parametrize("P", dg.SIZES)
def test_the_spatial_order_is_restored_after_a_densification(oracle, P):
    from gsplat_amd import synthetic
    flat_m = dg.build_model(oracle.api, "cpu", P, 7, spatial_order=True)
    so = dg.build_model(oracle.api, "cpu", P, 7, spatial_order=True)
    flat_m.spatial_order = False
    args = (dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, dg.OPA_THRESH)
    r0 = flat_m.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(3))
    r1 = so.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(3))
    assert r0 == r1
    if flat_m.P:
        perm = synthetic.morton_order(flat_m.params["xyz"])
        for part_so, part_flat in zip(dg.snapshot(so), dg.snapshot(flat_m)):
            for n in part_so:
                assert torch.equal(dg.bits(part_so[n]), dg.bits(part_flat[n][perm])), n


@pytest.mark.parametrize("spatial_order", (False, True))
@pytest.mark.parametrize("P", (1, 70, 257))
def test_with_the_gate_open_and_no_size_test_it_is_the_3dgs_rule(oracle, P, spatial_order):
    """opa_thresh below every opacity and max_screen_size = None (no world-size term on the 3DGS side either): without the
    outlier prune densify_and_prune_dng and densify_and_prune are one body - the same counts, the same draws, the same model bit
    for bit."""
    a, b = (dg.build_model(oracle.api, "cpu", P, 7, spatial_order=spatial_order) for _ in range(2))
    assert float(a.get_opacity.detach().min()) > -1.0
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    ra = a.densify_and_prune_dng(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, -1.0, max_dist=None, generator=ga)
    rb = b.densify_and_prune(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, generator=gb)
    assert ra == (0,) + rb and a.P == b.P
    assert torch.equal(ga.get_state(), gb.get_state())
    if P >= 70:
        assert all(c > 0 for c in rb) and a.P > 0
    for part_a, part_b in zip(dg.snapshot(a), dg.snapshot(b)):
        for n in part_b:
            assert part_a[n].shape == part_b[n].shape and torch.equal(dg.bits(part_a[n]), dg.bits(part_b[n])), n
    for sa, sb in zip(dg.statistics(a), dg.statistics(b)):
        assert sa.shape == sb.shape and torch.equal(dg.bits(sa), dg.bits(sb))


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dg.SIZES)
def test_the_device_form_restated_is_the_host_path(oracle, P, with_nir):
    """Gated flags per SOURCE row -> densify_reference's destination table -> the model it describes == the host path.  The
    gate reads the source's own opacity, which a clone and every sample carry unchanged, so nothing needs the new rows."""
    for seed in dg.SEEDS:
        for N in dg.NS:
            m = dg.build_model(oracle.api, "cpu", P, seed, with_nir=with_nir)
            thr = dg.thresholds(N, m.percent_dense)
            flags = dg.gated_flags(m.params["scaling"].detach(), m.params["opacity"].detach(), m.xyz_gradient_accum, m.denom, thr,
                                   dg.OPA_THRESH)
            plain = dr.plan_flags(m.params["scaling"].detach(), m.params["opacity"].detach(), m.xyz_gradient_accum, m.denom, thr,
                                  False)
            src, kind, noise_row, counts = dr.destination_table(flags, N)
            noise = torch.randn((counts[2] * N, 3), generator=torch.Generator().manual_seed(77)) if counts[2] else None
            want_p, want_a, want_b = dr.apply_table(m, src, kind, noise_row, noise, N)
            got = m.densify_and_prune_dng(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, dg.OPA_THRESH,
                                          generator=torch.Generator().manual_seed(77), N=N)
            assert got == (0,) + dr.returned_counts(counts, P, N)
            assert m.P == int(src.numel())
            p, a, b = dg.snapshot(m)
            sam = kind == dr.SAMPLE
            for n, _ in m.fields:
                if n in ("xyz", "scaling"):   # the samples' two computed fields: the last-bit bar tests/test_densify_cpu.py grants
                    assert torch.equal(dg.bits(p[n][~sam]), dg.bits(want_p[n][~sam])), n
                    assert torch.allclose(p[n][sam], want_p[n][sam], rtol=2e-6, atol=1e-6), n
                else:
                    assert torch.equal(dg.bits(p[n]), dg.bits(want_p[n])), n
                assert torch.equal(dg.bits(a[n]), dg.bits(want_a[n])) and torch.equal(dg.bits(b[n]), dg.bits(want_b[n])), n
            if P >= 70:     # the gate alone stops rows the 3DGS plan selects, and only selection bits differ
                diff = flags ^ plain
                assert int(diff[dg.ROW_GATED_CLONE]) == dr.CLONE and int(diff[dg.ROW_GATED_SPLIT]) == dr.SPLIT
                assert int(diff[dg.ROW_CLONE_SHUT]) == dr.CLONE and int(diff[dg.ROW_SPLIT_SHUT]) == dr.SPLIT
                assert int(diff[dg.ROW_CLONE_OPEN]) == 0 and int(diff[dg.ROW_SPLIT_OPEN]) == 0
                assert int(flags[dg.ROW_CLONE_OPEN]) & dr.CLONE and int(flags[dg.ROW_SPLIT_OPEN]) & dr.SPLIT
                assert int(flags[dg.ROW_FAINT]) & dr.PRUNE_SELF and not int(flags[dg.ROW_KEPT]) & dr.PRUNE_SELF
                assert int((diff & ~torch.tensor(dr.CLONE | dr.SPLIT, dtype=torch.uint8)).sum()) == 0


@pytest.mark.parametrize("P", dg.SIZES)
def test_the_prune_table_restated_is_the_host_path(oracle, P):
    for name, mask in dg.mask_patterns(P).items():
        src = dg.prune_table(mask)
        assert torch.equal(src, (~mask).nonzero().squeeze(1)), name
        assert int(dg.prune_block_counts(mask).sum()) == int(src.numel()) == P - int(mask.sum())
        m = dg.build_model(oracle.api, "cpu", P, 5)
        before, stats = dg.snapshot(m), dg.statistics(m)
        m.prune_points(mask)
        for part, old in zip(dg.snapshot(m), before):
            for n in part:
                assert torch.equal(dg.bits(part[n]), dg.bits(old[n][src])), (name, n)
        for new, old in zip(dg.statistics(m), stats):
            assert torch.equal(dg.bits(new), dg.bits(old[src])), name


def gpu_inputs(api):
    """Every model tests/test_gpu_dng_densify.py builds with dng_densify_reference.build_model, rebuilt here from the same recipe
    (its trainer-based test densifies a TRAINED model: it asserts the same condition on the GPU model itself)."""
    for P in dg.SIZES:
        for seed in dg.SEEDS:
            for nir in (False, True):
                for so in (False, True):
                    yield dg.build_model(api, "cpu", P, seed, with_nir=nir, spatial_order=so)


def test_every_gpu_input_is_decisive(oracle):
    """Margin condition: every row's gate, opacity, gradient and size comparison lies more than 1e-5 relative (about 100 fp32
    ulps) from its threshold in float64, so no last-bit difference between torch's exp / sigmoid / division and the kernel's
    can flip a decision.  (The placed opacities sit 1e-4 relative from theirs.)"""
    worst = float("inf")
    for m in gpu_inputs(oracle.api):
        for N in dg.NS:
            worst = min(worst, dg.smallest_margin(m, N))
        for min_opacity in (0.5,):      # prune(min_opacity) of the GPU test
            o = torch.sigmoid(m.params["opacity"].detach().double())
            worst = min(worst, float(((o - min_opacity).abs() / min_opacity).min()))
    print("smallest relative margin %.3e" % worst)
    assert worst > 1e-5
    assert worst < 2e-4     # ... and the placed rows are where they were put


@pytest.mark.parametrize("P", (1, 70, 257))
def test_prune_and_the_opacity_resets(oracle, P):
    m = dg.build_model(oracle.api, "cpu", P, 7, with_nir=True)
    ref = dg.Reference.of(m)
    assert m.prune(0.5) == ref.prune(0.5)
    assert_model_is(m, ref, "prune")
    if m.P == 0:
        return
    # the call without arguments: the bits of the literal expression it has always been
    op = torch.sigmoid(m.params["opacity"].detach().clone())
    new = torch.minimum(op, torch.full_like(op, 0.01))
    literal = torch.log(new / (1 - new))
    others = {n: m.params[n].detach().clone() for n, _ in m.fields if n != "opacity"}
    moments = [{n: v.clone() for n, v in m.optimizer.field_views(buf).items()} for buf in (m.optimizer.exp_avg, m.optimizer.exp_avg_sq)]
    m.reset_opacity()
    ref.reset_opacity()
    assert torch.equal(dg.bits(m.params["opacity"].detach()), dg.bits(literal))
    assert_model_is(m, ref, "reset_opacity()")
    for value, name in ((0.05, "reset_opacity"), (0.8, "reset_opacity_max"), (0.3, "reset_opacity_max")):
        getattr(m, name)(value)
        getattr(ref, name)(value)
        assert_model_is(m, ref, (name, value))
    m.reset_opacity_max()
    ref.reset_opacity_max()
    assert_model_is(m, ref, "reset_opacity_max()")
    for k, buf in enumerate((m.optimizer.exp_avg, m.optimizer.exp_avg_sq)):   # the opacity moments only
        views = m.optimizer.field_views(buf)
        assert int((dg.bits(views["opacity"]) != 0).sum()) == 0
        for n in others:
            assert torch.equal(dg.bits(views[n]), dg.bits(moments[k][n])), n
    for n, v in others.items():
        assert torch.equal(dg.bits(m.params[n].detach()), dg.bits(v)), n


def test_train_iteration_takes_the_dng_rule_on_schedule(oracle):
    from test_trainer_cpu import make_trainer
    from gsplat_amd.trainer import cameras_extent
    log = {}
    for rule in ("dng", "3dgs"):
        tr = make_trainer(oracle, P=60, W=48, H=40, dwt=False)
        model, cams = tr.model, tr.cameras
        calls = []
        for name in ("densify_and_prune_dng", "densify_and_prune"):
            def spy(*a, _inner=getattr(model, name), _name=name, **kw):
                calls.append((_name, a, {k: v for k, v in kw.items() if k != "generator"}, kw["generator"].initial_seed()))
                return _inner(*a, **kw)
            setattr(model, name, spy)
        opt = TrainOptions(iterations=20, densify_from_iter=2, densification_interval=3, opacity_reset_interval=100,
                           densify_until_iter=12, cameras_extent=cameras_extent([c.camera_center for c in cams]),
                           densify_grad_threshold=1e-7, seed=3, densify_rule=rule, split_opacity_thresh=0.2)
        model.active_sh_degree = 0
        out = [tr.train_iteration(it, opt) for it in range(1, 11)]
        log[rule] = (calls, out, model.P)
    calls, out, final_P = log["dng"]
    assert [c[0] for c in calls] == ["densify_and_prune_dng"] * 3
    for (name, a, kw, seed), it in zip(calls, (3, 6, 9)):
        assert a == (1e-7, 0.005, opt.cameras_extent, None, 0.2, None) and seed == 3 * 1000003 + it
        assert kw == dict(on_device=False)
    dens = [o["densified"] for o in out]
    assert [d is not None for d in dens] == [it in (3, 6, 9) for it in range(1, 11)]
    assert all(len(d) == 4 and d[0] == 0 for d in dens if d is not None)
    assert out[-1]["P"] == final_P
    calls, out, _ = log["3dgs"]
    assert [c[0] for c in calls] == ["densify_and_prune"] * 3
    assert all(len(o["densified"]) == 3 for o in out if o["densified"] is not None)
    assert TrainOptions().split_opacity_thresh == 0.1 and TrainOptions().densify_rule == "3dgs"
    tr = make_trainer(oracle, P=60, W=48, H=40, dwt=False)
    bad = TrainOptions(densify_from_iter=0, densification_interval=1, densify_rule="dng")
    bad.densify_rule = "other"
    with pytest.raises(ValueError, match="'3dgs', 'fsgs' or 'dng'"):
        tr.train_iteration(1, bad)


def test_the_new_entry_points_are_declared_everywhere():
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert name in PROTOTYPES and name in DEVICE_ONLY, name
        decl = re.search(r"\bgs_%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(PROTOTYPES[name][1]), name
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)
    # the gated plan is gs_densify_plan's argument list plus the gate
    assert len(PROTOTYPES["densify_plan_gated"][1]) == len(PROTOTYPES["densify_plan"][1]) + 1


def test_on_device_on_a_cpu_model_raises(oracle):
    m = dg.build_model(oracle.api, "cpu", 70, 7)
    before = m.flat.clone()
    mask = dg.mask_patterns(70)["alternating"]
    with pytest.raises(RuntimeError, match="no fallback"):
        m.prune_points(mask, on_device=True)
    with pytest.raises(RuntimeError, match="no fallback"):
        m.prune(0.5, on_device=True)
    with pytest.raises(RuntimeError, match="no fallback"):
        m.densify_and_prune_dng(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, dg.OPA_THRESH, on_device=True)
    with pytest.raises(RuntimeError, match="no fallback"):
        m.densify_and_prune_dng(dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, dg.OPA_THRESH, max_dist=0.1, on_device=True)
    assert m.P == 70 and torch.equal(m.flat, before)
    plain = GaussianModelLite(dr._scene(70, 3), torch.device("cpu"))   # torch Adam: no flat state either
    with pytest.raises(RuntimeError, match="no fallback"):
        plain.prune_points(mask, on_device=True)


def test_the_trainer_prunes_are_the_torch_composition(oracle):
    """prune_near_cameras = the reference's mask_near loop + prune_points; prune_unseen = clean_views: a forward-only render of
    every training camera, radii > 0 ORed, the rest pruned.  Both leave the training state of the cameras alone."""
    from test_trainer_cpu import make_trainer
    from gsplat_amd.trainer import render
    tr = make_trainer(oracle, P=300, W=48, H=40, dwt=False)
    m = tr.model
    for k in range(2):
        tr.step(k)
    xyz = m.params["xyz"].detach().clone()
    centers = torch.stack([xyz[5] + 0.01, xyz[200] - 0.02, torch.tensor([50.0, 50.0, 50.0])])
    near = 0.35
    want = None
    for c in centers:
        t = (xyz - c.repeat(xyz.shape[0], 1)).norm(dim=1, keepdim=True) < near
        want = want + t if want is not None else t
    want = want.squeeze()
    assert 0 < int(want.sum()) < 300
    ref = dg.Reference.of(m)
    ref.prune_points(want)
    assert tr.prune_near_cameras(centers, near) == int(want.sum())
    assert_model_is(m, ref, "near cameras")
    assert tr.prune_near_cameras(centers, near) == 0
    # clean_views: some rows behind both cameras
    c0, c1 = tr.cameras[0].camera_center, tr.cameras[1].camera_center
    assert float(c0 @ c1) > 0
    with torch.no_grad():
        m.params["xyz"][::13] = 5.0 * (c0 + c1) + m.params["xyz"][::13]
    ref = dg.Reference.of(m)
    seen = torch.zeros(m.P, dtype=torch.bool)
    with torch.no_grad():
        for cam in tr.cameras[:2]:
            seen |= render(cam, m, oracle.Rasterizer, oracle.Settings, tr.bg, filter_as_indices=None, clamp=False)["radii"] > 0
    assert 0 < int(seen.sum()) < m.P
    ref.prune_points(~seen)
    assert tr.prune_unseen(camera_indices=(0, 1)) == int((~seen).sum())
    assert_model_is(m, ref, "unseen")
    assert tr.prune_unseen(camera_indices=(0, 1)) == 0
    with pytest.raises(RuntimeError, match="no fallback"):
        tr.prune_unseen(on_device=True)
    with pytest.raises(RuntimeError, match="no fallback"):
        tr.prune_near_cameras(centers, near, opt=TrainOptions(densify_on_device=True))
    float(tr.step(2))     # the next step runs on the pruned model

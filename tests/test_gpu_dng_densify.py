"""prune_points / prune / densify_and_prune_dng with on_device=True - gs_prune_plan, gs_prune_emit, gs_densify_plan_gated and the
gather of csrc/gs_densify.hip - against the host path on the same GPU model.

A prune computes nothing: every bit of parameters, moments and statistics must be the host path's.  The densification's inputs
are those of tests/dng_densify_reference.py, whose every row tests/test_dng_densify_cpu.py shows to be decisive by more than
1e-5 relative, so the discrete results must be EQUAL and every copied value bit-identical; only the split samples' centres and
scales are computed on both sides, and get the bar tests/test_gpu_densify_device.py grants these two fields (rtol 2e-6, atol
1e-6)."""
import pytest
import torch

import densify_reference as dr
import dng_densify_reference as dg
from gsplat_amd import synthetic
from gsplat_amd.knn import dist2
from gsplat_amd.trainer import FlatAdam, TrainOptions, cameras_extent

pytestmark = pytest.mark.gpu
DEV = "cuda"
NULL, SHAPE, SCRATCH = -1, -2, -3
COUNTS = 5    # GS_DENSIFY_COUNTS: the scan's count layout, of which the prune uses column 0


def assert_same_model(a, b, what=""):
    """Parameters, moments and statistics: all bits equal, nothing exempt."""
    assert a.P == b.P, (what, a.P, b.P)
    for pa, pb in zip(dg.snapshot(a), dg.snapshot(b)):
        for n in pa:
            assert pa[n].shape == pb[n].shape and torch.equal(dg.bits(pa[n]), dg.bits(pb[n])), (what, n)
    for sa, sb in zip(dg.statistics(a), dg.statistics(b)):
        assert sa.shape == sb.shape and torch.equal(dg.bits(sa), dg.bits(sb)), (what, "statistics")


def adam_step(m, seed=11):
    """One FlatAdam step on a gradient from a CPU generator."""
    g = torch.randn(m.flat.numel(), generator=torch.Generator().manual_seed(seed)) * 1e-3
    m.flat_grad.copy_(g.to(m.flat.device))
    m.optimizer.step()


@pytest.mark.parametrize("spatial_order", (False, True))
@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dg.SIZES)
def test_prune_points_against_the_host_path(hip, P, with_nir, spatial_order):
    assert FlatAdam.USE_DORMANT
    for name, mask in dg.mask_patterns(P).items():
        a = dg.build_model(hip.api, DEV, P, 7, with_nir=with_nir, spatial_order=spatial_order)
        b = dg.build_model(hip.api, DEV, P, 7, with_nir=with_nir, spatial_order=spatial_order)
        if P > 768:
            for m in (a, b):    # two blocks whose rows never received a gradient: dormant, where they survive whole
                with torch.no_grad():
                    for buf in (m.optimizer.exp_avg, m.optimizer.exp_avg_sq):
                        for v in m.optimizer.field_views(buf).values():
                            v[256:768] = 0.0
        steps, generation = dict(b.optimizer.seg_steps), b.generation
        form = mask.to(DEV) if name != "alternating" else mask.to(torch.uint8)[:, None]   # (a CPU uint8 [P,1] mask is one too)
        na, nb = a.prune_points(form, on_device=False), b.prune_points(form, on_device=True)
        assert na == nb == int(mask.sum()), name
        assert_same_model(a, b, name)
        assert b.optimizer.seg_steps == steps
        if nb == 0:
            assert b.generation == generation
            continue
        assert all(p.grad is None for p in b.params.values())
        for t, shape in zip((b.xyz_gradient_accum, b.denom, b.max_radii2D), ((b.P, 1), (b.P, 1), (b.P,))):
            assert tuple(t.shape) == shape and t.is_cuda
        if b.P == 0:      # all true: both took the host path
            continue
        fa, fb = a.optimizer.dormant_flags(), b.optimizer.dormant_flags()
        assert torch.equal(fa, fb), name
        if name == "random_1pct" and P > 768:     # few rows went: a zeroed block is still whole
            assert int(fb.sum()) >= 1
        adam_step(a)
        adam_step(b)
        assert torch.equal(dg.bits(a.flat), dg.bits(b.flat)), name
        assert torch.equal(dg.bits(a.optimizer.exp_avg), dg.bits(b.optimizer.exp_avg)), name
        assert torch.equal(dg.bits(a.optimizer.exp_avg_sq), dg.bits(b.optimizer.exp_avg_sq)), name


def test_prune_by_opacity_builds_its_mask_on_the_device(hip):
    for P in (70, 1031):
        a, b = dg.build_model(hip.api, DEV, P, 5), dg.build_model(hip.api, DEV, P, 5)
        want = int((torch.sigmoid(a.params["opacity"].detach()) < 0.5).sum())
        assert a.prune(0.5) == b.prune(0.5, on_device=True) == want and 0 < want < P
        assert_same_model(a, b, "prune")


def gate_alone(m, N):
    """Rows the 3DGS plan selects and the gate stops (restatement, on the CPU)."""
    thr = dg.thresholds(N, m.percent_dense)
    args = (m.params["scaling"].detach().cpu(), m.params["opacity"].detach().cpu(), m.xyz_gradient_accum.cpu(), m.denom.cpu(), thr)
    return int((dg.gated_flags(*args, dg.OPA_THRESH) != dr.plan_flags(*args, False)).sum())


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dg.SIZES)
def test_densify_and_prune_dng_against_the_host_path(hip, P, with_nir):
    seen = set()
    for seed in dg.SEEDS:
        for N in dg.NS:
            for with_dist in (False, True):
                a = dg.build_model(hip.api, DEV, P, seed, with_nir=with_nir)
                b = dg.build_model(hip.api, DEV, P, seed, with_nir=with_nir)
                md = None
                if with_dist:     # the composition: gs_knn_mean_dist2, sqrt and compare on the device, the device prune
                    md = float(torch.sqrt(dist2(hip.api, a.params["xyz"].detach())).median()) * 1.5
                stopped = gate_alone(a, N) if not with_dist else 0
                steps = dict(b.optimizer.seg_steps)
                args = (dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, 20, dg.OPA_THRESH, md)
                ra = a.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(77), N=N)
                rb = b.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(77), N=N, on_device=True)
                assert ra == rb, (seed, N, with_dist)
                assert a.P == b.P
                if a.P == 0:
                    continue
                sa, sb = dg.snapshot(a), dg.snapshot(b)
                differing = torch.zeros((a.P,), dtype=torch.bool)
                for n, _ in a.fields:
                    if n in ("xyz", "scaling"):
                        assert torch.allclose(sb[0][n], sa[0][n], rtol=2e-6, atol=1e-6), n
                    else:
                        assert torch.equal(dg.bits(sa[0][n]), dg.bits(sb[0][n])), n
                    differing |= (dg.bits(sa[0][n]) != dg.bits(sb[0][n])).any(dim=1)
                    for k in (1, 2):
                        assert torch.equal(dg.bits(sa[k][n]), dg.bits(sb[k][n])), (n, "moments")
                assert int(differing.sum()) <= N * ra[2]
                # (reference order: the sample blocks are the last rows; everything in front of them is a copy)
                assert not bool(differing[:max(a.P - N * ra[2], 0)].any())
                for t in dg.statistics(b):
                    assert t.shape[0] == b.P and float(t.abs().sum()) == 0
                assert all(p.grad is None for p in b.params.values()) and b.optimizer.seg_steps == steps
                seen.add((ra[0] > 0, ra[1] > 0, ra[2] > 0, ra[3] > 0, stopped > 0))
    if P >= 70:
        assert any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen) and any(s[3] for s in seen)
        assert any(s[4] for s in seen)


def test_the_spatial_order_follows_a_device_densification(hip):
    for with_nir in (False, True):
        flat_m = dg.build_model(hip.api, DEV, 1031, 7, with_nir=with_nir, spatial_order=True)
        so = dg.build_model(hip.api, DEV, 1031, 7, with_nir=with_nir, spatial_order=True)
        flat_m.spatial_order = False
        args = (dg.MAX_GRAD, dg.MIN_OPACITY, dg.EXTENT, None, dg.OPA_THRESH)
        r0 = flat_m.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(3), on_device=True)
        r1 = so.densify_and_prune_dng(*args, generator=torch.Generator().manual_seed(3), on_device=True)
        assert r0 == r1 and r0[1] > 0 and r0[2] > 0 and flat_m.P == so.P
        perm = synthetic.morton_order(flat_m.params["xyz"]).cpu()
        for part_so, part_flat in zip(dg.snapshot(so), dg.snapshot(flat_m)):
            for n in part_so:
                assert torch.equal(dg.bits(part_so[n]), dg.bits(part_flat[n][perm])), n


def test_every_row_pruned_takes_the_host_path(hip):
    a, b = dg.build_model(hip.api, DEV, 70, 5), dg.build_model(hip.api, DEV, 70, 5)
    ga, gb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    ra = a.densify_and_prune_dng(dg.MAX_GRAD, 2.0, dg.EXTENT, None, dg.OPA_THRESH, generator=ga)
    rb = b.densify_and_prune_dng(dg.MAX_GRAD, 2.0, dg.EXTENT, None, dg.OPA_THRESH, generator=gb, on_device=True)
    assert ra == rb and a.P == b.P == 0 and torch.equal(ga.get_state(), gb.get_state())


def plan_args(m, N, thr):
    raw = {n: m.params[n].detach() for n, _ in m.fields}
    return [raw["scaling"].data_ptr(), raw["opacity"].data_ptr(), m.xyz_gradient_accum.data_ptr(), m.denom.data_ptr(), m.P, N,
            float(thr["max_grad"]), float(thr["scale_bound"]), float(thr["min_opacity"]), float(thr["world_bound"]),
            float(thr["sample_div"])]


def test_the_gated_plan_at_the_abi(hip):
    api = hip.api
    for P, N, screen in ((1031, 2, 0), (257, 3, 1), (70, 2, 0)):
        m = dg.build_model(api, DEV, P, 7)
        thr = dg.thresholds(N, m.percent_dense)
        cpu = (m.params["scaling"].detach().cpu(), m.params["opacity"].detach().cpu(), m.xyz_gradient_accum.cpu(), m.denom.cpu(), thr)
        flags = dg.gated_flags(*cpu, dg.OPA_THRESH, bool(screen))
        counts = dr.destination_table(flags, N)[3]
        nbytes = api.raw("densify_tmp_bytes")(P)
        gated, plain, open_ = (torch.zeros((nbytes,), dtype=torch.uint8, device=DEV) for _ in range(3))
        args = plan_args(m, N, thr) + [screen]
        api.call("densify_plan_gated", *args, float(dr.f32(dg.OPA_THRESH)), gated.data_ptr(), nbytes, None)
        api.call("densify_plan", *args, plain.data_ptr(), nbytes, None)
        api.call("densify_plan_gated", *args, -1.0, open_.data_ptr(), nbytes, None)
        torch.cuda.synchronize()
        assert gated[:20].view(torch.int32).cpu().tolist() == counts
        assert torch.equal(gated[256:256 + P].cpu(), flags)
        assert torch.equal(plain[256:256 + P].cpu(), dr.plan_flags(*cpu, bool(screen)))     # gs_densify_plan: what it always wrote
        assert torch.equal(open_, plain)                                                   # gate -1: the same bytes, all of tmp
        assert not torch.equal(gated, plain)


def prune_call(api, m, mask, tmp, nbytes, P2, table, new_xyz, new_stats):
    return api.raw("prune_emit")(tmp.data_ptr(), nbytes, mask.data_ptr(), m.params["xyz"].detach().data_ptr(), m.P, P2,
                                 table.data_ptr(), new_xyz.data_ptr(), m.xyz_gradient_accum.data_ptr(), m.denom.data_ptr(),
                                 m.max_radii2D.data_ptr(), new_stats[0].data_ptr(), new_stats[1].data_ptr(), new_stats[2].data_ptr(),
                                 None)


def test_the_prune_plan_and_table_at_the_abi(hip):
    api = hip.api
    for P in (70, 257, 1031):
        m = dg.build_model(api, DEV, P, 5)
        nbytes = api.raw("prune_tmp_bytes")(P)
        nb = (P + 255) // 256
        for name, mask in dg.mask_patterns(P).items():
            src = dg.prune_table(mask)
            P2 = int(src.numel())
            dmask = mask.to(torch.uint8).to(DEV) * 3      # any nonzero byte removes
            tmp = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
            api.call("prune_plan", dmask.data_ptr(), P, tmp.data_ptr(), nbytes, None)
            torch.cuda.synchronize()
            assert int(tmp[:4].view(torch.int32).cpu()) == P2, name
            per_block = tmp[256:256 + 4 * COUNTS * nb].view(torch.int32).view(nb, COUNTS)[:, 0].cpu().to(torch.int64)
            assert torch.equal(per_block, dg.prune_block_counts(mask)), name
            if P2 == 0:
                continue
            table = torch.full((P2,), -1, dtype=torch.int32, device=DEV)
            new_xyz = torch.full((P2, 3), 7.0, device=DEV)
            new_stats = [torch.full((P2,), 7.0, device=DEV) for _ in range(3)]
            # a count that is not the plan's: accepted as a shape, but the kernel finds another total in tmp and writes nothing
            if P2 > 1:
                assert prune_call(api, m, dmask, tmp, nbytes, P2 - 1, table, new_xyz, new_stats) == 0
                torch.cuda.synchronize()
                assert int((table != -1).sum()) == 0 and int((new_xyz != 7.0).sum()) == 0
                assert all(int((s != 7.0).sum()) == 0 for s in new_stats)
            assert prune_call(api, m, dmask, tmp, nbytes, P2, table, new_xyz, new_stats) == 0
            torch.cuda.synchronize()
            t = table.cpu().to(torch.int64) & 0xFFFFFFFF
            assert torch.equal(t & 0x3FFFFFFF, src) and int((t >> 30).sum()) == 0, name     # every row a survivor
            assert torch.equal(new_xyz.cpu(), m.params["xyz"].detach().cpu()[src])
            for s, old in zip(new_stats, dg.statistics(m)):
                assert torch.equal(dg.bits(s.cpu()), dg.bits(old.reshape(-1)[src]))


def test_abi_errors_touch_no_memory(hip):
    api = hip.api
    P, N = 300, 2
    assert api.raw("prune_tmp_bytes")(0) == 0
    nbytes, dn_bytes = api.raw("prune_tmp_bytes")(P), api.raw("densify_tmp_bytes")(P)
    tmp = torch.full((max(nbytes, dn_bytes),), 0x5A, dtype=torch.uint8, device=DEV)
    f = torch.zeros((P * 3,), device=DEV)
    out = torch.full((P * 3,), 7.0, device=DEV)
    tab = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    mask = torch.zeros((P,), dtype=torch.uint8, device=DEV)
    p, o = f.data_ptr(), out.data_ptr()

    def gated(scaling=p, tmp_ptr=tmp.data_ptr(), P_=P, N_=N, nbytes_=dn_bytes):
        return api.raw("densify_plan_gated")(scaling, p, p, p, P_, N_, 2e-4, 0.044, 0.005, 0.44, 1.6, 0, 0.1, tmp_ptr, nbytes_, None)

    def plan(mask_ptr=mask.data_ptr(), tmp_ptr=tmp.data_ptr(), P_=P, nbytes_=nbytes):
        return api.raw("prune_plan")(mask_ptr, P_, tmp_ptr, nbytes_, None)

    def emit(mask_ptr=mask.data_ptr(), xyz=p, table=tab.data_ptr(), stat=p, new_stat=o, P_=P, P2=P, nbytes_=nbytes):
        return api.raw("prune_emit")(tmp.data_ptr(), nbytes_, mask_ptr, xyz, P_, P2, table, o, stat, p, p, new_stat, o, o, None)

    assert gated(scaling=None) == NULL and gated(tmp_ptr=None) == NULL
    assert gated(P_=0) == SHAPE and gated(N_=0) == SHAPE and gated(N_=9) == SHAPE and gated(nbytes_=dn_bytes - 1) == SCRATCH
    assert plan(mask_ptr=None) == NULL and plan(tmp_ptr=None) == NULL and plan(P_=0) == SHAPE and plan(nbytes_=nbytes - 1) == SCRATCH
    assert emit(mask_ptr=None) == NULL and emit(xyz=None) == NULL and emit(table=None) == NULL
    assert emit(stat=None) == NULL and emit(new_stat=None) == NULL
    assert emit(P_=0) == SHAPE and emit(P2=0) == SHAPE and emit(P2=P + 1) == SHAPE and emit(nbytes_=nbytes - 1) == SCRATCH
    torch.cuda.synchronize()
    assert int((tmp != 0x5A).sum()) == 0 and int((out != 7.0).sum()) == 0 and int((tab != -1).sum()) == 0


def test_train_iteration_across_a_near_camera_prune_and_the_first_densification(hip):
    """densify_rule = "dng" with densify_on_device on and off: three iterations, a near-camera prune (on_device from the
    options the trainer last ran with), then the first densifying iteration.  The prune computes nothing, so the two models are
    the same bits going into the densification; behind it they hold the same P and the same rows outside the sample rows, which
    stay within the samples' bar.  The model is a trained one, which the CPU test cannot show decisive: the margin condition is
    asserted here, on the GPU model, in front of the prune and of the densification."""
    import dng_reg_reference as rr
    from test_gpu_densify_device import make_trainer
    runs = []
    for flag in (False, True):
        tr = make_trainer(hip)
        model = tr.model
        inner = model.densify_and_prune_dng
        seen = {}

        def checked(*a, _inner=inner, _m=model, _seen=seen, **kw):
            assert dg.smallest_margin(_m, kw.get("N", 2), opa_thresh=a[4], min_opacity=a[1], max_grad=a[0], extent=a[2],
                                      constructed=False) > 1e-5
            _seen["before"] = (dg.snapshot(_m), _m.P)
            _seen["on_device"] = kw["on_device"]
            return _inner(*a, **kw)
        model.densify_and_prune_dng = checked
        opt = TrainOptions(iterations=40, densify_from_iter=2, densification_interval=4, opacity_reset_interval=100,
                           densify_until_iter=30, cameras_extent=cameras_extent([c.camera_center for c in tr.cameras]),
                           densify_grad_threshold=1e-7, seed=3, densify_on_device=flag, densify_rule="dng")
        model.active_sh_degree = 0
        for it in (1, 2, 3):
            assert tr.train_iteration(it, opt)["densified"] is None
        tr.sync()
        xyz = model.params["xyz"].detach()
        centers = xyz[[5, 100, 250]].clone() + 0.01
        near = 0.3
        want, margin = rr.near_mask(xyz.cpu(), centers.cpu(), near)
        assert margin > 1e-5
        n_near = tr.prune_near_cameras(centers, near)
        assert n_near == int(want.sum()) and 0 < n_near < 300 and model.P == 300 - n_near
        out = tr.train_iteration(4, opt)
        assert seen["on_device"] is flag
        runs.append((n_near, out["densified"], out["P"], seen["before"], dg.snapshot(model)))
    off, on = runs
    assert off[:3] == on[:3] and len(on[1]) == 4
    n_out, n_clone, n_split, n_pruned = on[1]
    assert n_out == 0 and n_clone + n_split > 0
    for x, y in zip(off[3][0], on[3][0]):        # going into the densification: the same bits
        for n in x:
            assert torch.equal(dg.bits(x[n]), dg.bits(y[n])), n
    P2, copies = on[2], on[2] - 2 * n_split
    for k in range(3):
        for n in off[4][k]:
            x, y = off[4][k][n], on[4][k][n]
            assert x.shape == y.shape and x.shape[0] == P2
            if k == 0 and n in ("xyz", "scaling"):
                assert torch.equal(dg.bits(x[:max(copies, 0)]), dg.bits(y[:max(copies, 0)])), n
                assert torch.allclose(y, x, rtol=2e-6, atol=1e-6), n
            else:
                assert torch.equal(dg.bits(x), dg.bits(y)), (k, n)

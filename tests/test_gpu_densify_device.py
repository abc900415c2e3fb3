"""densify_and_prune(on_device=True) - the kernels of csrc/gs_densify.hip - against the host path on the same GPU model.

The inputs are those of tests/densify_reference.py, whose every row tests/test_densify_device_cpu.py shows to be decisive by
more than 1e-5 relative: no last-bit difference between torch's exp / sigmoid and the kernels' can flip a decision, so the
discrete results must be EQUAL and every copied value bit-identical.  Only the split samples' centres and scales are
computed on both sides; they get the bar tests/test_densify_cpu.py already grants these two fields (rtol 2e-6, atol 1e-6)."""
import ctypes as C

import pytest
import torch

import densify_reference as dr
from gsplat_amd import synthetic
from gsplat_amd.trainer import GaussianModelLite, TrainOptions, Trainer, camera_to, cameras_extent

pytestmark = pytest.mark.gpu
DEV = "cuda"


def densify(m, on_device, N=2, screen=None, min_opacity=dr.MIN_OPACITY, seed=77, **kw):
    gen = torch.Generator().manual_seed(seed)
    out = m.densify_and_prune(dr.MAX_GRAD, min_opacity, dr.EXTENT, screen, None, generator=gen, N=N, on_device=on_device, **kw)
    return out, gen


def assert_same_bits(x, y, what=""):
    px, ax, bx = x
    py, ay, by = y
    for n in px:
        assert px[n].shape == py[n].shape, (what, n)
        assert torch.equal(dr.bits(px[n]), dr.bits(py[n])), (what, n)
        assert torch.equal(dr.bits(ax[n]), dr.bits(ay[n])) and torch.equal(dr.bits(bx[n]), dr.bits(by[n])), (what, n, "moments")


def reference_counts(m, N, screen, min_opacity=dr.MIN_OPACITY):
    thr = dr.thresholds(dr.MAX_GRAD, min_opacity, dr.EXTENT, m.percent_dense, N)
    flags = dr.plan_flags(m.params["scaling"].detach().cpu(), m.params["opacity"].detach().cpu(), m.xyz_gradient_accum.cpu(),
                          m.denom.cpu(), thr, bool(screen))
    return flags, dr.destination_table(flags, N)


@pytest.mark.parametrize("with_nir", (False, True))
@pytest.mark.parametrize("P", dr.SIZES)
def test_against_the_host_path(hip, P, with_nir):
    seen = set()
    for seed in dr.SEEDS:
        for N in dr.NS:
            for screen in dr.SCREENS:
                a = dr.build_model(hip.api, DEV, P, seed, with_nir=with_nir)
                b = dr.build_model(hip.api, DEV, P, seed, with_nir=with_nir)
                _, (src, kind, _, counts) = reference_counts(a, N, screen)
                steps = dict(b.optimizer.seg_steps)
                (ra, _), (rb, _) = densify(a, False, N, screen), densify(b, True, N, screen)
                assert ra == rb == dr.returned_counts(counts, P, N), (ra, rb)
                assert a.P == b.P == int(src.numel())
                if a.P == 0:    # (P = 1 with the faint override: every row pruned, both took the host path)
                    continue
                sa, sb = dr.snapshot(a), dr.snapshot(b)
                sam = kind == dr.SAMPLE
                differing = torch.zeros((a.P,), dtype=torch.bool)
                for n, _ in a.fields:
                    if n in ("xyz", "scaling"):
                        assert torch.equal(dr.bits(sa[0][n][~sam]), dr.bits(sb[0][n][~sam])), n
                        assert torch.allclose(sb[0][n][sam], sa[0][n][sam], rtol=2e-6, atol=1e-6), n
                    else:
                        assert torch.equal(dr.bits(sa[0][n]), dr.bits(sb[0][n])), n
                    differing |= (dr.bits(sa[0][n]) != dr.bits(sb[0][n])).any(dim=1)
                    for k in (1, 2):
                        assert torch.equal(dr.bits(sa[k][n]), dr.bits(sb[k][n])), (n, "moments")
                assert int(differing.sum()) <= N * counts[2]
                assert all(p.grad is None for p in b.params.values()) and b.optimizer.seg_steps == steps
                seen.add((ra[0] > 0, ra[1] > 0, ra[2] > 0))
    if P >= 70:
        assert (True, True, True) in seen


def test_plan_and_emit_at_the_abi_are_the_reference_table(hip, oracle):
    """The flag bytes, the five totals and the destination table of the kernels equal the torch restatement's, entry for entry."""
    api = hip.api
    for N, screen in ((2, None), (3, 20)):
        m = dr.build_model(api, DEV, 1031, 7)
        P = m.P
        flags, (src, kind, noise_row, counts) = reference_counts(m, N, screen)
        thr = dr.thresholds(dr.MAX_GRAD, dr.MIN_OPACITY, dr.EXTENT, m.percent_dense, N)
        nbytes = api.raw("densify_tmp_bytes")(P)
        tmp = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
        raw = {n: m.params[n].detach() for n, _ in m.fields}
        api.call("densify_plan", raw["scaling"].data_ptr(), raw["opacity"].data_ptr(), m.xyz_gradient_accum.data_ptr(),
                 m.denom.data_ptr(), P, N, float(thr["max_grad"]), float(thr["scale_bound"]), float(thr["min_opacity"]),
                 float(thr["world_bound"]), float(thr["sample_div"]), 1 if screen else 0, tmp.data_ptr(), nbytes, None)
        torch.cuda.synchronize()
        assert tmp[:20].view(torch.int32).cpu().tolist() == counts
        assert torch.equal(tmp[256:256 + P].cpu(), flags)
        P2 = int(src.numel())
        noise = torch.randn((counts[2] * N, 3), generator=torch.Generator().manual_seed(5))
        table = torch.full((P2,), -1, dtype=torch.int32, device=DEV)
        new_xyz = torch.zeros((P2, 3), device=DEV)
        nz = noise.to(DEV)
        args = [tmp.data_ptr(), nbytes, raw["xyz"].data_ptr(), raw["scaling"].data_ptr(), raw["rotation"].data_ptr(), nz.data_ptr(),
                P, N, counts[0], counts[1], counts[2], counts[3], P2, table.data_ptr(), new_xyz.data_ptr(), None]
        api.call("densify_emit", *args)
        torch.cuda.synchronize()
        t = table.cpu().to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(t & 0x3FFFFFFF, src) and torch.equal(t >> 30, kind)
        want = dr.apply_table(dr.build_model(oracle.api, "cpu", 1031, 7), src, kind, noise_row, noise, N)[0]["xyz"]
        assert torch.allclose(new_xyz.cpu(), want, rtol=2e-6, atol=1e-6)
        assert torch.equal(new_xyz.cpu()[kind != dr.SAMPLE], want[kind != dr.SAMPLE])
        # counts that are not the plan's: accepted as a shape, but the kernel finds other totals in tmp and writes nothing
        table.fill_(-1)
        bad = list(args)
        bad[8], bad[12] = counts[0] - 1, P2 - 1
        api.call("densify_emit", *bad)
        torch.cuda.synchronize()
        assert int((table != -1).sum()) == 0


@pytest.mark.parametrize("P,with_nir", ((1, False), (70, False), (257, False), (1031, False), (1031, True)))
def test_spatial_order(hip, P, with_nir):
    """(P = 1 without the overrides, which would prune its only row: one point, hi == lo in the codes kernel; its statistic is
    set so that the row is left alone with no screen size and split with one.)"""
    kw = dict(with_nir=with_nir, spatial_order=True, overrides=P > 1)
    for seed in dr.SEEDS:
        for N in dr.NS:
            for screen in dr.SCREENS:
                flat_m, so = dr.build_model(hip.api, DEV, P, seed, **kw), dr.build_model(hip.api, DEV, P, seed, **kw)
                flat_m.spatial_order = False          # the same model, re-laid out in the reference order
                if P == 1:
                    for m in (flat_m, so):
                        m.xyz_gradient_accum.fill_(1e-3 if screen else 0.0)
                        m.denom.fill_(1.0)
                (r0, _), (r1, _) = densify(flat_m, True, N, screen), densify(so, True, N, screen)
                assert r0 == r1 and flat_m.P == so.P > 0
                assert r0[1] > 0 or P < 257 and (P > 1 or not screen), (r0, P, screen)
                perm = synthetic.morton_order(flat_m.params["xyz"]).cpu()
                want = tuple({n: v[perm] for n, v in part.items()} for part in dr.snapshot(flat_m))
                assert_same_bits(dr.snapshot(so), want, "spatial order")
                xyz = so.params["xyz"].detach()
                assert torch.equal(xyz, xyz[synthetic.morton_order(xyz)])
        # clone / prune only: nothing is computed, so the host path's result is the device's bit for bit, order included
        host = dr.build_model(hip.api, DEV, P, seed, percent_dense=1e9, **kw)
        dev = dr.build_model(hip.api, DEV, P, seed, percent_dense=1e9, **kw)
        (rh, _), (rd, _) = densify(host, False), densify(dev, True)
        assert rh == rd and host.P == dev.P > 0
        assert P < 257 or (rh[0] > 0 and rh[1] == 0 and rh[2] > 0)
        assert_same_bits(dr.snapshot(dev), dr.snapshot(host), "clone / prune only")


def test_nothing_selected_and_nothing_pruned_is_a_copy(hip):
    for P in (70, 1031):
        m = dr.build_model(hip.api, DEV, P, 5, overrides=False)
        m.xyz_gradient_accum.zero_()
        before, generation = dr.snapshot(m), m.generation
        (res, gen) = densify(m, True, min_opacity=1e-9)
        assert res == (0, 0, 0) and m.P == P and m.generation == generation + 1
        assert_same_bits(dr.snapshot(m), before, "copy")
        assert torch.equal(gen.get_state(), torch.Generator().manual_seed(77).get_state())   # ns == 0: no draw
        for t, shape in ((m.xyz_gradient_accum, (P, 1)), (m.denom, (P, 1)), (m.max_radii2D, (P,))):
            assert t.shape == shape and t.is_cuda and float(t.abs().sum()) == 0


def test_a_single_gaussian(hip):
    """P = 1 through the kernels (without the overrides, which prune row 0): statistic 0 is a pure survivor copy, 1e-3 a split
    into N samples.  Copied values and both moments bit for bit; only the samples' xyz and scaling are computed."""
    for seed in dr.SEEDS:
        for accum, N, want in ((0.0, 2, (0, 0, 0)), (1e-3, 2, (0, 1, 0)), (1e-3, 3, (0, 1, 0))):
            a, b = (dr.build_model(hip.api, DEV, 1, seed, overrides=False) for _ in range(2))
            for m in (a, b):
                m.xyz_gradient_accum.fill_(accum)
                m.denom.fill_(1.0)
            (ra, _), (rb, _) = densify(a, False, N), densify(b, True, N)
            assert ra == rb == want and a.P == b.P == (N if accum else 1)
            sa, sb = dr.snapshot(a), dr.snapshot(b)
            for n in sa[0]:
                if accum and n in ("xyz", "scaling"):
                    assert torch.allclose(sb[0][n], sa[0][n], rtol=2e-6, atol=1e-6), (seed, accum, n)
                else:
                    assert torch.equal(dr.bits(sb[0][n]), dr.bits(sa[0][n])), (seed, accum, n)
                for k in (1, 2):
                    assert torch.equal(dr.bits(sb[k][n]), dr.bits(sa[k][n])), (seed, accum, n, "moments")
            if not accum:   # the survivor keeps its moments, signed zeros included
                assert int((dr.bits(sb[1]["features"]) != 0).sum()) > 0 and int((dr.bits(sb[2]["features"]) != 0).sum()) > 0


def test_every_row_pruned_and_the_parity_instrument_take_the_host_path(hip):
    a, b = dr.build_model(hip.api, DEV, 70, 3), dr.build_model(hip.api, DEV, 70, 3)
    (ra, ga), (rb, gb) = densify(a, False, min_opacity=2.0), densify(b, True, min_opacity=2.0)
    assert ra == rb and a.P == b.P == 0 and torch.equal(ga.get_state(), gb.get_state())
    a, b = dr.build_model(hip.api, DEV, 257, 3), dr.build_model(hip.api, DEV, 257, 3)
    d = {}
    (ra, _), (rb, _) = densify(a, False), densify(b, True, decisions=d)
    assert ra == rb and {"clone", "split", "prune", "g"} <= set(d)
    assert_same_bits(dr.snapshot(b), dr.snapshot(a), "decisions")   # (both the host path: the same bits)


def test_postfix_padding_and_dormant_flags(hip):
    m = dr.build_model(hip.api, DEV, 1031, 3, spatial_order=True)
    opt = m.optimizer
    with torch.no_grad():   # two blocks whose rows never received a gradient
        for buf in (opt.exp_avg, opt.exp_avg_sq):
            for v in opt.field_views(buf).values():
                v[256:768] = 0.0
    steps = dict(opt.seg_steps)
    densify(m, True, 3, 20)
    assert all(p.grad is None for p in m.params.values()) and opt.seg_steps == steps
    n = m.P * m.width
    assert m.flat_padded.numel() % 3360 == 0 and opt.exp_avg_padded.numel() == m.flat_padded.numel()
    for buf in (m.flat_padded, opt.exp_avg_padded, opt.exp_avg_sq_padded):
        assert int((buf[n:].view(torch.int32) != 0).sum()) == 0
    nb = (m.P + 255) // 256
    live = torch.zeros((nb * 256,), dtype=torch.bool, device=DEV)
    for buf in (opt.exp_avg, opt.exp_avg_sq):
        for v in opt.field_views(buf).values():
            live[:m.P] |= (v.view(torch.int32) != 0).any(dim=1)
    assert torch.equal(opt.dormant_flags(), (~live.view(nb, 256).any(dim=1)).to(torch.uint8))


def test_two_runs_give_the_same_bits(hip):
    runs = []
    for _ in range(2):
        m = dr.build_model(hip.api, DEV, 1031, 7, with_nir=True, spatial_order=True)
        res, _ = densify(m, True, 3, 20)
        runs.append((res, dr.snapshot(m)))
    assert runs[0][0] == runs[1][0] and runs[0][0][1] > 0
    assert_same_bits(runs[0][1], runs[1][1], "determinism")


def test_abi_errors_touch_no_memory(hip):
    api = hip.api
    P, N = 300, 2
    assert api.raw("densify_tmp_bytes")(0) == 0
    nbytes = api.raw("densify_tmp_bytes")(P)
    tmp = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    f = torch.zeros((P * 59,), device=DEV)
    out = torch.full((P * 59,), 7.0, device=DEV)
    tab = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    p = f.data_ptr()
    widths = (C.c_int32 * 5)(3, 48, 1, 3, 4)
    NULL, SHAPE = -1, -2

    def plan(scaling=p, tmp_ptr=tmp.data_ptr(), P_=P, N_=N):
        return api.raw("densify_plan")(scaling, p, p, p, P_, N_, 2e-4, 0.044, 0.005, 0.44, 1.6, 0, tmp_ptr, nbytes, None)

    def emit(xyz=p, table=tab.data_ptr(), P_=P, N_=N, n_keep=P, P2=P):
        return api.raw("densify_emit")(tmp.data_ptr(), nbytes, xyz, p, p, None, P_, N_, n_keep, 0, 0, 0, P2, table, out.data_ptr(), None)

    def gather(table=tab.data_ptr(), P_=P, P2=P, nfields=5):
        return api.raw("densify_gather")(None, table, p, P2, p, p, p, P_, out.data_ptr(), out.data_ptr(), out.data_ptr(), nfields,
                                         widths, 0, 3, 1.6, None)

    assert plan(scaling=None) == NULL and plan(tmp_ptr=None) == NULL
    assert plan(P_=0) == SHAPE and plan(N_=0) == SHAPE and plan(N_=9) == SHAPE
    assert emit(xyz=None) == NULL and emit(table=None) == NULL
    assert emit(P_=0) == SHAPE and emit(N_=0) == SHAPE and emit(N_=9) == SHAPE
    assert emit(P2=P + 1) == SHAPE and emit(n_keep=P + 1, P2=P + 1) == SHAPE     # counts that do not add up / exceed P
    assert gather(table=None) == NULL and gather(P_=0) == SHAPE and gather(P2=0) == SHAPE and gather(nfields=9) == SHAPE
    codes = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    assert api.raw("morton_codes")(None, P, p, p, codes.data_ptr(), None) == NULL
    assert api.raw("morton_codes")(p, 0, p, p, codes.data_ptr(), None) == SHAPE
    torch.cuda.synchronize()
    assert int((tmp != 0x5A).sum()) == 0 and int((out != 7.0).sum()) == 0 and int((tab != -1).sum()) == 0
    assert int((codes != -1).sum()) == 0


def make_trainer(hip, P=300, W=96, H=80):
    import diff_gaussian_rasterization as dgr
    import lgdwt_loss
    dev = torch.device(DEV)
    sc = synthetic.trained_like(P, seed=0, scale_mult=1.5)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:4]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g).to(dev) for _ in cams]
    model = GaussianModelLite(sc, dev, api=hip.api)
    crit = lgdwt_loss.criterion(dwt_enable=False, patch_dwt_enable=False)
    return Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, torch.zeros(3, device=dev))


def test_a_train_step_after_the_device_densify_is_the_one_after_the_host_densify(hip):
    """Clone / prune only (nothing computed): the two models are the same bits, and stay so through the next fused step.
    The inputs are three trained steps away from a synthetic scene, so the CPU test cannot show them decisive: the margin
    condition is asserted here, on the GPU model, before it is densified."""
    a, b = make_trainer(hip), make_trainer(hip)
    for tr in (a, b):
        for k in range(3):
            tr.step(k)
        tr.sync()
        tr.gather_optimizer_state()
        tr.model.percent_dense = 1e9
        assert dr.smallest_margin(tr.model, 4.4, 2, 0.005) > 1e-5
    ra = a.model.densify_and_prune(1e-7, 0.005, 4.4, None, None, generator=torch.Generator().manual_seed(1))
    rb = b.model.densify_and_prune(1e-7, 0.005, 4.4, None, None, generator=torch.Generator().manual_seed(1), on_device=True)
    assert ra == rb and ra[0] > 0 and ra[1] == 0 and a.model.P == b.model.P
    assert_same_bits(dr.snapshot(b.model), dr.snapshot(a.model), "before the step")
    for tr in (a, b):
        tr.step(3)
        tr.sync()
    torch.cuda.synchronize()
    print("step path", a.last["path"], b.last["path"])
    # "manual": the fused step (gs_backward_step: backward, statistics and Adam in one pass) driven without autograd
    assert a.last["path"] == b.last["path"] == "manual"
    assert torch.equal(a.model.flat, b.model.flat)
    assert torch.equal(a.model.optimizer.exp_avg, b.model.optimizer.exp_avg)
    assert torch.equal(a.model.optimizer.exp_avg_sq, b.model.optimizer.exp_avg_sq)


def test_train_iteration_schedule_with_the_device_densify(hip):
    """The shape of tests/test_densify_cpu.py::test_train_iteration_schedule (P = 300, 96 x 80) with densify_on_device on and off:
    the same P sequence and (n_clone, n_split, n_pruned) tuples, losses within 1e-5 relative up to the first split.  At the
    first split the samples' centres and scales may differ in their last bits (rtol 2e-6, atol 1e-6, as above), so the losses
    are not compared bit for bit behind it; the discrete sequence is still asserted over the whole schedule.
    The models are trained ones, which the CPU test cannot show decisive: the margin condition is asserted on the GPU model
    in front of every densification of either run."""
    runs = []
    for flag in (False, True):
        tr = make_trainer(hip)
        inner = tr.model.densify_and_prune

        def checked(max_grad, min_opacity, extent, *a, _inner=inner, _m=tr.model, **kw):
            assert dr.smallest_margin(_m, extent, kw.get("N", 2), min_opacity) > 1e-5
            return _inner(max_grad, min_opacity, extent, *a, **kw)
        tr.model.densify_and_prune = checked
        opt = TrainOptions(iterations=40, densify_from_iter=3, densification_interval=4, opacity_reset_interval=10,
                           densify_until_iter=30, sh_increase_interval=5,
                           cameras_extent=cameras_extent([c.camera_center for c in tr.cameras]), densify_grad_threshold=1e-7,
                           seed=3, densify_on_device=flag)
        tr.model.active_sh_degree = 0
        log = []
        for it in range(1, 26):
            out = tr.train_iteration(it, opt)
            log.append((out["P"], out["densified"], float(out["loss"])))
        runs.append(log)
    off, on = runs
    assert [r[:2] for r in off] == [r[:2] for r in on]
    dens = [r[1] for r in on if r[1] is not None]
    assert len(dens) >= 5 and any(d[0] + d[1] > 0 for d in dens)
    first_split = next((k for k, r in enumerate(on) if r[1] is not None and r[1][1] > 0), len(on) - 1)
    for k in range(first_split + 1):
        assert abs(on[k][2] - off[k][2]) <= 1e-5 * abs(off[k][2]), (k, on[k], off[k])

"""densify_and_prune_fsgs(on_device=True) - the gs_densify_fsgs_* kernels of csrc/gs_densify.hip and two HIP kNN searches -
against the host path on the same GPU model and against the CPU run with the oracle's kNN.

The inputs are those of tests/fsgs_densify_reference.py, which tests/test_fsgs_densify_cpu.py shows to be decisive by more
than 1e-5 relative with unambiguous neighbour lists: no last-bit difference between torch's exp / sigmoid and the kernels',
or between the two sides' sample centres in front of kNN #2, can flip a decision or a neighbour.  So counts and row order
must be EQUAL and every copied value and every moment bit-identical.  Only what goes back to a split sample is computed on
both sides - the samples' centres and scalings, and the proximity rows derived from them; these get the bar
tests/test_gpu_densify_device.py grants those fields (rtol 2e-6, atol 1e-6)."""
import ctypes as C

import pytest
import torch

import fsgs_densify_reference as fr
from gsplat_amd import synthetic
from gsplat_amd.knn import dist2_with_indices
from gsplat_amd.trainer import GaussianModelLite, TrainOptions, Trainer, camera_to

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(it, N, screen) for it in fr.ITERATIONS for N in fr.NS for screen in fr.SCREENS]


def hip_knn(hip):
    def knn(xyz):
        dist, nearest = dist2_with_indices(hip.api, xyz.to(DEV))
        return dist.cpu(), nearest.cpu()
    return knn


def assert_same_model(got, want, computed=None, what=""):
    """Snapshots (params, exp_avg, exp_avg_sq): moments and copied values bit for bit; with `computed` (field -> row mask) those
    rows of xyz / scaling at the samples' bar."""
    assert got[0]["xyz"].shape == want[0]["xyz"].shape, what
    for n in want[0]:
        g, w = got[0][n], want[0][n]
        if computed is not None and n in computed:
            c = computed[n]
            assert torch.equal(fr.bits(g[~c]), fr.bits(w[~c])), (what, n)
            assert torch.allclose(g[c], w[c], rtol=2e-6, atol=1e-6), (what, n)
        else:
            assert torch.equal(fr.bits(g), fr.bits(w)), (what, n)
        for k in (1, 2):
            assert torch.equal(fr.bits(got[k][n]), fr.bits(want[k][n])), (what, n, "moments")


def computed_rows(m, knn, it, N, screen):
    """Which rows of the result go back to a split sample (from the restatement on this model's rows, reference order)."""
    _, counts, info = fr.run_reference(m, knn, it, N, screen)
    return counts, info["computed"]


@pytest.mark.parametrize("P", fr.SIZES)
def test_against_the_host_path(hip, P):
    knn = hip_knn(hip)
    seen = set()
    for it, N, screen in CASES:
        a, b = fr.build_model(hip.api, DEV, P), fr.build_model(hip.api, DEV, P)
        counts, computed = computed_rows(a, knn, it, N, screen)
        steps = dict(b.optimizer.seg_steps)
        (ra, ga), (rb, gb) = fr.run_model(a, it, N, screen), fr.run_model(b, it, N, screen, on_device=True)
        assert ra == rb == counts, (it, N, screen, ra, rb, counts)
        assert a.P == b.P == int(computed["xyz"].numel()) > 0
        assert torch.equal(ga.get_state(), gb.get_state())
        sa, sb = fr.snapshot(a), fr.snapshot(b)
        assert_same_model(sb, sa, computed, (it, N, screen))
        # new rows' moments are +0 (the bits, not just the value); the surviving rows come first and keep theirs
        n_old = P - (ra[1] if it > fr.PRUNE_FROM else 0)
        for k in (1, 2):
            for n in sb[k]:
                assert int((fr.bits(sb[k][n][min(n_old, b.P):]) != 0).sum()) == 0, (it, N, screen, n)
        assert all(p.grad is None for p in b.params.values()) and b.optimizer.seg_steps == steps
        for t, shape in ((b.xyz_gradient_accum, (b.P, 1)), (b.denom, (b.P, 1)), (b.max_radii2D, (b.P,))):
            assert t.shape == shape and t.is_cuda and float(t.abs().sum()) == 0
        seen.add(tuple(c > 0 for c in ra))
    if P >= 70:
        assert (True, True, True, True) in seen and (True, True, True, False) in seen and (True, True, False, True) in seen


@pytest.mark.parametrize("P", fr.SIZES)
def test_spatial_order(hip, P):
    """The same model densified with and without the spatial order: the rows of the first are the rows of the second in Morton
    order of their centres (stable), bit for bit - and the host path agrees on the discrete result."""
    for it, N, screen in CASES:
        flat_m, so, host = (fr.build_model(hip.api, DEV, P, spatial_order=True) for _ in range(3))
        flat_m.spatial_order = False          # the same rows, re-laid out in the reference order
        (r0, _), (r1, _) = fr.run_model(flat_m, it, N, screen, on_device=True), fr.run_model(so, it, N, screen, on_device=True)
        rh, _ = fr.run_model(host, it, N, screen)
        assert r0 == r1 == rh and flat_m.P == so.P == host.P > 0
        perm = synthetic.morton_order(flat_m.params["xyz"]).cpu()
        want = tuple({n: v[perm] for n, v in part.items()} for part in fr.snapshot(flat_m))
        assert_same_model(fr.snapshot(so), want, None, ("spatial order", it, N, screen))
        xyz = so.params["xyz"].detach()
        assert torch.equal(xyz, xyz[synthetic.morton_order(xyz)])


@pytest.mark.parametrize("P", fr.SIZES)
def test_against_the_cpu_run_with_the_oracle_knn(hip, oracle, P):
    for it, N, screen in CASES:
        cpu, gpu = fr.build_model(oracle.api, "cpu", P), fr.build_model(hip.api, DEV, P)
        counts, computed = computed_rows(cpu, lambda x: dist2_with_indices(oracle.api, x), it, N, screen)
        (rc, _), (rg, _) = fr.run_model(cpu, it, N, screen), fr.run_model(gpu, it, N, screen, on_device=True)
        assert rc == rg == counts, (it, N, screen, rc, rg)
        assert_same_model(fr.snapshot(gpu), fr.snapshot(cpu), computed, ("cpu", it, N, screen))


def test_two_runs_give_the_same_bits(hip):
    runs = []
    for _ in range(2):
        m = fr.build_model(hip.api, DEV, 1031, spatial_order=True)
        res, _ = fr.run_model(m, 600, 3, 20, on_device=True)
        runs.append((res, fr.snapshot(m)))
    assert runs[0][0] == runs[1][0] and all(c > 0 for c in runs[0][0])
    assert_same_model(runs[0][1], runs[1][1], None, "determinism")


def test_fallbacks_take_the_host_path_with_one_draw(hip):
    """Fewer than 4 points in front of kNN #1, and every row pruned: on_device returns what the host path returns, the model is
    the host path's bit for bit and the generator has been drawn from exactly once (the same state as after the host run)."""
    def three(api):
        m = fr.build_model(api, DEV, 3)
        with torch.no_grad():
            m.params["scaling"][1] = -3.0       # wider than the extent: with infinite distances the distance rule splits it
        m.xyz_gradient_accum.zero_()            # no clones: kNN #1 would see 3 points
        return m
    a, b = three(hip.api), three(hip.api)
    (ra, ga), (rb, gb) = fr.run_model(a, 600, 2, None), fr.run_model(b, 600, 2, None, on_device=True)
    assert ra == rb and ra[0] == 0 and ra[1] > 0
    assert torch.equal(ga.get_state(), gb.get_state())
    assert not torch.equal(ga.get_state(), torch.Generator().manual_seed(77).get_state())
    assert_same_model(fr.snapshot(b), fr.snapshot(a), None, "three points")
    a, b = fr.build_model(hip.api, DEV, 70), fr.build_model(hip.api, DEV, 70)
    outs = []
    for m, flag in ((a, False), (b, True)):
        gen = torch.Generator().manual_seed(77)
        outs.append((m.densify_and_prune_fsgs(fr.MAX_GRAD, 2.0, fr.EXTENT, None, 600, generator=gen, on_device=flag), gen))
    assert outs[0][0] == outs[1][0] and a.P == b.P == 0 and outs[0][0][1] > 0
    assert torch.equal(outs[0][1].get_state(), outs[1][1].get_state())
    # percent_dense > 1: a clone could be split, which the device plan excludes
    a, b = fr.build_model(hip.api, DEV, 257), fr.build_model(hip.api, DEV, 257)
    a.percent_dense = b.percent_dense = 1.5
    (ra, ga), (rb, gb) = fr.run_model(a, 600, 2, None), fr.run_model(b, 600, 2, None, on_device=True)
    assert ra == rb and torch.equal(ga.get_state(), gb.get_state())
    assert_same_model(fr.snapshot(b), fr.snapshot(a), None, "percent_dense")


def test_abi_errors_touch_no_memory(hip):
    api = hip.api
    P, N = 300, 2
    assert api.raw("densify_fsgs_tmp_bytes")(0) == 0
    nbytes = api.raw("densify_fsgs_tmp_bytes")(P)
    assert nbytes >= 256 + P
    tmp = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    f = torch.zeros((P * 59,), device=DEV)
    out = torch.full((2 * P * 59,), 7.0, device=DEV)
    tab = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    kind = torch.full((P,), 0x5A, dtype=torch.uint8, device=DEV)
    p, o, t = f.data_ptr(), out.data_ptr(), tmp.data_ptr()
    widths = (C.c_int32 * 5)(3, 48, 1, 3, 4)
    NULL, SHAPE, SCRATCH = -1, -2, -3

    def plan(scaling=p, tmp_ptr=t, P_=P, N_=N, xyz1=o, nb=nbytes):
        return api.raw("densify_fsgs_plan")(scaling, p, p, p, p, P_, N_, 2e-4, 2e-4, 0.005, 0.002, 0.02, 1.6, 0, tmp_ptr, nb, xyz1, None)

    def merge(dist=p, P_=P, nb=nbytes):
        return api.raw("densify_fsgs_merge")(t, nb, dist, P_, 0.2, 1, None)

    def emit(xyz=p, table=tab.data_ptr(), P_=P, N_=N, n_clone=0, n_split=0, n_stay=P, nQ=P, noise=None, nb=nbytes):
        return api.raw("densify_fsgs_emit")(t, nb, xyz, p, p, noise, P_, N_, n_clone, n_split, n_stay, nQ, 1, table, o, None)

    def prox_plan(table=tab.data_ptr(), dist=p, nearest=p, P_=P, nQ=P, nb=nbytes):
        return api.raw("densify_fsgs_prox_plan")(t, nbytes, P_, table, nQ, dist, nearest, 0.1, 1, t, nb, None)

    def final(table=tab.data_ptr(), nQ=P, n_keep=P, S=0, n_prox=0, P2=P, sel=None, nb=nbytes):
        return api.raw("densify_fsgs_final")(t, nb, p, p, p, nQ, n_keep, S, n_prox, P2, table, kind.data_ptr(), o, sel, sel, None)

    def gather(table=tab.data_ptr(), P_=P, P2=P, nfields=5, rotation_field=4):
        return api.raw("densify_fsgs_gather")(None, table, kind.data_ptr(), p, P2, p, p, p, P_, o, o, o, nfields, widths, 0, 3, 2,
                                              rotation_field, 1.6, None)

    assert plan(scaling=None) == NULL and plan(tmp_ptr=None) == NULL and plan(xyz1=None) == NULL
    assert plan(P_=0) == SHAPE and plan(N_=0) == SHAPE and plan(N_=9) == SHAPE and plan(nb=nbytes - 1) == SCRATCH
    assert merge(dist=None) == NULL and merge(P_=0) == SHAPE and merge(nb=nbytes - 1) == SCRATCH
    assert emit(xyz=None) == NULL and emit(table=None) == NULL and emit(P_=0) == SHAPE and emit(N_=9) == SHAPE
    assert emit(nQ=P + 1) == SHAPE and emit(n_split=1, n_stay=P, nQ=P + 2) == SHAPE     # (prune on: a split row does not stay)
    assert emit(n_split=1, n_stay=P - 1, nQ=P + 1) == NULL and emit(nb=nbytes - 1) == SCRATCH   # rows split, no noise
    assert prox_plan(table=None) == NULL and prox_plan(nearest=None) == NULL and prox_plan(nQ=0) == SHAPE
    assert prox_plan(nb=nbytes - 1) == SCRATCH
    assert final(table=None) == NULL and final(P2=P + 1) == SHAPE and final(n_keep=P + 1, P2=P + 1) == SHAPE
    assert final(S=1, n_prox=4, P2=P + 4, sel=p) == SHAPE and final(S=1, n_prox=1, P2=P + 1) == NULL
    assert final(nb=nbytes - 1) == SCRATCH
    assert gather(table=None) == NULL and gather(P_=0) == SHAPE and gather(P2=0) == SHAPE and gather(nfields=9) == SHAPE
    assert gather(rotation_field=3) == SHAPE and gather(rotation_field=5) == SHAPE      # coincides with scaling / out of range
    torch.cuda.synchronize()
    assert int((tmp != 0x5A).sum()) == 0 and int((out != 7.0).sum()) == 0 and int((tab != -1).sum()) == 0
    assert int((kind != 0x5A).sum()) == 0


GATHER_P, PROXIMITY = 257, 3
MODEL_WIDTHS, ODD_WIDTHS = (3, 48, 1, 3, 4), (3, 5, 1, 3, 4)   # (5: no constant-width instantiation, the run-time width)
SENTINEL = 0x7FC12345                                          # a NaN no gather computes or copies


def run_both_gathers(hip, P2, with_perm, widths, prox_at=None):
    """gs_densify_gather and gs_densify_fsgs_gather (all-zero nb_kind) on one table of P2 entries over GATHER_P source rows, from
    CPU generators -> the two (flat, exp_avg, exp_avg_sq) triples as int32 bits [P2 * sum(widths)], and the permutation."""
    api, P, W = hip.api, GATHER_P, sum(widths)
    g = torch.Generator().manual_seed(1000 * P2 + len(widths) + 7 * with_perm)
    old = [torch.randn((P * W,), generator=g).to(DEV) for _ in range(3)]
    src = torch.randint(0, P, (P2,), generator=g)
    kind = torch.randint(0, PROXIMITY, (P2,), generator=g)            # survivor, clone, sample
    if P2 >= 3:
        kind[:3] = torch.arange(3)                                    # (each of them at least once)
    if prox_at is not None:
        kind[prox_at] = PROXIMITY
    entry = src | (kind << 30)
    table = torch.where(entry >= 2 ** 31, entry - 2 ** 32, entry).to(torch.int32).to(DEV)   # (the uint32's bits)
    new_xyz = torch.randn((P2, 3), generator=g).to(DEV)
    perm = torch.randperm(P2, generator=g).to(DEV) if with_perm else None
    nb_kind = torch.zeros((P2,), dtype=torch.uint8, device=DEV)
    cw = (C.c_int32 * len(widths))(*widths)
    outs = []
    for entry in ("densify_gather", "densify_fsgs_gather"):
        new = [torch.full((P2 * W,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)]
        lead = [None if perm is None else perm.data_ptr(), table.data_ptr()]
        tail = [0, 3]
        if entry == "densify_fsgs_gather":
            lead.append(nb_kind.data_ptr())
            tail += [2, 4]
        rc = api.raw(entry)(*lead, new_xyz.data_ptr(), P2, old[0].data_ptr(), old[1].data_ptr(), old[2].data_ptr(), P,
                            new[0].data_ptr(), new[1].data_ptr(), new[2].data_ptr(), len(widths), cw, *tail, 1.6, None)
        assert rc == 0, (entry, rc)
        outs.append(new)
    torch.cuda.synchronize()
    return outs[0], outs[1], perm


def rows_of(buf, P2, widths):
    """[P2, sum(widths)]: the field-major buffer's rows side by side."""
    parts, off = [], 0
    for w in widths:
        parts.append(buf[off:off + P2 * w].view(P2, w))
        off += P2 * w
    return torch.cat(parts, dim=1)


@pytest.mark.parametrize("widths", (MODEL_WIDTHS, ODD_WIDTHS))
@pytest.mark.parametrize("with_perm", (False, True))
@pytest.mark.parametrize("P2", (1, 255, 257))
def test_the_two_gathers_are_one_kernel_body(hip, P2, with_perm, widths):
    """A table of survivors, clones and samples only: both entry points write the same bytes into parameters and both moments,
    and every one of them."""
    plain, fsgs, _ = run_both_gathers(hip, P2, with_perm, widths)
    for a, b in zip(plain, fsgs):
        assert torch.equal(a, b) and int((a == SENTINEL).sum()) == 0


def test_only_the_fsgs_gather_writes_a_proximity_row(hip):
    """One GS_DENSIFY_PROXIMITY entry: gs_densify_gather, which has no neighbour kinds, drops it - that output row keeps its
    sentinel in every field of all three buffers - and gs_densify_fsgs_gather writes the row; the other rows are the same."""
    P2, at = 257, 100
    plain, fsgs, perm = run_both_gathers(hip, P2, True, MODEL_WIDTHS, prox_at=at)
    row = int((perm == at).nonzero())
    others = torch.arange(P2, device=DEV) != row
    for a, b in zip(plain, fsgs):
        a, b = rows_of(a, P2, MODEL_WIDTHS), rows_of(b, P2, MODEL_WIDTHS)
        assert torch.equal(a[others], b[others]) and int((a[others] == SENTINEL).sum()) == 0
        assert int((a[row] != SENTINEL).sum()) == 0 and int((b[row] == SENTINEL).sum()) == 0


def conditions_hold(hip, m, it, N=2, screen=None, **kw):
    """The input conditions of tests/test_fsgs_densify_cpu.py on a model the CPU test cannot rebuild (a trained one)."""
    state = fr.snapshot(m)
    gen = torch.Generator()
    gen.set_state(kw["generator"].get_state())     # the same noise as the run it stands in front of
    _, _, info = fr.densify_and_prune(state, m.xyz_gradient_accum.cpu().clone(), m.denom.cpu().clone(), hip_knn(hip),
                                      kw["max_grad"], kw["min_opacity"], kw["extent"], screen, it,
                                      gen, N=N, dist_thres=kw["dist_thres"],
                                      prune_from_iter=kw["prune_from_iter"], proximity_until_iter=kw["proximity_until_iter"],
                                      percent_dense=m.percent_dense)
    return info


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
    """Clone / prune only (percent_dense = 1 with an extent above every scale: nothing is large, nothing is computed): the two
    models are the same bits, and stay so through the next fused step."""
    a, b = make_trainer(hip), make_trainer(hip)
    kw = dict(dist_thres=10.0, prune_from_iter=500, proximity_until_iter=2000)
    for tr in (a, b):
        for k in range(3):
            tr.step(k)
        tr.sync()
        tr.gather_optimizer_state()
        tr.model.percent_dense = 1.0
    ra = a.model.densify_and_prune_fsgs(1e-7, 0.005, 1e3, None, 600, generator=torch.Generator().manual_seed(1), **kw)
    rb = b.model.densify_and_prune_fsgs(1e-7, 0.005, 1e3, None, 600, generator=torch.Generator().manual_seed(1), on_device=True, **kw)
    assert ra == rb and ra[0] > 0 and ra[1] == 0 and a.model.P == b.model.P
    assert_same_model(fr.snapshot(b.model), fr.snapshot(a.model), None, "before the step")
    for tr in (a, b):
        tr.step(3)
        tr.sync()
    torch.cuda.synchronize()
    assert a.last["path"] == b.last["path"] == "manual"
    assert torch.equal(a.model.flat, b.model.flat)
    assert torch.equal(a.model.optimizer.exp_avg, b.model.optimizer.exp_avg)
    assert torch.equal(a.model.optimizer.exp_avg_sq, b.model.optimizer.exp_avg_sq)


def test_train_iteration_with_the_fsgs_rule_on_the_device(hip):
    """densify_rule = "fsgs" through train_iteration across the first densifying iteration, with densify_on_device on and off: the
    same 4-tuple and row count, the models equal at the bars above, and training goes on.  The model is a trained one, so the
    input conditions are asserted on it in front of the densification."""
    runs = []
    # (against the trained scene's scales, 0.3 .. 2.2, and mean squared distances, 0.03 .. 0.2: both distance rules select
    # some rows and not all; nothing is small enough to be cloned)
    extent, thr = 0.015, dict(dist_thres=8.0, prune_from_iter=2, proximity_until_iter=100)
    for flag in (False, True):
        tr = make_trainer(hip)
        seen = {}
        inner = tr.model.densify_and_prune_fsgs

        def checked(max_grad, min_opacity, ext, screen, it, *, _inner=inner, _m=tr.model, _seen=seen, **kw):
            info = conditions_hold(hip, _m, it, screen=screen, max_grad=max_grad, min_opacity=min_opacity, extent=ext,
                                   generator=kw["generator"], **{k: kw[k] for k in thr})
            assert fr.neighbours_are_separated(info["knn1"]) and fr.neighbours_are_separated(info["knn2"])
            assert fr.smallest_margin(info, _m.xyz_gradient_accum.cpu(), _m.denom.cpu(), 2, screen, _m.percent_dense, ext,
                                      kw["dist_thres"], max_grad, min_opacity, constructed=False) > 1e-5
            _seen.update(computed=info["computed"], splits=int(info["dist_split"].sum()), prox=int(info["proximity"].sum()))
            return _inner(max_grad, min_opacity, ext, screen, it, **kw)
        tr.model.densify_and_prune_fsgs = checked
        opt = TrainOptions(iterations=40, densify_from_iter=3, densification_interval=4, opacity_reset_interval=100,
                           densify_until_iter=30, cameras_extent=extent, densify_grad_threshold=1e-7, seed=3,
                           densify_rule="fsgs", densify_on_device=flag, **thr)
        tr.model.active_sh_degree = 0
        log = [tr.train_iteration(it, opt) for it in range(1, 5)]
        snap = fr.snapshot(tr.model)
        log += [tr.train_iteration(it, opt) for it in range(5, 7)]
        tr.sync()
        runs.append((log, snap, seen))
    (off, snap_off, seen), (on, snap_on, _) = runs
    assert [o["densified"] is not None for o in on] == [False, False, False, True, False, False]
    assert on[3]["densified"] == off[3]["densified"] and len(on[3]["densified"]) == 4 and on[3]["P"] == off[3]["P"]
    assert all(c > 0 for c in on[3]["densified"][1:]) and 0 < seen["splits"] and 0 < seen["prox"]
    assert_same_model(snap_on, snap_off, seen["computed"], "after the densification")
    assert all(o["P"] == on[3]["P"] and torch.isfinite(torch.as_tensor(o["loss"])) for o in on[4:])

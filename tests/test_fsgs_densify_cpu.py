"""FSGS's densification without a GPU: GaussianModelLite.densify_and_prune_fsgs's host path (the oracle's kNN) against the
literal restatement of the reference's sequence (tests/fsgs_densify_reference.py), bit for bit - parameters, both Adam moments
and the row order -, and the conditions on the shared inputs that let tests/test_gpu_fsgs_densify.py demand equal discrete
results of the HIP kernels: every decision decisive, every neighbour list unambiguous, every rule selecting something."""
import os
import re

import pytest
import torch

import fsgs_densify_reference as fr
from gsplat_amd import synthetic
from gsplat_amd.knn import dist2_with_indices
from gsplat_amd.trainer import GaussianModelLite, TrainOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("densify_fsgs_tmp_bytes", "densify_fsgs_plan", "densify_fsgs_merge", "densify_fsgs_emit", "densify_fsgs_prox_plan",
               "densify_fsgs_final", "densify_fsgs_gather")
GRID = [(it, N, screen, so) for it in fr.ITERATIONS for N in fr.NS for screen in fr.SCREENS for so in (False, True)]


def knn_of(oracle):
    return lambda xyz: dist2_with_indices(oracle.api, xyz)


def ordered(state, spatial_order):
    if not spatial_order or state[0]["xyz"].shape[0] == 0:
        return state
    perm = synthetic.morton_order(state[0]["xyz"])
    return tuple({k: v[perm] for k, v in part.items()} for part in state)


@pytest.mark.parametrize("P", fr.SIZES)
def test_the_host_path_is_the_restatement_bit_for_bit(oracle, P):
    for it, N, screen, so in GRID:
        m = fr.build_model(oracle.api, "cpu", P, spatial_order=so)
        want, counts, info = fr.run_reference(m, knn_of(oracle), it, N, screen)
        want = ordered(want, so)
        generation = m.generation
        got_counts, _ = fr.run_model(m, it, N, screen)
        assert got_counts == counts, (it, N, screen, so)
        assert m.P == want[0]["xyz"].shape[0] and m.generation > generation
        got = fr.snapshot(m)
        for part_got, part_want in zip(got, want):
            for k in part_want:
                assert torch.equal(fr.bits(part_got[k]), fr.bits(part_want[k])), (it, N, screen, so, k)
        if it <= fr.PRUNE_FROM:   # no prune at all: the split originals stay, nothing is counted as pruned
            assert counts[3] == 0 and m.P == P + counts[0] + N * counts[1] + counts[2]
        if it >= fr.PROX_UNTIL:
            assert counts[2] == 0 and "proximity" not in info
        for stat, shape in ((m.xyz_gradient_accum, (m.P, 1)), (m.denom, (m.P, 1)), (m.max_radii2D, (m.P,))):
            assert tuple(stat.shape) == shape and not stat.any()
        assert all(p.grad is None for p in m.params.values())
        if so and m.P:
            xyz = m.params["xyz"].detach()
            assert torch.equal(synthetic.morton_order(xyz), torch.arange(m.P))


def test_the_shared_inputs_meet_the_conditions_of_the_gpu_tests(oracle):
    """On exactly what tests/test_gpu_fsgs_densify.py uses (fr.build_model at every size, with and without the spatial order,
    over the whole case grid, noise seed 77): (1) every discrete decision - both distance rules, both scale rules, the
    statistic, the opacity, the world-size rule - is more than 1e-5 relative (about 100 fp32 ulps) from its threshold; (2) for
    every row of both kNN point sets the 1st .. 4th neighbour distances are more than 1e-5 relative apart, or the tied
    points carry identical centre, scaling and opacity; (3) at every size >= 70 each of clone, grad-split, distance-split-only,
    proximity and faint selects at least one row and not all."""
    worst = float("inf")
    for P in fr.SIZES:
        for it, N, screen, so in GRID:
            m = fr.build_model(oracle.api, "cpu", P, spatial_order=so)
            _, counts, info = fr.run_reference(m, knn_of(oracle), it, N, screen)
            worst = min(worst, fr.smallest_margin(info, m.xyz_gradient_accum, m.denom, N, screen, m.percent_dense))
            assert fr.neighbours_are_separated(info["knn1"]), (P, it, N, screen, so)
            assert "knn2" not in info or fr.neighbours_are_separated(info["knn2"]), (P, it, N, screen, so)
            if P >= 70:
                rules = dict(clone=info["clone"], grad_split=info["grad_split"],
                             dist_split_only=info["dist_split"] & ~info["grad_split"], faint=info["faint"])
                if "proximity" in info:
                    rules["proximity"] = info["proximity"]
                for name, mask in rules.items():
                    assert 0 < int(mask.sum()) < mask.numel(), (P, it, N, screen, so, name)
    print("smallest relative margin %.3e" % worst)
    assert worst > 1e-5


def test_constructed_rows_and_the_empty_block(oracle):
    """x / 0 = inf is selected, 0 / 0 -> 0 is not; the clone rule looks at |g|, the split rule at g; g == float32(max_grad) is
    selected (>=), the fp32 below is not; and no rule selects a row of the empty block of the five-block model."""
    m = fr.build_model(oracle.api, "cpu", 1031)
    _, _, info = fr.run_reference(m, knn_of(oracle), 600, 2, None)
    P = 1031
    clone, gs, ds = info["clone"], info["grad_split"][:P], info["dist_split"][:P]
    sel = clone | gs
    assert bool(sel[fr.ROW_INF]) and not bool(sel[fr.ROW_NAN])
    assert bool(clone[fr.ROW_NEG_SMALL]) and not bool(sel[fr.ROW_NEG_LARGE])
    assert bool(clone[fr.ROW_EXACT]) and not bool(sel[fr.ROW_BELOW])
    lo, hi = fr.EMPTY_BLOCK * 256, fr.EMPTY_BLOCK * 256 + 256
    assert not bool((sel | ds)[lo:hi].any())
    for b in range(5):
        if b != fr.EMPTY_BLOCK:
            assert bool(sel[b * 256]) and bool(sel[min(b * 256 + 255, P - 1)]), b
    assert not bool(info["dist_split"][P:].any()) and not bool(info["grad_split"][P:].any())   # a clone is never split


def test_proximity_inside_the_call_reproduces_the_tiling(oracle):
    """With S > 1 selected rows, new row j lies midway between neighbour j of the flattened lists and selected row j % S - so
    some new row is NOT between a Gaussian and its own neighbour."""
    m = fr.build_model(oracle.api, "cpu", 257)
    state, counts, info = fr.run_reference(m, knn_of(oracle), 400, 2, None)   # (no prune: every new row is still there)
    k2, rows = info["knn2"], info["proximity"].nonzero().squeeze(1)
    S, nQ = int(rows.numel()), info["knn2"]["xyz"].shape[0]
    assert S > 1 and counts[2] == 3 * S
    fr.run_model(m, 400, 2, None)
    new = m.params["xyz"].detach()[nQ:nQ + 3 * S]
    own = 0
    for j in range(3 * S):
        nb = k2["nearest"][rows[j // 3], j % 3].long()
        assert torch.equal(new[j], (k2["xyz"][rows[j % S]] + k2["xyz"][nb]) / 2)
        own += int(torch.equal(new[j], (k2["xyz"][rows[j // 3]] + k2["xyz"][nb]) / 2))
    assert own < 3 * S


@pytest.mark.parametrize("spatial_order", (False, True))
@pytest.mark.parametrize("S", (1, 3))
def test_proximity_alone_is_the_proximity_stage_of_the_call(oracle, S, spatial_order):
    """proximity() and densify_and_prune_fsgs with nothing to clone (statistic 0 against max_grad 1), nothing to split (the
    distance rule's bound out of reach) and no prune (iteration <= prune_from_iter) append the same rows, bit for bit: with one
    selected row and with three, the tiling case.  The extent is placed midway between the S-th and the (S+1)-th largest of the
    rows' min(dist / 5, max scale), so exactly S rows pass both of the rule's comparisons."""
    a, b = (fr.build_model(oracle.api, "cpu", 257, spatial_order=spatial_order) for _ in range(2))
    for m in (a, b):
        m.xyz_gradient_accum.zero_()
        m.denom.fill_(1.0)
    dist, _ = dist2_with_indices(oracle.api, a.params["xyz"].detach())
    v = torch.minimum(dist / 5, a.get_scaling.detach().max(dim=1).values).sort(descending=True).values
    assert float(v[S - 1]) > float(v[S]) * (1 + 1e-3)
    extent = (float(v[S - 1]) + float(v[S])) / 2
    gen = torch.Generator().manual_seed(77)
    n = a.proximity(extent)
    counts = b.densify_and_prune_fsgs(1.0, 0.0, extent, None, 400, dist_thres=1e6, prune_from_iter=500, proximity_until_iter=2000,
                                      generator=gen)
    assert counts == (0, 0, n, 0) and n == 3 * S and a.P == b.P == 257 + n
    assert torch.equal(gen.get_state(), torch.Generator().manual_seed(77).get_state())
    for part_a, part_b in zip(fr.snapshot(a), fr.snapshot(b)):
        for k in part_a:
            assert torch.equal(fr.bits(part_a[k]), fr.bits(part_b[k])), k


def test_with_nir_raises(oracle):
    m = GaussianModelLite(synthetic.trained_like(64, seed=0), torch.device("cpu"), api=oracle.api, with_nir=True)
    with pytest.raises(NotImplementedError):
        m.densify_and_prune_fsgs(fr.MAX_GRAD, fr.MIN_OPACITY, fr.EXTENT, None, 600)


def test_on_device_on_a_cpu_model_raises(oracle):
    m = fr.build_model(oracle.api, "cpu", 70)
    before = m.flat.clone()
    with pytest.raises(RuntimeError, match="no fallback"):
        m.densify_and_prune_fsgs(fr.MAX_GRAD, fr.MIN_OPACITY, fr.EXTENT, None, 600, on_device=True)
    assert m.P == 70 and torch.equal(m.flat, before)
    plain = GaussianModelLite(fr._scene(70, 3), torch.device("cpu"))   # torch Adam: no flat state either
    with pytest.raises(RuntimeError, match="no fallback"):
        plain.densify_and_prune_fsgs(fr.MAX_GRAD, fr.MIN_OPACITY, fr.EXTENT, None, 600, on_device=True)


def test_train_iteration_takes_the_fsgs_rule_on_schedule(oracle):
    """densify_rule = "fsgs" through Trainer.train_iteration on a CPU model: on densifying iterations the new method is called
    with max_screen_size None, the iteration, the options' thresholds and the per-iteration generator seed; `densified` is its
    4-tuple.  The default rule still calls densify_and_prune."""
    from test_trainer_cpu import make_trainer
    from gsplat_amd.trainer import cameras_extent
    log = {}
    for rule in ("fsgs", "3dgs"):
        tr = make_trainer(oracle, P=60, W=48, H=40, dwt=False)
        model, cams = tr.model, tr.cameras
        calls = []
        for name in ("densify_and_prune_fsgs", "densify_and_prune"):
            def spy(*a, _inner=getattr(model, name), _name=name, **kw):
                calls.append((_name, a, {k: v for k, v in kw.items() if k != "generator"}, kw["generator"].initial_seed()))
                return _inner(*a, **kw)
            setattr(model, name, spy)
        opt = TrainOptions(iterations=20, densify_from_iter=2, densification_interval=3, opacity_reset_interval=100,
                           densify_until_iter=12, cameras_extent=cameras_extent([c.camera_center for c in cams]),
                           densify_grad_threshold=1e-7, seed=3, densify_rule=rule, prune_from_iter=4, proximity_until_iter=8,
                           dist_thres=2.5)
        model.active_sh_degree = 0
        out = [tr.train_iteration(it, opt) for it in range(1, 11)]
        log[rule] = (calls, out, model.P)
    calls, out, final_P = log["fsgs"]
    assert [c[0] for c in calls] == ["densify_and_prune_fsgs"] * 3
    for (name, a, kw, seed), it in zip(calls, (3, 6, 9)):
        assert a == (1e-7, 0.005, opt.cameras_extent, None, it) and seed == 3 * 1000003 + it
        assert kw == dict(dist_thres=2.5, prune_from_iter=4, proximity_until_iter=8, on_device=False)
    dens = [o["densified"] for o in out]
    assert [d is not None for d in dens] == [it in (3, 6, 9) for it in range(1, 11)]
    assert all(len(d) == 4 for d in dens if d is not None)
    assert dens[2][3] == 0 and dens[8][2] == 0       # iteration 3: no prune yet; iteration 9: proximity is over
    assert out[-1]["P"] == final_P > 60
    calls, out, _ = log["3dgs"]
    assert [c[0] for c in calls] == ["densify_and_prune"] * 3
    assert all(len(o["densified"]) == 3 for o in out if o["densified"] is not None)
    with pytest.raises(TypeError):
        TrainOptions(densify_rules="fsgs")


def test_the_default_options_leave_the_3dgs_rule():
    o = TrainOptions()
    assert (o.densify_rule, o.dist_thres, o.prune_from_iter, o.proximity_until_iter) == ("3dgs", 10.0, 500, 2000)


def test_the_new_entry_points_are_declared_everywhere():
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert name in PROTOTYPES and name in DEVICE_ONLY, name
        decl = re.search(r"\bgs_%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(PROTOTYPES[name][1]), name    # one ctypes argument per C parameter
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)
    for flag, value in (("GS_DENSIFY_PROXIMITY", 3), ("GS_DENSIFY_FSGS_CLONE", 1), ("GS_DENSIFY_FSGS_GRAD_SPLIT", 2),
                        ("GS_DENSIFY_FSGS_SPLIT", 4), ("GS_DENSIFY_FSGS_PRUNE_SELF", 8), ("GS_DENSIFY_FSGS_PRUNE_SAMPLE", 16),
                        ("GS_DENSIFY_FSGS_WIDE_SELF", 32), ("GS_DENSIFY_FSGS_WIDE_SAMPLE", 64), ("GS_DENSIFY_FSGS_MERGE_AT", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), header), flag

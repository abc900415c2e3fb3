"""gsplat_amd/cli.py without a GPU: its parser against the reference parser's record (tests/golden/lgdwt_args.json), cfg_args
written and read back without eval, and the flags the Trainer cannot honour."""
import argparse
import json
import os

import pytest

from gsplat_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "lgdwt_args.json")))
GROUP_FLAGS = [(g, f["name"]) for g in ("ModelParams", "PipelineParams", "OptimizationParams") for f in RECORD[g]]


def actions_of(command):
    sub = next(a for a in cli.build_parser()._actions if isinstance(a, argparse._SubParsersAction))
    return {a.dest: a for a in sub.choices[command]._actions if not any(s.startswith("--no-") for s in a.option_strings)}


def test_the_record_is_complete():
    assert (len(RECORD["ModelParams"]), len(RECORD["PipelineParams"]), len(RECORD["OptimizationParams"])) == (12, 4, 40)
    for g, flags in cli.GROUPS.items():
        assert [f[0] for f in flags] == [f["name"] for f in RECORD[g]], g


@pytest.mark.parametrize("group,name", GROUP_FLAGS)
def test_train_parser_has_the_references_flag(group, name):
    rec = next(f for f in RECORD[group] if f["name"] == name)
    a = actions_of("train")[name]
    assert "--" + name in a.option_strings
    shorts = [s[1:] for s in a.option_strings if not s.startswith("--")]
    assert shorts == ([rec["shorthand"]] if rec["shorthand"] else [])
    if rec["type"] == "bool":
        assert isinstance(a, argparse._StoreTrueAction)
    else:
        assert a.type.__name__ == rec["type"]
    assert a.default == rec["default"] and type(a.default) is type(rec["default"])
    if group != "OptimizationParams":   # render.py takes the loading and pipeline groups, the loading one with None defaults
        r = actions_of("render")[name]
        assert r.option_strings == a.option_strings and r.default == (None if group == "ModelParams" else rec["default"])


def test_the_scripts_own_flags():
    tr, rd = actions_of("train"), actions_of("render")
    for rec in RECORD["train"]:
        if rec["name"] in ("test_iterations", "save_iterations", "quiet", "start_checkpoint"):
            a = tr[rec["name"]]
            assert a.default == rec["default"]
            if rec["type"] == "bool":
                assert isinstance(a, argparse._StoreTrueAction)
            else:
                assert a.type.__name__ == rec["type"] and a.nargs == rec["nargs"]
    for rec in RECORD["render"]:
        a = rd[rec["name"]]
        assert a.default == rec["default"]
        assert isinstance(a, argparse._StoreTrueAction) if rec["type"] == "bool" else a.type.__name__ == rec["type"]
    me = actions_of("metrics")
    assert me["model_paths"].option_strings == ["--model_paths", "-m"] and me["model_paths"].required


def test_true_defaults_have_a_twin_and_method_3dgs_is_both_off():
    p = cli.build_parser()
    a = p.parse_args(["train", "-s", "x"])
    assert a.dwt_enable is True and a.patch_dwt_enable is True and a.method == "lgdwt" and a.seed == 0
    a = p.parse_args(["train", "-s", "x", "--no-dwt_enable"])
    assert a.dwt_enable is False and a.patch_dwt_enable is True
    a = p.parse_args(["train", "-s", "x", "--no-patch_dwt_enable", "--dwt_enable"])
    assert a.dwt_enable is True and a.patch_dwt_enable is False
    a = p.parse_args(["train", "-s", "x", "-m", "out", "-r", "2", "-w", "--eval", "--iterations", "60", "--test_iterations", "7", "9"])
    assert (a.source_path, a.model_path, a.resolution, a.white_background, a.eval, a.iterations) == ("x", "out", 2, True, True, 60)
    assert a.test_iterations == [7, 9]
    with pytest.raises(SystemExit):
        p.parse_args(["train", "--method", "other"])


def test_cfg_args_round_trip_and_refusal(tmp_path):
    args = cli.build_parser().parse_args(["train", "-s", "/data/it's a \"scene\"", "-m", str(tmp_path), "-r", "4", "--eval",
                                          "--n_views", "3", "--point_cloud_type", "sparse"])
    dataset = cli.extract(args, cli.MODEL_FLAGS)
    text = cli.cfg_args_text(dataset)
    assert text.startswith("Namespace(") and list(vars(dataset)) == [f[0] for f in cli.MODEL_FLAGS]
    back = cli.parse_cfg_args(text)
    assert vars(back) == vars(dataset)
    assert all(type(v) is type(vars(dataset)[k]) for k, v in vars(back).items())
    # the render command merges the file with its own command line (None = not given)
    (tmp_path / "cfg_args").write_text(text)
    r = cli.build_parser().parse_args(["render", "-m", str(tmp_path), "--iteration", "7", "-r", "2"])
    full = cli.combined_args(r)
    assert (full.resolution, full.eval, full.n_views, full.iteration, full.source_path) == (2, True, 3, 7, dataset.source_path)
    # anything but literals is refused, and nothing of it runs
    marker = tmp_path / "ran"
    for bad in ("Namespace(a=open(%r, 'w'))" % str(marker), "Namespace(a=__import__('os').mkdir(%r))" % str(marker),
                "open(%r, 'w')" % str(marker), "Namespace(a=[x for x in (1,)])", "Namespace(1, 2)", "Namespace(**{'a': 1})",
                "Other(a=1)", "Namespace(a=b)", "Namespace(a=1) + 1", "Namespace(a=", "import os"):
        with pytest.raises(ValueError, match="cfg_args"):
            cli.parse_cfg_args(bad)
    assert not marker.exists()
    assert vars(cli.parse_cfg_args("Namespace(a=-1, b=[1, 2.5], c=None, d=True, e='x')")) == dict(a=-1, b=[1, 2.5], c=None, d=True, e="x")


def test_flags_the_trainer_cannot_honour_raise():
    p = cli.build_parser()
    cli.check_supported(p.parse_args(["train", "-s", "x"]))
    for extra, what in ((["--data_device", "cpu"], "data_device"), (["--feature_lr", "0.01"], "feature_lr"),
                        (["--position_lr_init", "0.1"], "position_lr_init"), (["--exposure_lr_final", "0.1"], "exposure_lr_final"),
                        (["--sh_degree", "2"], "sh_degree"), (["--convert_SHs_python"], "convert_SHs_python"),
                        (["--compute_cov3D_python"], "compute_cov3D_python"), (["--start_checkpoint", "c.pth"], "start_checkpoint"),
                        (["--optimizer_type", "lion"], "optimizer_type")):
        with pytest.raises(cli.UnsupportedFlag, match=what):
            cli.check_supported(p.parse_args(["train", "-s", "x"] + extra))
    # and what it can honour reaches TrainOptions
    a = p.parse_args(["train", "-s", "x", "--iterations", "60", "--densify_from_iter", "20", "--densification_interval", "10",
                      "--seed", "5", "--random_background", "-w"])
    opt = cli.options_from(a, 3.5)
    assert (opt.iterations, opt.densify_from_iter, opt.densification_interval, opt.seed, opt.cameras_extent) == (60, 20, 10, 5, 3.5)
    assert opt.random_background is True and opt.white_background is True and opt.densify_until_iter == 15_000

"""python -m gsplat_amd.cli {train,render,metrics} - the __main__ blocks of LGDWT-GS/train.py, render.py and metrics.py over
gsplat_amd.scene.Scene and gsplat_amd.trainer.Trainer; cli.main(argv) is the same from Python.

Flags: every flag of the reference's ModelParams, PipelineParams and OptimizationParams (arguments/__init__.py:47-122) under its
name, one-letter shorthand, type and default (the tables below; tests/golden/lgdwt_args.json holds the reference parser's own
record of them), train.py's --test_iterations, --save_iterations, --quiet, and:
  --no-dwt_enable, --no-patch_dwt_enable   the reference declares both as store_true flags whose default is True, so its
                          command line cannot turn them off; these can
  --method {lgdwt,3dgs}   3dgs = both of them off: the plain 3DGS loss
  --seed                  TrainOptions.seed: the camera draw, the densification noise, NeRF-synthetic's random points
A flag this Trainer cannot honour raises (UnsupportedFlag) instead of being ignored: learning rates other than the reference's
defaults (they are constants of gsplat_amd.trainer), a data_device that is not the GPU, sh_degree other than 3, the Python SH /
covariance paths, --start_checkpoint (Trainer.checkpoint() carries neither the iteration nor the camera stack).  dwt_weight is
accepted and unused, as in the reference's own loop (train.py never reads it).
cfg_args is written as the reference writes it - str(Namespace(...)) of the ModelParams - so that its render.py / metrics.py can
read a model directory made here; it is read back WITHOUT eval: parse_cfg_args accepts a Namespace(...) call whose arguments
are literals and refuses anything else unexecuted.
Out of scope here: the FSGS, DNGaussian and multispectral loops (TrainerFSGS, TrainerDNG*, TrainerNIR) - they need mono-depth
files, masks and readers of their own; they are the follow-up."""
import argparse
import ast
import os
import sys
import uuid

# (name, shorthand?, default): the type is the default's, a bool is a store_true flag - ParamGroup's rule
MODEL_FLAGS = (("sh_degree", False, 3), ("source_path", True, ""), ("model_path", True, ""), ("images", True, "images"),
               ("depths", True, ""), ("resolution", True, -1), ("white_background", True, False), ("train_test_exp", False, False),
               ("data_device", False, "cuda"), ("eval", False, False), ("n_views", False, 0), ("point_cloud_type", False, "dense"))
PIPELINE_FLAGS = (("convert_SHs_python", False, False), ("compute_cov3D_python", False, False), ("debug", False, False),
                  ("antialiasing", False, False))
OPTIMIZATION_FLAGS = (
    ("iterations", False, 30_000), ("position_lr_init", False, 0.00016), ("position_lr_final", False, 0.0000016),
    ("position_lr_delay_mult", False, 0.01), ("position_lr_max_steps", False, 30_000), ("feature_lr", False, 0.0025),
    ("opacity_lr", False, 0.025), ("scaling_lr", False, 0.005), ("rotation_lr", False, 0.001), ("exposure_lr_init", False, 0.01),
    ("exposure_lr_final", False, 0.001), ("exposure_lr_delay_steps", False, 0), ("exposure_lr_delay_mult", False, 0.0),
    ("percent_dense", False, 0.01), ("lambda_dssim", False, 0.2), ("densification_interval", False, 100),
    ("opacity_reset_interval", False, 3000), ("densify_from_iter", False, 500), ("densify_until_iter", False, 15_000),
    ("densify_grad_threshold", False, 0.0002), ("depth_l1_weight_init", False, 1.0), ("depth_l1_weight_final", False, 0.01),
    ("random_background", False, False), ("optimizer_type", False, "default"), ("dwt_enable", False, True),
    ("dwt_weight", False, 0.5), ("dwt_ll1_weight", False, 1.0), ("dwt_lh1_weight", False, 1.0), ("dwt_hl1_weight", False, 1.0),
    ("dwt_hh1_weight", False, 0.0), ("dwt_ll2_weight", False, 0.0), ("dwt_lh2_weight", False, 0.0), ("dwt_hl2_weight", False, 0.0),
    ("dwt_hh2_weight", False, 0.0), ("patch_dwt_enable", False, True), ("patch_dwt_weight", False, 0.1), ("patch_size", False, 128),
    ("patch_percentile", False, 0.2), ("patch_dwt_lh1_weight", False, 1.0), ("patch_dwt_hl1_weight", False, 1.0))
GROUPS = {"ModelParams": MODEL_FLAGS, "PipelineParams": PIPELINE_FLAGS, "OptimizationParams": OPTIMIZATION_FLAGS}
# what the Trainer holds as constants (gsplat_amd.trainer.LRS, GaussianModelLite.update_learning_rate)
FIXED = ("position_lr_init", "feature_lr", "opacity_lr", "scaling_lr", "rotation_lr", "exposure_lr_init", "exposure_lr_final",
         "exposure_lr_delay_steps", "exposure_lr_delay_mult")


class UnsupportedFlag(ValueError):
    pass


def add_group(parser, title, flags, fill_none=False):
    """ParamGroup.__init__ (arguments/__init__.py:20-38); fill_none: render.py's sentinel, every default None"""
    group = parser.add_argument_group(title)
    for name, short, default in flags:
        names = ["--" + name] + (["-" + name[0]] if short else [])
        value = None if fill_none else default
        if isinstance(default, bool):
            group.add_argument(*names, default=value, action="store_true")
            if default:   # a store_true flag that is already True: its twin turns it off
                group.add_argument("--no-" + name, dest=name, action="store_false", help="turn %s off" % name)
        else:
            group.add_argument(*names, default=value, type=type(default))
    return group


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gsplat_amd.cli", description="Train, render and score a scene on disk")
    sub = parser.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", description="Training script parameters")
    add_group(tr, "Loading Parameters", MODEL_FLAGS)
    add_group(tr, "Optimization Parameters", OPTIMIZATION_FLAGS)
    add_group(tr, "Pipeline Parameters", PIPELINE_FLAGS)
    tr.add_argument("--test_iterations", nargs="+", type=int, default=[7_000, 30_000])
    tr.add_argument("--save_iterations", nargs="+", type=int, default=[7_000, 30_000])
    tr.add_argument("--quiet", action="store_true")
    tr.add_argument("--start_checkpoint", type=str, default=None)
    tr.add_argument("--seed", type=int, default=0)
    tr.add_argument("--method", choices=("lgdwt", "3dgs"), default="lgdwt")
    rd = sub.add_parser("render", description="Testing script parameters")
    add_group(rd, "Loading Parameters", MODEL_FLAGS, fill_none=True)
    add_group(rd, "Pipeline Parameters", PIPELINE_FLAGS)
    rd.add_argument("--iteration", default=-1, type=int)
    rd.add_argument("--skip_train", action="store_true")
    rd.add_argument("--skip_test", action="store_true")
    rd.add_argument("--quiet", action="store_true")
    me = sub.add_parser("metrics", description="Score <model>/test/ours_*/{renders,gt}")
    me.add_argument("--model_paths", "-m", required=True, nargs="+", type=str, default=[])
    me.add_argument("--lpips_weights", nargs=2, metavar=("VGG16", "LIN"), default=None,
                    help="torchvision's vgg16 weights and the LPIPS lin weights: results then carry LPIPS")
    return parser


def extract(args, flags):
    """ParamGroup.extract: the group's fields of the parsed arguments, in the group's order"""
    return argparse.Namespace(**{name: getattr(args, name) for name, _, _ in flags if hasattr(args, name)})


# -------------------------------------------------------------------------------------------------------- cfg_args
def cfg_args_text(dataset):
    """What train.py:305-306 writes: str(Namespace(**vars(dataset)))"""
    return str(argparse.Namespace(**vars(dataset)))


def parse_cfg_args(text):
    """The Namespace(...) text of a cfg_args file -> Namespace, without eval: one call of the name Namespace with keyword
    arguments whose values are Python literals.  Anything else - another callee, positional arguments, a call or a name
    inside a value - raises ValueError, and nothing of the text is executed."""
    try:
        node = ast.parse(text.strip(), mode="eval").body
    except SyntaxError as e:
        raise ValueError("cfg_args: not a Namespace(...) expression (%s)" % e)
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "Namespace" and not node.args):
        raise ValueError("cfg_args: expected Namespace(name=literal, ...)")
    out = {}
    for kw in node.keywords:
        if kw.arg is None:
            raise ValueError("cfg_args: ** is not a literal")
        try:
            out[kw.arg] = ast.literal_eval(kw.value)
        except (ValueError, TypeError, SyntaxError):
            raise ValueError("cfg_args: the value of %s is not a literal" % kw.arg)
    return argparse.Namespace(**out)


def combined_args(args):
    """get_combined_args (arguments/__init__.py:125-145): cfg_args of the model directory, overridden by what the command line
    gave (its sentinel defaults are None)"""
    merged = {}
    if args.model_path:
        path = os.path.join(args.model_path, "cfg_args")
        if os.path.exists(path):
            with open(path) as fp:
                merged = dict(vars(parse_cfg_args(fp.read())))
    for k, v in vars(args).items():
        if v is not None:
            merged[k] = v
    for name, _, default in MODEL_FLAGS:   # (a model directory without cfg_args: the groups' defaults)
        merged.setdefault(name, default)
    return argparse.Namespace(**merged)


# -------------------------------------------------------------------------------------------------------- checks
def check_supported(args):
    for name, _, default in OPTIMIZATION_FLAGS:
        if name in FIXED and hasattr(args, name) and getattr(args, name) != default:
            raise UnsupportedFlag("--%s %r: this rate is a constant of gsplat_amd.trainer (%r), the Trainer cannot take another"
                                  % (name, getattr(args, name), default))
    if not str(args.data_device).startswith("cuda"):
        raise UnsupportedFlag("--data_device %s: the images live on the GPU the Trainer runs on" % args.data_device)
    if args.sh_degree != 3:
        raise UnsupportedFlag("--sh_degree %d: GaussianModelLite holds degree 3" % args.sh_degree)
    for name in ("convert_SHs_python", "compute_cov3D_python"):
        if getattr(args, name, False):
            raise UnsupportedFlag("--%s: colours and covariances are evaluated by the rasterizer's kernels" % name)
    if getattr(args, "start_checkpoint", None):
        raise UnsupportedFlag("--start_checkpoint: Trainer.checkpoint() carries neither the iteration nor the camera stack")
    if getattr(args, "optimizer_type", "default") not in ("default", "sparse_adam"):
        raise UnsupportedFlag("--optimizer_type %s: 'default' or 'sparse_adam'" % args.optimizer_type)


def _device(args):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("gsplat_amd.cli needs a GPU - there is no CPU path")
    return torch.device(args.data_device if str(args.data_device).startswith("cuda") else "cuda")


def criterion_from(args):
    import lgdwt_loss
    on = args.method != "3dgs"
    return lgdwt_loss.criterion(
        lambda_dssim=args.lambda_dssim, dwt_enable=bool(args.dwt_enable and on), patch_dwt_enable=bool(args.patch_dwt_enable and on),
        dwt_weights=(args.dwt_ll1_weight, args.dwt_lh1_weight, args.dwt_hl1_weight, args.dwt_hh1_weight, args.dwt_ll2_weight,
                     args.dwt_lh2_weight, args.dwt_hl2_weight, args.dwt_hh2_weight),
        patch_size=args.patch_size, patch_percentile=args.patch_percentile, patch_dwt_weight=args.patch_dwt_weight,
        patch_lh1_weight=args.patch_dwt_lh1_weight, patch_hl1_weight=args.patch_dwt_hl1_weight)


def options_from(args, cameras_extent, **kw):
    from .trainer import TrainOptions
    names = ("iterations", "position_lr_final", "position_lr_delay_mult", "position_lr_max_steps", "densification_interval",
             "opacity_reset_interval", "densify_from_iter", "densify_until_iter", "densify_grad_threshold", "depth_l1_weight_init",
             "depth_l1_weight_final", "optimizer_type", "white_background", "random_background", "seed")
    return TrainOptions(cameras_extent=cameras_extent, **dict({n: getattr(args, n) for n in names}, **kw))


def trainer_from(args, scene, device):
    """The Trainer of train.py's loop over a loaded Scene -> (trainer, options)"""
    import diff_gaussian_rasterization as dgr
    import torch
    from .trainer import Trainer
    model = scene.model
    model.percent_dense = args.percent_dense
    if args.train_test_exp:
        model.enable_exposure(len(scene.train_cameras[1.0]))
    bg = torch.tensor([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    trainer = Trainer(model, scene.train_cameras[1.0], scene.gt_images[1.0], criterion_from(args), dgr.GaussianRasterizer,
                      dgr.GaussianRasterizationSettings, bg, optimizer_type=args.optimizer_type,
                      alpha_masks=scene.alpha_masks[1.0] if scene.masked else None)
    if args.depths:
        scene.load_depth_priors(trainer)
    return trainer, options_from(args, scene.cameras_extent)


def report(trainer, scene, iteration, out=print):
    """training_report (train.py:323-346): L1 / PSNR over the test cameras and over five training cameras.  (With
    train_test_exp the reference scores the right half of each image; the figures here are over the whole image.)"""
    n = len(scene.train_cameras[1.0])
    pick = [idx % n for idx in range(5, 30, 5)]
    configs = (("test", scene.test_cameras[1.0], scene.test_gt_images[1.0]),
               ("train", [scene.train_cameras[1.0][i] for i in pick], [scene.gt_images[1.0][i] for i in pick]))
    lines = []
    for name, cams, gts in configs:
        if cams:
            res = trainer.evaluate(cams, gts, quantise=False, clamp=True)
            lines.append("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, name, res["L1"], res["PSNR"]))
            out(lines[-1])
    return lines


# -------------------------------------------------------------------------------------------------------- commands
def train(args):
    from ._lib import hip_api
    from .scene import Scene
    check_supported(args)
    if args.antialiasing or args.debug:
        raise UnsupportedFlag("--antialiasing / --debug: the Trainer's step renders without them")
    device = _device(args)
    args.save_iterations = list(args.save_iterations) + [args.iterations]
    if not args.model_path:
        args.model_path = os.path.join("./output/", str(uuid.uuid4())[0:10])
    say = (lambda *a, **k: None) if args.quiet else print
    say("Optimizing " + args.model_path)
    os.makedirs(args.model_path, exist_ok=True)
    dataset = extract(args, MODEL_FLAGS)
    dataset.source_path = os.path.abspath(dataset.source_path)
    with open(os.path.join(args.model_path, "cfg_args"), "w") as fp:
        fp.write(cfg_args_text(dataset))
    dataset.seed = args.seed
    scene = Scene(dataset, device, api=hip_api())
    trainer, opt = trainer_from(args, scene, device)
    last = None
    for iteration in range(1, opt.iterations + 1):
        last = trainer.train_iteration(iteration, opt)
        if iteration in args.test_iterations:
            report(trainer, scene, iteration, out=say)
        if iteration in args.save_iterations:
            trainer.sync()
            say("\n[ITER {}] Saving Gaussians".format(iteration))
            scene.save(iteration)
    trainer.sync()
    say("\nTraining complete.")
    return dict(scene=scene, trainer=trainer, options=opt, last=last)


def render_sets(args):
    import diff_gaussian_rasterization as dgr
    import torch
    from ._lib import hip_api
    from .render_set import write_render_set
    from .scene import Scene
    from .trainer import render
    full = combined_args(args)
    check_supported(full)
    device = _device(full)
    say = (lambda *a, **k: None) if args.quiet else print
    say("Rendering " + full.model_path)
    dataset = extract(full, MODEL_FLAGS)
    scene = Scene(dataset, device, api=hip_api(), load_iteration=args.iteration)
    bg = torch.tensor([1.0, 1.0, 1.0] if dataset.white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    out = {}
    sets = (("train", args.skip_train, scene.train_cameras[1.0], scene.gt_images[1.0]),
            ("test", args.skip_test, scene.test_cameras[1.0], scene.test_gt_images[1.0]))
    for name, skip, cams, gts in sets:
        if skip or not cams:
            continue

        def views():
            with torch.no_grad():
                for cam, gt in zip(cams, gts):
                    img = render(cam, scene.model, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg, clamp=False,
                                 antialiasing=bool(full.antialiasing), debug=bool(full.debug))["render"]
                    if dataset.train_test_exp:   # render.py:40-42: the half the test set scores
                        img, gt = img[..., img.shape[-1] // 2:], gt[..., gt.shape[-1] // 2:]
                    yield {"render": img, "gt": gt}
        out[name] = write_render_set(full.model_path, name, scene.loaded_iter, views())
    return out


def metrics(args):
    from .render_set import evaluate_dir
    lp = None
    if args.lpips_weights:
        from .lpips import LpipsWeights
        lp = LpipsWeights.from_files(*args.lpips_weights)
    out = {}
    for model_path in args.model_paths:
        print("Scene:", model_path)
        res = evaluate_dir(model_path, "test", lpips=lp)   # (writes results.json and per_view.json)
        for method, r in res.items():
            print("Method:", method)
            for k in ("SSIM", "PSNR", "LPIPS", "L1"):
                if k in r:
                    print("  {} : {:>12.7f}".format(k, r[k]))
        out[model_path] = res
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    return {"train": train, "render": render_sets, "metrics": metrics}[args.command](args)


if __name__ == "__main__":
    main(sys.argv[1:])

"""Generator of tests/golden/lgdwt_args.json (run by hand with the reference checked out: the path of its LGDWT-GS directory is
the one argument; the tests only read what it wrote).

The file holds settings only: for each of the reference's three parameter groups (arguments/__init__.py: ModelParams,
PipelineParams, OptimizationParams) the flags its ArgumentParser ends up with, read back from the parser's own actions -
  name, shorthand (the one-letter option or null), type ("int", "float", "str" or "bool" = store_true), default
in the order the parser holds them, and under "train" / "render" the flags the two scripts add themselves (train.py:362-371,
render.py:67-70), recorded the same way from a parser built with the same calls' values."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, type, default, nargs) of the scripts' own flags
TRAIN_OWN = (("ip", "str", "127.0.0.1", None), ("port", "int", 6009, None), ("debug_from", "int", -1, None),
             ("detect_anomaly", "bool", False, None), ("test_iterations", "int", [7000, 30000], "+"),
             ("save_iterations", "int", [7000, 30000], "+"), ("quiet", "bool", False, None), ("disable_viewer", "bool", False, None),
             ("checkpoint_iterations", "int", [], "+"), ("start_checkpoint", "str", None, None))
RENDER_OWN = (("iteration", "int", -1, None), ("skip_train", "bool", False, None), ("skip_test", "bool", False, None),
              ("quiet", "bool", False, None))


def group_flags(cls):
    parser = argparse.ArgumentParser()
    cls(parser)
    out = []
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        longs = [s for s in a.option_strings if s.startswith("--")]
        shorts = [s for s in a.option_strings if not s.startswith("--")]
        kind = "bool" if isinstance(a, argparse._StoreTrueAction) else a.type.__name__
        out.append({"name": longs[0][2:], "shorthand": shorts[0][1:] if shorts else None, "type": kind, "default": a.default})
    return out


def main(ref):
    sys.path.insert(0, ref)
    import arguments
    rec = {"ModelParams": group_flags(arguments.ModelParams), "PipelineParams": group_flags(arguments.PipelineParams),
           "OptimizationParams": group_flags(arguments.OptimizationParams),
           "train": [{"name": n, "type": t, "default": d, "nargs": g} for n, t, d, g in TRAIN_OWN],
           "render": [{"name": n, "type": t, "default": d, "nargs": g} for n, t, d, g in RENDER_OWN]}
    with open(os.path.join(HERE, "lgdwt_args.json"), "w") as fp:
        json.dump(rec, fp, indent=1)
        fp.write("\n")
    print("wrote lgdwt_args.json: %d + %d + %d group flags" % tuple(len(rec[k]) for k in ("ModelParams", "PipelineParams",
                                                                                          "OptimizationParams")))


if __name__ == "__main__":
    main(sys.argv[1])

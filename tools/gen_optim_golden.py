"""Record tests/golden/optim/groups.json: the genuine reference's weight-decay grouping (CPU).

    python tools/gen_optim_golden.py

Builds the reference's models (imported through oracle.ref_import) for `msrvtt_care` and `msrvtt_base_ami` and runs
misc/utils.py's own filter_weight_decay under filter_biases off / on and skip_substr_list [] / ['LayerNorm', 'embedding'];
stores, per case, each returned group's parameter NAMES (in the order of its list) and weight_decay, and per model the
number of parameter tensors and elements - names and numbers only.  tests/test_optim_cpu.py holds
care_amd.optim.filter_weight_decay and configure_optimizers to it.
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "optim", "groups.json")

CONFIGS = ("msrvtt_care", "msrvtt_base_ami")
WEIGHT_DECAY = 5e-4
SKIPS = ([], ["LayerNorm", "embedding"])


def main():
    from oracle.ref_import import import_reference

    get_framework, _ = import_reference()
    from misc.utils import filter_weight_decay

    from care_amd.configs import make_opt

    out = {"weight_decay": WEIGHT_DECAY, "models": {}, "cases": []}
    for config in CONFIGS:
        model = get_framework(make_opt(config))
        names = {id(p): n for n, p in model.named_parameters()}
        out["models"][config] = {"tensors": len(names), "elements": sum(p.numel() for p in model.parameters()),
                                 "trainable": [n for n, p in model.named_parameters() if p.requires_grad]}
        for filter_biases in (False, True):
            for skip in SKIPS:
                with contextlib.redirect_stdout(io.StringIO()):   # (the function prints every name it exempts)
                    groups = filter_weight_decay(model, weight_decay=WEIGHT_DECAY, filter_biases=filter_biases, skip_list=(),
                                                 skip_substr_list=skip)
                out["cases"].append({"config": config, "filter_biases": filter_biases, "skip_substr_list": skip,
                                     "groups": [{"weight_decay": g["weight_decay"], "params": [names[id(p)] for p in g["params"]]}
                                                for g in groups]})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    for config, m in out["models"].items():
        print("{:18s} {:3d} tensors {:10d} elements".format(config, m["tensors"], m["elements"]))
    print("{} {} bytes".format(os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

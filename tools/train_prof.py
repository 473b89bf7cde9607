"""The training step of bench.py's `training_step` leg on its own (for rocprofv3 --kernel-trace --stats):
    python tools/train_prof.py [clips] [steps] [--fused-head] [--optim {none,torch,torch-fused,care}] [--clip V] [--repeat R]
--fused-head: model.set_fused_head(True) and care_amd's criterion behind the model (label smoothing 0.1, the labels on the host) -
the head's products, the loss and their backward then run over the live label rows inside the criterion.
--optim: what follows backward() inside the timed loop.  none (default): nothing, the gradients are dropped; torch:
torch.optim.Adam as the reference builds it (Wrapper.py:316-386); torch-fused: torch.optim.Adam(fused=True); care:
care_amd.optim.Adam (csrc/optim.hip).  With an optimiser a step is zero_grad(), forward + backward, (torch*, with --clip V > 0)
clip_grad_norm_(parameters, V), optimizer.step(); care takes V as max_grad_norm.  --repeat R: R timed blocks of `steps`
steps, one line each and their median."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from care_amd import get_framework
from care_amd.configs import feat_shapes, make_opt
from care_amd.synth import synth_input_ids, synth_state_dict

FUSED = "--fused-head" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--fused-head"]


def _option(name, default):
    if name in argv:
        i = argv.index(name)
        value = argv[i + 1]
        del argv[i:i + 2]
        return value
    return default


OPTIM = _option("--optim", "none")
CLIP = float(_option("--clip", "0"))
REPEAT = int(_option("--repeat", "1"))
if OPTIM not in ("none", "torch", "torch-fused", "care"):
    sys.exit("--optim must be one of none, torch, torch-fused, care")
B = int(argv[0]) if len(argv) > 0 else 64
steps = int(argv[1]) if len(argv) > 1 else 10
dev = torch.device("cuda:0")
opt = make_opt("msrvtt_care", label_smoothing=0.1)
model = get_framework(opt)
model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
model.set_compute_dtype(os.environ.get("CARE_TRAIN_DTYPE", "fp32"))
model.to(dev)
model.train()
gen = torch.Generator(device=dev)
gen.manual_seed(5)
feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, B)]
ids = synth_input_ids(7, B, opt["max_len"] - 1, opt["vocab_size"]).to(dev)
batch = {"feats": feats, "input_ids": ids}
g = None
if FUSED:
    from care_amd import get_criterion
    from care_amd.synth import synth_labels

    model.set_fused_head(True)
    crit = get_criterion(opt)
    labels = synth_labels(ids.cpu())
    labels_attr = (torch.rand(B, opt["attribute_prediction_k"], generator=gen, device=dev) > 0.96).float()
params = [prm for prm in model.parameters() if prm.requires_grad]
optim = None
if OPTIM == "care":
    from care_amd.optim import Adam

    optim = Adam(params, lr=opt.get("learning_rate", 5e-4), weight_decay=opt.get("weight_decay", 5e-4), max_grad_norm=CLIP)
elif OPTIM != "none":
    optim = torch.optim.Adam(params, lr=opt.get("learning_rate", 5e-4), weight_decay=opt.get("weight_decay", 5e-4),
                             **({"fused": True} if OPTIM == "torch-fused" else {}))


def step():
    global g
    if optim is None:
        for prm in model.parameters():
            prm.grad = None
    else:
        optim.zero_grad()
    out = model(batch)
    if FUSED:
        crit.get_loss({**out, "labels": labels, "labels_attr": labels_attr}).backward()
    else:
        if g is None:
            g = torch.randn_like(out["logits"]) * 1e-3
        torch.autograd.backward([out["logits"]], [g])
    if optim is not None:
        if CLIP > 0 and OPTIM != "care":
            torch.nn.utils.clip_grad_norm_(params, CLIP)
        optim.step()


for _ in range(3):
    step()
what = "training step%s%s, %d clips" % (" (fused head + criterion)" if FUSED else "",
                                        "" if optim is None else " + %s Adam%s" % (OPTIM, ", clip %g" % CLIP if CLIP > 0 else ""), B)
times = []
for _ in range(REPEAT):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) / steps * 1e3)
    print("%s: %.3f ms" % (what, times[-1]))
if REPEAT > 1:
    print("%s: median of %d: %.3f ms" % (what, REPEAT, sorted(times)[REPEAT // 2]))

"""The mean-teacher step, timed (one JSON line):

    python tools/interplay_bench.py [--clips 64,512] [--windows 5] [--window-s 0.3] [--no-step]

1. THE MOVING AVERAGE ALONE over the parameter list of msrvtt_care (two modules on the device): care_amd.ema_update (one
   care_ema_step for all tensors) against the reference's three calls, torch._foreach_mul_ / _foreach_mul / _foreach_add_
   (Wrapper.py:574-581); and care_ema_step on descriptors built once, which leaves out ema_update's host side - back to back
   with nothing else queued the host side is what a call costs, inside a step it runs ahead of the device.
2. THE DISTILLATION TERM, forward + backward, on logits [clips, 29, 10547]: care_amd.distillation_mse against the eager
   expression ((a - b) ** 2).mean() (Wrapper.py:565), the gradient to `a` only in both.
3. THE WHOLE STEP (msrvtt_care; zero_grad, forward, criterion, backward, care_amd's Adam with clipping): the plain `Model` step
   of tools/train_prof.py, InterplayStep.training_step, and the same sequence with the two eager forms of 1 and 2 in place of the
   kernels.

tools/loss_bench.py's method: device events around a window of calls; every shape and every variant warmed up first; the variants
ALTERNATE window by window in one process; medians of >= 5 windows of >= 0.3 s each, with min and max.  Floors from shapes, at the
6.29 TB/s float4-copy rate: 12 B per parameter for the average (read t, s, write t), 8 B per logit forward (read a, b) and 12 B
backward (read a, b, write the gradient).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from care_amd import _lib
from care_amd import InterplayStep, configure_optimizers, distillation_mse, ema_update, get_criterion, get_framework
from care_amd.configs import feat_shapes, make_opt
from care_amd.constants import PAD
from care_amd.synth import synth_state_dict
from loss_bench import COPY_RATE, EPS, K, T, V, mixed_labels, summary, windows


def _model(opt, seed, dev):
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(seed, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    return model.to(dev).train()


def ema_alone(dev, n_windows, window_s):
    opt = make_opt("msrvtt_care")
    teacher, student = list(_model(opt, 1, dev).parameters()), list(_model(opt, 0, dev).parameters())
    elements = sum(p.numel() for p in teacher)

    def ours():
        ema_update(teacher, student, 0.999)

    @torch.no_grad()
    def eager():
        torch._foreach_mul_(teacher, 0.999)
        torch._foreach_add_(teacher, torch._foreach_mul(student, 1 - 0.999))

    # the kernel without ema_update's host side (its checks and the descriptors of 55 pairs, built per call): descriptors built once
    descs = (_lib.EmaTensor * len(teacher))()
    for d, t, s in zip(descs, teacher, student):
        d.t, d.s, d.n = t.data_ptr(), s.data_ptr(), t.numel()

    def kernel_only():
        _lib.call("care_ema_step", descs, len(teacher), 0.999, 1 - 0.999)

    ts = windows({"care_amd": ours, "eager_torch": eager, "care_ema_step_alone": kernel_only}, n_windows, window_s)
    floor = 12 * elements
    ours_s, eager_s, kernel_s = (statistics.median(ts[k]) for k in ("care_amd", "eager_torch", "care_ema_step_alone"))
    return dict(tensors=len(teacher), elements=elements, floor_bytes=floor, floor_us_at_copy_rate=round(floor / COPY_RATE * 1e6, 2),
                care_amd=summary(ts["care_amd"]), eager_torch=summary(ts["eager_torch"]), care_ema_step_alone=summary(ts["care_ema_step_alone"]),
                eager_over_care_amd=round(eager_s / ours_s, 3), care_amd_share_of_copy_rate=round(floor / ours_s / COPY_RATE, 3),
                care_ema_step_alone_share_of_copy_rate=round(floor / kernel_s / COPY_RATE, 3))


def distillation_alone(clips, dev, n_windows, window_s):
    gen = torch.Generator(device=dev).manual_seed(clips)
    a = (torch.randn(clips, T, V, generator=gen, device=dev) * 2.0).requires_grad_(True)
    b = a.detach() + 0.5 * torch.randn(clips, T, V, generator=gen, device=dev)

    def ours():
        a.grad = None
        distillation_mse(a, b).backward()

    def eager():
        a.grad = None
        ((a - b) ** 2).mean().backward()

    ours()
    g_ours, l_ours = a.grad.clone(), float(distillation_mse(a, b).detach())
    eager()
    l_eager = float(((a - b) ** 2).mean().detach())
    grad_diff = float((g_ours - a.grad).abs().max() / a.grad.abs().max())
    del g_ours
    ts = windows({"care_amd": ours, "eager_torch": eager}, n_windows, window_s)
    n = a.numel()
    floor = 20 * n
    ours_s, eager_s = statistics.median(ts["care_amd"]), statistics.median(ts["eager_torch"])
    return dict(clips=clips, logits=n, logits_bytes=4 * n, floor_bytes=floor, floor_ms_at_copy_rate=round(floor / COPY_RATE * 1e3, 4),
                care_amd=summary(ts["care_amd"]), eager_torch=summary(ts["eager_torch"]), eager_over_care_amd=round(eager_s / ours_s, 3),
                care_amd_share_of_copy_rate=round(floor / ours_s / COPY_RATE, 3), loss_care_amd=l_ours, loss_eager=l_eager,
                max_rel_grad_difference=grad_diff)


def whole_step(clips, dev, n_windows, window_s):
    opt = make_opt("msrvtt_care", label_smoothing=EPS, gradient_clip_val=5.0)
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, clips)]
    labels = mixed_labels(clips, 12)
    ids = torch.full_like(labels, PAD)
    ids[:, 0] = 2
    ids[:, 1:] = labels[:, :-1]                      # teacher forcing: input = BOS + the labels shifted
    labels_attr = (torch.rand(clips, K, generator=gen, device=dev) > 0.96).float()
    batch = {"feats": feats, "input_ids": ids.to(dev), "labels": labels.to(dev), "labels_attr": labels_attr}

    plain_model = _model(opt, 0, dev)
    plain_crit = get_criterion(opt, override_opt={"calculate_mAP": False})
    plain_optim = configure_optimizers(opt, plain_model)["optimizer"]

    def plain():
        loss = plain_crit.get_loss({**plain_model(batch, current_epoch=0), **batch})
        plain_optim.zero_grad()
        loss.backward()
        plain_optim.step()

    hip = InterplayStep(opt, _model(opt, 0, dev), teacher=_model(opt, 1, dev))
    eag = InterplayStep(opt, _model(opt, 0, dev), teacher=_model(opt, 1, dev))

    def interplay():
        hip.training_step(batch)

    def interplay_eager():
        s = eag.captioner(batch, current_epoch=0)
        cap = eag.criterion.get_loss({**s, **batch})
        with torch.no_grad():
            t = eag.teacher_captioner(batch, current_epoch=0)
        loss = cap + eag.distillation_weight * ((s["logits"] - t["logits"]) ** 2).mean()
        eag.optimizer.zero_grad()
        loss.backward()
        eag.optimizer.step()
        with torch.no_grad():
            w = eag.ema_weight
            ps, pt = list(eag.captioner.parameters()), list(eag.teacher_captioner.parameters())
            torch._foreach_mul_(pt, w)
            torch._foreach_add_(pt, torch._foreach_mul(ps, 1 - w))

    ts = windows({"plain_model_step": plain, "interplay_care_amd": interplay, "interplay_eager_pieces": interplay_eager}, n_windows, window_s)
    for c in (plain_crit, hip.criterion, eag.criterion):
        c.reset_loss_recorder()
    return dict(clips=clips, **{k: summary(v) for k, v in ts.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="64,512")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interplay_bench.py measures on the MI355X: no GPU, no numbers")
    if a.windows < 5 or a.window_s < 0.3:
        raise SystemExit("at least 5 windows of at least 0.3 s")
    dev = torch.device("cuda:0")
    sizes = [int(c) for c in a.clips.split(",")]
    res = dict(tool="interplay_bench", shape=dict(positions=T, vocab=V), copy_rate_bytes_per_s=COPY_RATE,
               ema_alone=ema_alone(dev, a.windows, a.window_s),
               distillation_alone=[distillation_alone(c, dev, a.windows, a.window_s) for c in sizes])
    if not a.no_step:
        res["whole_step"] = [whole_step(c, dev, a.windows, a.window_s) for c in sizes]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

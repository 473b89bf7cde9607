"""The training criteria, timed (one JSON line):

    python tools/loss_bench.py [--clips 64,512] [--windows 5] [--window-s 0.3] [--no-step] [--head [--chunk-rows 0,4096,2048]] [--no-alone]

1. THE CRITERION ALONE, forward + backward, at 64 and 512 clips x 29 positions x 10547 columns (+ the concept BCE on [clips, 500]),
   captions of mixed length (mean ~8 of 29 positions, the rest PAD - like bench.py's model that ends its captions):
   care_amd.criterion against an eager-torch restatement of the same formulas (misc/Crit/crit_lang.py, crit_attribute.py:
   log_softmax, max, gather, mean, NLLLoss, the mask; three .item() per step as in the reference) on the same device and inputs.
   Device events around a window of calls; every shape and both variants warmed up first; the two variants ALTERNATE window by
   window in one process; medians of >= 5 windows of >= 0.3 s each, with the spread (min .. max) reported.
2. THE TRAINING STEP of tools/train_prof.py (msrvtt_care, forward + backward of the whole model) without a criterion (a fixed
   upstream gradient on the logits, as bench.py's training legs) and with care_amd's criterion and with the eager one.

3. THE HEAD AND THE CRITERION TOGETHER (--head), forward + backward from the decoder's hidden states [clips, 29, 512]
   and the head's weight [10547, 512] - the head's three products are inside every variant, so the comparison is like for like:
   `unfused` (training.py's `_Linear` + the criterion on its logits), `fused` (criterion.DeferredLogits: projection, loss and
   backward over the live rows, HEAD_CHUNK_ROWS as --chunk-rows gives them, 0 = whole) and `eager_torch` (matmul + the eager
   criterion); and the training step with the fused head beside the three of 2.

Bytes are computed from shapes: the floor is three sweeps of the LIVE rows (one read forward, one read + one write backward)
plus the zero fill of the dead rows of the gradient; bytes / time is set against the 6.29 TB/s float4-copy rate.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from care_amd import get_criterion, get_framework
from care_amd.configs import feat_shapes, make_opt
from care_amd.constants import EOS, PAD
from care_amd.synth import synth_state_dict

COPY_RATE = 6.29e12   # bytes / s, float4 copy
T, V, K = 29, 10547, 500
EPS = 0.1


def mixed_labels(clips, seed):
    """labels [clips, 29]: words, EOS, then PAD; lengths geometric with mean ~8, clipped to 2 .. 29."""
    g = torch.Generator().manual_seed(seed)
    lengths = (2 + torch.empty(clips).exponential_(1.0 / 6.0, generator=g)).long().clamp_(2, T)
    labels = torch.randint(6, V, (clips, T), generator=g)
    pos = torch.arange(T).unsqueeze(0)
    labels[pos == (lengths - 1).unsqueeze(1)] = EOS
    labels[pos >= lengths.unsqueeze(1)] = PAD
    return labels


def eager_criterion(logits, labels, preds, labels_attr, eps=EPS):
    """What a user writes today: the reference's chain in eager torch, its three host synchronisations included."""
    lsm = torch.log_softmax(logits, dim=-1)
    ind = labels.ne(PAD)
    pred = lsm.max(-1)[1][ind]
    acc = (pred == labels[ind]).sum().item() / pred.size(0)
    logp = lsm.gather(2, labels.unsqueeze(2)).squeeze(2)
    n_words = float(torch.sum(ind))
    ce = (-torch.sum(logp * ind) / n_words).item()
    flat, lab = lsm.contiguous().view(-1, lsm.size(2)), labels.contiguous().view(-1)
    loss = (1 - eps) * torch.nn.functional.nll_loss(flat, lab, reduction="none") + eps * -flat.mean(dim=-1)
    lang = torch.sum(loss * lab.ne(PAD).float()) / logits.size(0)
    total, rec = lang, [lang.item()]
    if preds is not None:
        p = torch.clamp(preds, 0.01, 0.99)
        y = labels_attr[:, : p.shape[1]]
        bce = -(y * torch.log(p) + (1.0 - y) * torch.log(1.0 - p))
        attr = (bce.sum(1) / torch.max(torch.tensor(1.0, device=p.device), y.sum(1))).sum() / p.size(0)
        total = total + attr
    return total, (acc, ce, rec)


def windows(variants, n_windows, window_s):
    """variants: {name: callable}; returns {name: [seconds per call, per window]} with the variants alternated."""
    iters = {}
    for name, fn in variants.items():     # warm up, and size the window
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3):
            fn()
        b.record()
        torch.cuda.synchronize()
        iters[name] = max(3, int(math.ceil(window_s / (a.elapsed_time(b) * 1e-3 / 3))))
    out = {name: [] for name in variants}
    for _ in range(n_windows):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1e-3 / iters[name])
    return out


def summary(ts):
    return dict(ms=round(statistics.median(ts) * 1e3, 4), min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4), windows=len(ts))


def criterion_alone(clips, dev, n_windows, window_s):
    gen = torch.Generator(device=dev).manual_seed(clips)
    logits = (torch.randn(clips, T, V, generator=gen, device=dev) * 2.0).requires_grad_(True)
    preds = torch.rand(clips, K, generator=gen, device=dev).requires_grad_(True)
    labels = mixed_labels(clips, 11).to(dev)
    labels_attr = (torch.rand(clips, K, generator=gen, device=dev) > 0.96).float()
    crit = get_criterion(make_opt("msrvtt_care", label_smoothing=EPS))
    results = {"logits": logits, "labels": labels, "preds_attr": preds, "avg_prob_attr": None, "labels_attr": labels_attr}

    def ours():
        logits.grad = preds.grad = None
        crit.get_loss(results).backward()

    def eager():
        logits.grad = preds.grad = None
        eager_criterion(logits, labels, preds, labels_attr)[0].backward()

    # the two compute the same thing (at the sizes timed)
    ours()
    g_ours, l_ours = logits.grad.clone(), float(crit.get_loss(results).detach())
    eager()
    l_eager = float(eager_criterion(logits, labels, preds, labels_attr)[0].detach())
    grad_diff = float((g_ours - logits.grad).abs().max())
    del g_ours
    crit.reset_loss_recorder()
    ts = windows({"care_amd": ours, "eager_torch": eager}, n_windows, window_s)
    live = int(labels.ne(PAD).sum())
    rows = clips * T
    floor_bytes = 3 * live * V * 4 + (rows - live) * V * 4
    ours_s, eager_s = statistics.median(ts["care_amd"]), statistics.median(ts["eager_torch"])
    return dict(clips=clips, rows=rows, live_rows=live, logits_bytes=rows * V * 4, live_logits_bytes=live * V * 4,
                floor_bytes=floor_bytes, floor_ms_at_copy_rate=round(floor_bytes / COPY_RATE * 1e3, 4),
                all_rows_three_sweeps_bytes=3 * rows * V * 4,
                care_amd=summary(ts["care_amd"]), eager_torch=summary(ts["eager_torch"]),
                eager_over_care_amd=round(eager_s / ours_s, 3),
                care_amd_floor_bytes_per_s=round(floor_bytes / ours_s / 1e12, 3), care_amd_share_of_copy_rate=round(floor_bytes / ours_s / COPY_RATE, 3),
                loss_care_amd=l_ours, loss_eager=l_eager, max_abs_grad_difference=grad_diff)


def head_and_criterion(clips, dev, n_windows, window_s, chunk_rows):
    """Forward + backward from (hidden, W): unfused, fused (one variant per chunk size) and eager, alternating."""
    from care_amd import criterion as crit_mod
    from care_amd import training
    from care_amd.criterion import DeferredLogits

    d = 512
    gen = torch.Generator(device=dev).manual_seed(clips + 1)
    hidden = torch.randn(clips, T, d, generator=gen, device=dev).requires_grad_(True)
    W = (torch.randn(V, d, generator=gen, device=dev) * (2.0 / math.sqrt(d))).requires_grad_(True)
    preds = torch.rand(clips, K, generator=gen, device=dev).requires_grad_(True)
    labels_host = mixed_labels(clips, 11)
    labels = labels_host.to(dev)
    labels_attr = (torch.rand(clips, K, generator=gen, device=dev) > 0.96).float()
    crit = get_criterion(make_opt("msrvtt_care", label_smoothing=EPS))
    live = int(labels_host.ne(PAD).sum())

    def zero():
        hidden.grad = W.grad = preds.grad = None

    def unfused():
        zero()
        logits = training._Linear.apply(hidden.view(clips * T, d), W, None).view(clips, T, V)
        crit.get_loss({"logits": logits, "labels": labels_host, "preds_attr": preds, "avg_prob_attr": None, "labels_attr": labels_attr}).backward()

    def fused_with(rows):
        def run():
            zero()
            crit_mod.HEAD_CHUNK_ROWS = rows if rows > 0 else 1 << 30
            crit.get_loss({"logits": DeferredLogits(hidden, W), "labels": labels_host, "preds_attr": preds, "avg_prob_attr": None,
                           "labels_attr": labels_attr}).backward()
        return run

    def eager():
        zero()
        eager_criterion(hidden @ W.t(), labels, preds, labels_attr)[0].backward()

    default_rows = crit_mod.HEAD_CHUNK_ROWS
    variants = {"unfused": unfused, "eager_torch": eager}
    for rows in chunk_rows:
        variants["fused_chunk_{}".format(rows if rows > 0 else "whole")] = fused_with(rows)
    unfused()
    gh, gw = hidden.grad.clone(), W.grad.clone()
    fused_with(chunk_rows[0])()
    diff = dict(dhidden=float((hidden.grad - gh).abs().max() / gh.abs().max()), dW=float((W.grad - gw).abs().max() / gw.abs().max()))
    del gh, gw
    crit.reset_loss_recorder()
    try:
        ts = windows(variants, n_windows, window_s)
    finally:
        crit_mod.HEAD_CHUNK_ROWS = default_rows
    rows = clips * T
    # what must move once: W and its gradient, the hidden rows and their gradient (fp32), the gradient's pieces written and read
    # twice (8 bytes per live row and column, hi | lo and the transpose); 3 + 1 products over the live rows (forward, the
    # recomputation, dh, dW) of 2 R V d flops each, three fp16 passes per product
    floor_bytes = 2 * V * d * 4 + 2 * rows * d * 4 + 3 * 8 * live * V // 2
    flops = 4 * 2.0 * live * V * d
    return dict(clips=clips, rows=rows, live_rows=live, live_share=round(live / rows, 4), floor_bytes=floor_bytes,
                floor_ms_at_copy_rate=round(floor_bytes / COPY_RATE * 1e3, 4), product_flops=flops,
                fused_vs_unfused_max_rel_grad_difference=diff, **{k: summary(v) for k, v in ts.items()})


def training_step(clips, dev, n_windows, window_s, fused=False):
    opt = make_opt("msrvtt_care", label_smoothing=EPS)
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model.to(dev)
    model.train()
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, clips)]
    labels = mixed_labels(clips, 12)
    ids = torch.full_like(labels, PAD)
    ids[:, 0] = 2
    ids[:, 1:] = labels[:, :-1]                      # teacher forcing: input = BOS + the labels shifted
    batch = {"feats": feats, "input_ids": ids.to(dev)}
    labels = labels.to(dev)
    labels_attr = (torch.rand(clips, K, generator=gen, device=dev) > 0.96).float()
    crit = get_criterion(opt)
    fixed = {}

    def zero():
        for prm in model.parameters():
            prm.grad = None

    def no_criterion():
        zero()
        out = model(batch)
        if "g" not in fixed:
            fixed["g"] = torch.randn_like(out["logits"]) * 1e-3
        torch.autograd.backward([out["logits"]], [fixed["g"]])

    def with_care_amd():
        zero()
        crit.get_loss({**model(batch), "labels": labels, "labels_attr": labels_attr}).backward()

    def with_eager():
        zero()
        out = model(batch)
        eager_criterion(out["logits"], labels, out["preds_attr"], labels_attr)[0].backward()

    labels_host = labels.cpu()

    def with_fused_head():
        zero()
        model.set_fused_head(True)
        try:
            crit.get_loss({**model(batch), "labels": labels_host, "labels_attr": labels_attr}).backward()
        finally:
            model.set_fused_head(False)

    variants = {"no_criterion": no_criterion, "care_amd_criterion": with_care_amd, "eager_criterion": with_eager}
    if fused:
        variants["fused_head_and_criterion"] = with_fused_head
    ts = windows(variants, n_windows, window_s)
    live = int(labels_host.ne(PAD).sum())
    return dict(clips=clips, live_rows=live, live_share=round(live / (clips * T), 4), **{k: summary(v) for k, v in ts.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="64,512")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    ap.add_argument("--head", action="store_true", help="head + criterion together: unfused, fused, eager (and the fused training step)")
    ap.add_argument("--chunk-rows", default="4096", help="HEAD_CHUNK_ROWS of the fused variants, comma separated (0 = whole)")
    ap.add_argument("--no-alone", action="store_true", help="skip the criterion on ready logits")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench.py measures on the MI355X: no GPU, no numbers")
    if a.windows < 5 or a.window_s < 0.3:
        raise SystemExit("at least 5 windows of at least 0.3 s")
    dev = torch.device("cuda:0")
    sizes = [int(c) for c in a.clips.split(",")]
    res = dict(tool="loss_bench", shape=dict(positions=T, vocab=V, concepts=K, label_smoothing=EPS), copy_rate_bytes_per_s=COPY_RATE,
               criterion_alone=[] if a.no_alone else [criterion_alone(c, dev, a.windows, a.window_s) for c in sizes])
    if a.head:
        chunk_rows = [int(c) for c in a.chunk_rows.split(",")]
        res["head_and_criterion"] = [head_and_criterion(c, dev, a.windows, a.window_s, chunk_rows) for c in sizes]
    if not a.no_step:
        res["training_step"] = [training_step(c, dev, a.windows, a.window_s, fused=a.head) for c in sizes]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

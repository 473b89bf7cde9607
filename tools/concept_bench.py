"""The concept metrics, timed (one JSON line):

    python tools/concept_bench.py [--clips 128,512] [--windows 5] [--window-s 0.2] [--epoch-batches 24] [--repeats 3] [--no-epoch]
                                  [--videos 2990] [--batch 128]

1. ONE STEP at K = 500 concepts, about 25 positives a clip, 128 and 512 clips, device events around a window of calls, the
   variants ALTERNATED window by window in one process, medians of >= 5 windows with the spread (min .. max):
   `kernel`  care_concept_metrics into preallocated outputs and running totals (two launches);
   `caller`  care_amd.metrics.concept_metrics_device (the same plus its three small allocations);
   `sorted`  the route this replaces, per step: clamp, topk(50), six gathers and the F1 arithmetic in eager torch on the device
             (what NoisyOrMIL._step ran), and the clamped copy kept for the epoch's end.
2. AN EPOCH of `--epoch-batches` steps of 128 clips up to the numbers on the host, wall clock around a synchronised run (median
   of `--repeats` after a warm-up): `kernel` = the steps and ONE read of the totals; `sorted` = the steps and then, for mAP, two
   full sorts a batch, the ranks copied to the host and the Python loop over the clips (crit_attribute.py:73-86).
3. THE VALIDATION EPOCH of tools/validation_bench.py (2990 videos x 20 references, msrvtt_care, greedy, batch 128), with and
   without `labels_attr` in the batches: what concept scoring adds to an epoch.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from care_amd import _lib
from care_amd.metrics import TOPK_LIST, concept_metrics_device, concept_scores, concept_totals

K = 500


def windows(variants, n_windows, window_s):
    """variants: {name: callable}; {name: [seconds per call, per window]} with the variants alternated (tools/loss_bench.py)."""
    iters = {}
    for name, fn in variants.items():
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


def summary(ts, unit=1e6, key="us"):
    return {key: round(statistics.median(ts) * unit, 3), "min_" + key: round(min(ts) * unit, 3), "max_" + key: round(max(ts) * unit, 3),
            "windows": len(ts)}


def inputs(clips, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    preds = torch.rand(clips, K, generator=gen, device=dev) * 1.1 - 0.05
    labels = (torch.rand(clips, K, generator=gen, device=dev) < 25.0 / K).float()
    return preds, labels


def sorted_step(preds, labels, acc, pending):
    """The metric half of the NoisyOrMIL._step this replaces."""
    p = torch.clamp(preds, 0.01, 0.99)
    _, cand = p.topk(max(TOPK_LIST), dim=1, sorted=True, largest=True)
    n_pos = labels.sum(1)
    f1s = []
    for k in TOPK_LIST:
        hit = labels.gather(1, cand[:, :k]).sum(1)
        hit = torch.where(hit.eq(0), torch.full_like(hit, 1e-3), hit)
        precision, recall = hit / k, hit / n_pos
        f1s.append((2 * precision * recall / (precision + recall)).sum())
    acc += torch.stack(f1s).double()
    if pending is not None:
        pending.append((p, labels))


def sorted_mean_ap(pending):
    """crit_attribute.py:72-86 at the epoch's end: two sorts a batch, the ranks to the host, a loop over the clips."""
    aps = []
    for p, y in pending:
        _, idx = p.sort(dim=1, descending=True)
        _, rank = idx.sort(dim=1)
        rank, y = rank.cpu(), y.cpu()
        for i in range(y.shape[0]):
            pos = y[i].nonzero().squeeze(1)
            hit_rank, _ = rank[i][pos].sort()
            ids = torch.arange(len(pos))
            aps.append(float(((ids + 1).float() / (hit_rank + 1)).mean()))
    return sum(aps) / len(aps)


def one_step(clips, dev, n_windows, window_s):
    preds, labels = inputs(clips, dev, clips)
    n = len(TOPK_LIST)
    ap = torch.empty(clips, device=dev, dtype=torch.float64)
    hits = torch.empty(clips, n, device=dev, dtype=torch.int32)
    n_pos = torch.empty(clips, device=dev, dtype=torch.int32)
    td, ti = concept_totals(n, dev)
    tk = (ctypes.c_int32 * n)(*TOPK_LIST)
    acc = torch.zeros(n, device=dev, dtype=torch.float64)

    def kernel():
        _lib.call("care_concept_metrics", preds.data_ptr(), K, labels.data_ptr(), K, clips, K, tk, n, ap.data_ptr(), hits.data_ptr(),
                  n_pos.data_ptr(), td.data_ptr(), ti.data_ptr())

    ts = windows({"kernel": kernel, "caller": lambda: concept_metrics_device(preds, labels, totals=(td, ti)),
                  "sorted": lambda: sorted_step(preds, labels, acc, None)}, n_windows, window_s)
    out = {name: summary(t) for name, t in ts.items()}
    out["sorted_over_kernel"] = round(out["sorted"]["us"] / out["kernel"]["us"], 1)
    out["mean_positives"] = round(float(labels.sum(1).mean()), 1)
    return out


def one_epoch(batches, clips, dev, repeats):
    data = [inputs(clips, dev, 100 + b) for b in range(batches)]
    n = len(TOPK_LIST)

    def kernel():
        totals = concept_totals(n, dev)
        for p, y in data:
            concept_metrics_device(p, y, totals=totals)
        return concept_scores(totals[0].cpu().tolist(), totals[1].cpu().tolist())

    def by_sort():
        acc, pending = torch.zeros(n, device=dev, dtype=torch.float64), []
        for p, y in data:
            sorted_step(p, y, acc, pending)
        out = {"F1-%02d" % k: v / (batches * clips) for k, v in zip(TOPK_LIST, acc.cpu().tolist())}
        out["mAP"] = sorted_mean_ap(pending)
        return out

    res = {}
    for name, fn in (("kernel", kernel), ("sorted", by_sort)):
        fn()
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[name] = dict(summary(ts, 1e3, "ms"), mAP=got["mAP"], F1_50=got["F1-50"])
    res["sorted_over_kernel"] = round(res["sorted"]["ms"] / res["kernel"]["ms"], 1)
    return res


def validation_epoch(videos, batch, dev, repeats):
    from care_amd import MetricBank, ValidationEpoch, get_framework
    from care_amd.configs import feat_shapes, make_opt
    from care_amd.synth import synth_state_dict
    from scst_bench import synthetic_corpus

    bank = MetricBank(synthetic_corpus(videos, 20), 10547, device=dev)
    opt = make_opt("msrvtt_care")
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, batch)]
    labels = (torch.rand(batch, 3000, generator=gen, device=dev) < 25.0 / K).float()
    bare = [{"feats": [f[: min(batch, videos - lo)] for f in feats], "video_ids": list(range(lo, min(lo + batch, videos)))}
            for lo in range(0, videos, batch)]
    full = [dict(b, labels_attr=labels[: len(b["video_ids"])]) for b in bare]
    epoch = ValidationEpoch(opt, model, bank, beam_size=1)
    res = {"videos": videos, "batch": batch, "batches": len(bare)}
    ts = {"without_labels_attr": [], "with_labels_attr": []}
    for name, batches in (("without_labels_attr", bare), ("with_labels_attr", full)):
        epoch.run(batches)
    for _ in range(repeats):   # alternated
        for name, batches in (("without_labels_attr", bare), ("with_labels_attr", full)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = epoch.run(batches)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
            res[name + "_mAP"] = got.get("mAP")
    for name, t in ts.items():
        res[name] = summary(t, 1e3, "ms")
    res["added_ms"] = round(res["with_labels_attr"]["ms"] - res["without_labels_attr"]["ms"], 3)
    res["added_us_per_batch"] = round(res["added_ms"] * 1e3 / len(bare), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="128,512")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--epoch-batches", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-epoch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("concept_bench.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    res = dict(tool="concept_bench", K=K, topk=list(TOPK_LIST))
    res["step"] = {c: one_step(int(c), dev, a.windows, a.window_s) for c in a.clips.split(",")}
    res["epoch_of_%d_batches_of_128" % a.epoch_batches] = one_epoch(a.epoch_batches, 128, dev, a.repeats)
    if not a.no_epoch:
        res["validation_epoch"] = validation_epoch(a.videos, a.batch, dev, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

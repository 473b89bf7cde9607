"""The tests' own restatement of the concept metrics (misc/Crit/crit_attribute.py:58-89) in float64 numpy - the yardstick of
tests/test_concept_metrics_cpu.py (pinned there to the recorded reference, tests/golden/crit) and of the GPU tests of
care_concept_metrics (csrc/concept_metrics.hip), of NoisyOrMIL and of the validation epoch.

The order of a clip's columns (include/care_hip.h, "Concept metrics"): clamp(p, 0.01, 0.99) in fp32 descending, NaN before every
number, the lower column first among equals - a STABLE argsort of a key that is -inf for NaN and -p otherwise.  From it, per
positive column j (label != 0, j < K): rank_j = the columns before j, posrank_j = the positives before j; then the reference's
formulas on those integers in float64, the sum of a clip's AP terms exactly rounded (math.fsum)."""
import math

import numpy as np

TOPK_LIST = (5, 10, 20, 30, 40, 50)
LO, HI = np.float32(0.01), np.float32(0.99)


def clamp32(preds):
    """torch.clamp(p, 0.01, 0.99) on fp32: NaN stays NaN."""
    p = np.asarray(preds, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p), p, np.minimum(np.maximum(p, LO), HI)).astype(np.float32)


def order(row):
    """The columns of one clamped fp32 row, first to last."""
    key = np.where(np.isnan(row), -np.inf, -row.astype(np.float64))
    return np.argsort(key, kind="stable")


def f1(hit, k, n_pos):
    """crit_attribute.py:64-68 for one clip, in float64: hit == 0 -> 1e-3; no positive -> x / 0 -> NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.float64(1e-3 if hit == 0 else hit)
        precision, recall = h / np.float64(k), h / np.float64(n_pos)
        return float(2 * precision * recall / (precision + recall))


def clip(preds_row, labels_row, topk=TOPK_LIST):
    """One clip: dict(rank, posrank - int arrays over the positives in ascending column order -, hits [len(topk)], n_pos, ap, f1)."""
    K = len(preds_row)
    row = clamp32(preds_row)
    positive = np.asarray(labels_row)[:K] != 0
    o = order(row)
    place = np.empty(K, dtype=np.int64)
    place[o] = np.arange(K)
    cols = np.nonzero(positive)[0]
    rank = place[cols]
    posrank = np.argsort(np.argsort(rank, kind="stable"), kind="stable") if len(cols) else rank
    P = int(len(cols))
    hits = [int((rank < k).sum()) for k in topk]
    terms = [(int(s) + 1) / (int(r) + 1) for s, r in zip(posrank, rank)]
    ap = math.fsum(terms) / P if P else float("nan")
    return {"rank": rank, "posrank": posrank, "hits": hits, "n_pos": P, "ap": ap, "f1": [f1(h, k, P) for h, k in zip(hits, topk)]}


def batch(preds, labels, topk=TOPK_LIST):
    """A batch [B, K] / [B, >= K]: per-clip arrays (ap float64 [B], hits int [B, n], n_pos int [B], f1 float64 [B, n]), the
    totals the kernel adds (totals_d = sum F1@k .., sum AP - NaN as soon as one clip has no positive -, totals_i = clips, clips
    without a positive) and the scores (the sums over the clip count)."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    clips = [clip(preds[b], labels[b], topk) for b in range(preds.shape[0])]
    B, n = len(clips), len(topk)
    out = {"clips": clips,
           "ap": np.array([c["ap"] for c in clips], dtype=np.float64),
           "hits": np.array([c["hits"] for c in clips], dtype=np.int64).reshape(B, n),
           "n_pos": np.array([c["n_pos"] for c in clips], dtype=np.int64),
           "f1": np.array([c["f1"] for c in clips], dtype=np.float64).reshape(B, n)}
    out["totals_d"] = np.array([math.fsum(out["f1"][:, t]) if np.isfinite(out["f1"][:, t]).all() else float("nan") for t in range(n)] +
                               [math.fsum(out["ap"]) if np.isfinite(out["ap"]).all() else float("nan")], dtype=np.float64)
    out["totals_i"] = np.array([B, int((out["n_pos"] == 0).sum())], dtype=np.int64)
    return out


def scores(totals_d, totals_i, topk=TOPK_LIST):
    """{"F1-05": .., "mAP": ..} of summed totals."""
    with np.errstate(invalid="ignore"):
        d = np.asarray(totals_d, dtype=np.float64) / float(totals_i[0])
    out = {"F1-%02d" % k: float(d[t]) for t, k in enumerate(topk)}
    out["mAP"] = float(d[len(topk)])
    return out


def epoch(batches, topk=TOPK_LIST):
    """scores over [(preds, labels), ...] plus "n_no_positive"."""
    res = [batch(p, y, topk) for p, y in batches]
    d = np.sum([r["totals_d"] for r in res], axis=0)
    i = np.sum([r["totals_i"] for r in res], axis=0)
    out = scores(d, i, topk)
    out["n_no_positive"] = int(i[1])
    return out

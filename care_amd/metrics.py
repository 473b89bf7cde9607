"""The evaluation metrics step next to the path.

* `language_metrics`: word accuracy and perplexity of the teacher-forced pass
  (misc/Crit/crit_lang.py:75-103), from the fused device scoring (engine.score_teacher_forced).
* `concept_metrics`: F1@k and mAP of the concept probabilities against multi-hot labels
  (misc/Crit/crit_attribute.py:58-89), evaluated on the (all-gathered) `preds_attr` with torch's sort and top-k;
  `concept_metrics_device`: the same numbers from care_concept_metrics (csrc/concept_metrics.hip) - no sort, equal
  probabilities in ONE defined order, per-clip results and running totals that stay on the device.
Of the COCO text metrics only METEOR and the PTB tokenizer need the reference's Java tools and stay external; BLEU, ROUGE-L and
CIDEr are scored on the device over token ids (care_amd/capmetrics.py, care_amd/validation.py).
"""
import ctypes
import math
from typing import Dict, Tuple

import torch

from . import _lib
from .constants import PAD

TOPK_LIST = (5, 10, 20, 30, 40, 50)  # crit_attribute.py:20


def concept_totals(n_topk: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Zeroed running totals of care_concept_metrics: (double [n_topk + 1] = sum F1@k .., sum AP; int64 [2] = clips, clips
    without a positive)."""
    return (torch.zeros(n_topk + 1, device=device, dtype=torch.float64), torch.zeros(2, device=device, dtype=torch.int64))


def concept_metrics_device(preds_attr: torch.Tensor, labels_attr: torch.Tensor, topk=TOPK_LIST, totals=None, per_clip: bool = False):
    """F1@k and AP of a batch through care_concept_metrics (csrc/concept_metrics.hip): the formulas of `concept_metrics` with
    ONE order of equal probabilities (the lower column first, NaN before every number), nothing read on the host.
    preds_attr [B, K] and labels_attr [B, Kl >= K] on the device (labels are read in place).  `totals`: a `concept_totals`
    pair the batch is ADDED to (made when None).  Returns the totals pair, or with per_clip
    (totals, {"ap": double [B], "hits": int32 [B, len(topk)], "n_pos": int32 [B]})."""
    for t, what in ((preds_attr, "preds_attr"), (labels_attr, "labels_attr")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("`{}` must be a tensor on the MI355X (there is no CPU fallback)".format(what))
    if preds_attr.dim() != 2 or labels_attr.dim() != 2 or labels_attr.shape[0] != preds_attr.shape[0] or \
            labels_attr.shape[1] < preds_attr.shape[1]:
        raise ValueError("preds_attr [B, K] and labels_attr [B, >= K] expected, got {} and {}".format(
            tuple(preds_attr.shape), tuple(labels_attr.shape)))
    topk = [int(k) for k in topk]
    preds, labels = (t if t.dtype == torch.float32 else t.float() for t in (preds_attr.detach(), labels_attr))
    preds, labels = (t if t.stride(-1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous() for t in (preds, labels))
    B, K = preds.shape
    dev = preds.device
    if totals is None:
        totals = concept_totals(len(topk), dev)
    if totals[0].numel() != len(topk) + 1 or totals[0].dtype != torch.float64 or totals[1].numel() != 2 or totals[1].dtype != torch.int64:
        raise ValueError("`totals` must be the pair of concept_totals({}, device)".format(len(topk)))
    ap = torch.empty(B, device=dev, dtype=torch.float64)
    hits = torch.empty(B, len(topk), device=dev, dtype=torch.int32)
    n_pos = torch.empty(B, device=dev, dtype=torch.int32)
    # (a single row may carry any stride: it is never used)
    _lib.call("care_concept_metrics", _lib.ptr(preds), max(preds.stride(0), K), _lib.ptr(labels), max(labels.stride(0), K), B, K,
              (ctypes.c_int32 * len(topk))(*topk), len(topk),
              _lib.ptr(ap), _lib.ptr(hits), _lib.ptr(n_pos), _lib.ptr(totals[0]), _lib.ptr(totals[1]), tag="concept_metrics")
    return (totals, {"ap": ap, "hits": hits, "n_pos": n_pos}) if per_clip else totals


def concept_scores(totals_d, totals_i, topk=TOPK_LIST) -> Dict[str, float]:
    """{"F1-05": .., "mAP": .., "n_no_positive": ..} of totals READ BACK (lists or host tensors): the sums over the clip count.
    A NaN (a clip without a positive, counted in n_no_positive) is the one object `math.nan`, so that two epochs' score dicts
    with the same numbers compare equal."""
    n = int(totals_i[0])
    d = [(float(x) / n if x == x else math.nan) if n else 0 for x in totals_d]
    out = {"F1-%02d" % k: d[i] for i, k in enumerate(topk)}
    out["mAP"] = d[len(topk)]
    out["n_no_positive"] = int(totals_i[1])
    return out


def language_metrics(logp: torch.Tensor, pred: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
    labels = labels.to(pred.device)
    mask = labels.ne(PAD)
    n = float(mask.sum())
    acc = float(((pred.long() == labels) & mask).sum()) / n
    ce = float(-(logp * mask).sum()) / n
    return {"Word Acc0": acc, "Perplexity": math.exp(ce), "n_words": n}


def concept_metrics(preds_attr: torch.Tensor, labels_attr: torch.Tensor, calculate_mAP: bool = True) -> Dict[str, float]:
    preds = torch.clamp(preds_attr.float(), 0.01, 0.99)
    labels = labels_attr[:, : preds.shape[1]].to(preds.device).float()
    out = {}
    _, cand = preds.topk(max(TOPK_LIST), dim=1, sorted=True, largest=True)
    n_pos = labels.sum(1)
    for k in TOPK_LIST:
        hit = labels.gather(1, cand[:, :k]).sum(1)
        hit[hit.eq(0)] = 1e-3
        precision, recall = hit / k, hit / n_pos
        out["F1-%02d" % k] = float((2 * precision * recall / (precision + recall)).mean())
    if calculate_mAP:
        _, idx = preds.sort(dim=1, descending=True)
        _, rank = idx.sort(dim=1)
        aps = []
        for i in range(labels.shape[0]):
            pos = labels[i].nonzero().squeeze(1)
            hit_rank, _ = rank[i][pos].sort()
            ids = torch.arange(len(pos), device=pos.device)
            aps.append(float(((ids + 1).float() / (hit_rank + 1)).mean()))
        out["mAP"] = sum(aps) / len(aps)
    return out

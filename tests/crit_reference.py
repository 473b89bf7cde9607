"""The tests' own restatement of the reference's training criteria in plain torch (any dtype, any device) - the yardstick of
tests/test_criterion_cpu.py (pinned there to the recorded reference, tests/golden/crit) and of tests/test_gpu_criterion.py.
Formulas: misc/Crit/crit_lang.py:49-71,75-103, misc/Crit/crit_attribute.py:38-48, misc/Crit/base.py:39-47,95."""
import glob
import json
import math
import os

import numpy as np
import torch

CRIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crit")
PAD = 0


def crit_cases(kind):
    out = []
    for p in sorted(glob.glob(os.path.join(CRIT_DIR, "*.npz"))):
        if str(np.load(p)["kind"]) == kind:
            out.append(os.path.basename(p)[:-4])
    return out


def load_case(name):
    return np.load(os.path.join(CRIT_DIR, name + ".npz"))


def lang_rows(logits, labels, eps):
    """Per label position: (row loss, log-prob of the label, arg-max, lse); logits [N, t or t + 1, V], labels [N, t]."""
    if logits.size(1) == labels.size(1) + 1:
        logits = logits[:, :-1, :]
    assert logits.size(1) == labels.size(1)
    lsm = torch.log_softmax(logits, dim=-1)
    logp = lsm.gather(2, labels.unsqueeze(2)).squeeze(2)
    row = (1 - eps) * -logp + eps * -lsm.mean(dim=-1)
    return row, logp, lsm.max(-1)[1], torch.logsumexp(logits, dim=-1)


def lang_step(logits, labels, eps):
    """LanguageGeneration._step: the sum over the non-PAD positions."""
    row, _, _, _ = lang_rows(logits, labels, eps)
    return (row * labels.ne(PAD).to(row.dtype)).sum()


def lang_counts(logits, labels):
    """(hits, words, sum of -logp over the words)."""
    _, logp, pred, _ = lang_rows(logits, labels, 0.0)
    mask = labels.ne(PAD)
    return int(((pred == labels) & mask).sum()), int(mask.sum()), float(-(logp * mask).sum())


def bce_rows(preds, labels):
    """NoisyOrMIL._step per clip: (row loss, denominator)."""
    # (the reference clamps fp32 tensors: its bounds are fp32's 0.01 and 0.99, also when this runs in float64 - an entry equal
    # to fp32's 0.01 is inside the clamp and gets its gradient)
    lo, hi = float(torch.tensor(0.01, dtype=torch.float32)), float(torch.tensor(0.99, dtype=torch.float32))
    p = torch.clamp(preds, lo, hi)
    y = labels[:, : p.shape[1]].to(p.dtype)
    den = torch.clamp(y.sum(1), min=1.0)
    return -(y * torch.log(p) + (1.0 - y) * torch.log(1.0 - p)).sum(1) / den, den


def bce_step(preds, labels):
    return bce_rows(preds, labels)[0].sum()


def total_loss(out, labels, labels_attr, eps, scales=(1.0, 1.0)):
    """Criterion.get_loss for crits ['lang'] or ['lang', 'attribute']: each step's sum over its batch size, scaled, added."""
    lg = out["logits"]
    loss = scales[0] * lang_step(lg, labels, eps) / float(lg.size(0))
    if labels_attr is not None:
        pa = out["preds_attr"].reshape(lg.size(0), -1)
        loss = loss + scales[1] * bce_step(pa, labels_attr) / float(pa.size(0))
    return loss


def info_of_batches(batches, eps, scales_unused=None):
    """get_loss_info() of get_criterion(['lang', 'attribute']) after the given batches [(logits, labels, preds, labels_attr)]
    in float64: AverageMeter sums weighted by the sample count (base.py:95), accuracy over words, exp(mean -logp)."""
    from care_amd.metrics import TOPK_LIST, concept_metrics

    n = sum_l = sum_a = hits = words = nlogp = 0.0
    f1 = {k: 0.0 for k in TOPK_LIST}
    aps = []
    for logits, labels, preds, labels_attr in batches:
        B = logits.shape[0]
        n += B
        sum_l += float(lang_step(logits.double(), labels, eps))
        sum_a += float(bce_step(preds.double(), labels_attr))
        h, w, s = lang_counts(logits.double(), labels)
        hits, words, nlogp = hits + h, words + w, nlogp + s
        c = concept_metrics(preds, labels_attr, calculate_mAP=True)
        for k in TOPK_LIST:
            f1[k] += c["F1-%02d" % k] * B
        aps.append((c["mAP"], B))
    info = {"Lang Loss": sum_l / n, "V-Attr": sum_a / n, "Word Acc0": hits / words, "Perplexity": math.exp(nlogp / words)}
    info.update({"F1-%02d" % k: f1[k] / n for k in TOPK_LIST})
    info["mAP"] = sum(a * b for a, b in aps) / n
    return info


def criterion_batches(z):
    return [tuple(torch.from_numpy(z["b%d_%s" % (b, k)]) for k in ("logits", "labels", "preds_attr", "labels_attr")) for b in (0, 1)]


def criterion_opt(z):
    from care_amd.configs import make_opt

    return make_opt(str(z["config"]), **json.loads(str(z["overrides"])))

"""Record tests/golden/crit/*.npz: the genuine reference's training criteria on small inputs (CPU).

    python tools/gen_crit_golden.py

Runs misc/Crit's own LanguageGeneration, NoisyOrMIL and get_criterion (imported through oracle.ref_import) and stores, per
case, the inputs, the loss and its denominator, get_info(), and the reference autograd's d loss / d logits and
d loss / d preds_attr - data only.  tests/test_criterion_cpu.py pins a float64 restatement to these files,
tests/test_gpu_criterion.py pins care_amd.criterion to them.  The inputs come from seeded torch generators, so a re-run
rewrites the same files.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "crit")

K_ATTR = 500


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lang_inputs(seed, N, t_logits, t_labels, V, lengths):
    """logits [N, t_logits, V] ~ 3 N(0, 1) - c; labels [N, t_labels]: lengths[i] words in [1, V), then PAD (0)."""
    g = _gen(seed)
    logits = torch.randn(N, t_logits, V, generator=g) * 3.0
    # centred so that log-sum-exp is near 0: the reference's fp32 log_softmax rounds at one ulp of lse, which at lse ~ 12 is the
    # 1e-6 these fixtures are pinned to float64 at (tests/test_criterion_cpu.py)
    logits -= torch.logsumexp(logits, dim=-1).mean()
    labels = torch.zeros(N, t_labels, dtype=torch.int64)
    # Labels of a wide vocabulary come from its last 256 columns.  The reference's fp32 autograd sums the V gradient terms of a
    # row (eps / V each, 1 - eps at the label) in log_softmax's backward; every term added after the label's rounds the same way
    # at one ulp of 1 - eps, so its error against float64 grows with the number of columns behind the label - 2e-6 of the
    # largest gradient at V = 2003 with the label in front, 1e-7 with it near the end.  A fixture pins a float64 restatement to
    # the reference at 1e-6, so it has to be one the reference itself computes to better than that.
    lo = 1 if V <= 1024 else V - 256
    for i, n in enumerate(lengths):
        labels[i, :n] = torch.randint(lo, V, (n,), generator=g)
    # one position where the label IS the arg-max and one where it is not, whatever the seed (word accuracy strictly in (0, 1))
    labels[0, 0] = max(int(logits[0, 0, lo:].argmax()) + lo, 1)
    logits[0, 0, labels[0, 0]] = logits[0, 0].max() + 0.5
    if int(logits[1, 0].argmax()) == int(labels[1, 0]):
        labels[1, 0] = 1 + (int(labels[1, 0]) % (V - 1))
    return logits, labels


def attr_inputs(seed, B, Kl, empty_clip=None):
    """preds_attr [B, 500] in (0, 1) with entries below 0.01 and above 0.99 (both sides of the clamp, some exactly on it);
    labels [B, Kl > 500] multi-hot (positives also in the unused columns); `empty_clip` has no positive.

    The clamp makes 41 probabilities EQUAL at each end, and in which order a sort or top-k returns equal entries is the
    implementation's choice (the CPU's and the GPU's differ).  So without `empty_clip` (where F1@k / mAP are compared) all of
    the top group are positives and all of the bottom group negatives: the hits among the first k and the positives' set of
    ranks are then the same in any order.  With `empty_clip` (F1@k / mAP are NaN anyway) both groups hold both labels."""
    g = _gen(seed)
    preds = 0.02 + 0.95 * torch.rand(B, K_ATTR, generator=g)   # (0.02, 0.97): no column outside the two groups reaches the clamp
    preds[:, 0:40] = torch.rand(B, 40, generator=g) * 0.02          # many below 0.01
    preds[:, 40:80] = 1.0 - torch.rand(B, 40, generator=g) * 0.02   # many above 0.99
    preds[:, 80], preds[:, 81] = 0.01, 0.99          # on the clamp's ends: the gradient passes (torch.clamp's rule)
    labels = (torch.rand(B, Kl, generator=g) > 0.95).float()
    if empty_clip is not None:
        labels[:, 3], labels[:, 45] = 1.0, 1.0       # positives inside both clamped ranges
        labels[empty_clip, :K_ATTR] = 0.0
    else:
        labels[:, 0:40], labels[:, 80] = 0.0, 0.0
        labels[:, 40:80], labels[:, 81] = 1.0, 1.0
    return preds, labels


def main():
    from oracle.ref_import import import_reference

    import_reference()
    from misc.Crit import get_criterion
    from misc.Crit.crit_attribute import NoisyOrMIL
    from misc.Crit.crit_lang import LanguageGeneration

    from care_amd.configs import make_opt

    os.makedirs(OUT, exist_ok=True)
    written = []

    def save(name, **arrays):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        written.append((name, os.path.getsize(path)))

    # ---- LanguageGeneration: eps 0 and 0.1 on the same inputs
    lang_cases = [
        ("lang_v131", dict(seed=101, N=3, t_logits=6, t_labels=6, V=131, lengths=[2, 1, 3])),          # mostly PAD
        ("lang_v2003", dict(seed=102, N=2, t_logits=5, t_labels=5, V=2003, lengths=[4, 2])),
        ("lang_v131_drop_last", dict(seed=103, N=3, t_logits=7, t_labels=6, V=131, lengths=[6, 2, 1])),  # t_logits = t_labels + 1
    ]
    for name, kw in lang_cases:
        logits, labels = lang_inputs(**kw)
        eps_list, losses, infos, grads, dens = [0.0, 0.1], [], [], [], []
        for eps in eps_list:
            crit = LanguageGeneration({"label_smoothing": eps})
            crit.reset_recorder()
            x = logits.clone().requires_grad_(True)
            loss, den = crit({"logits": x, "labels": labels})
            loss.backward()
            losses.append(float(loss.detach()))
            dens.append(den)
            names, info = crit.get_info()
            assert names == ["Word Acc0", "Perplexity"]
            infos.append(info)
            grads.append(x.grad.numpy())
        save(name, kind="lang", logits=logits.numpy(), labels=labels.numpy(), eps=np.asarray(eps_list), loss=np.asarray(losses),
             denominator=np.asarray(dens), info=np.asarray(infos, dtype=np.float64), dlogits=np.stack(grads))

    # ---- NoisyOrMIL (calculate_mAP on): every clip with positives; one clip without (the reference's F1 / mAP are NaN there)
    for name, kw in (("attr_b3", dict(seed=201, B=3, Kl=520)), ("attr_b3_no_positive", dict(seed=202, B=3, Kl=507, empty_clip=1))):
        preds, labels = attr_inputs(**kw)
        crit = NoisyOrMIL({"calculate_mAP": True})
        crit.reset_recorder()
        x = preds.clone().requires_grad_(True)
        loss, den = crit({"preds_attr": x, "avg_prob_attr": x.mean(1), "labels_attr": labels})
        loss.backward()
        names, info = crit.get_info()
        save(name, kind="attr", preds_attr=preds.numpy(), labels_attr=labels.numpy(), loss=np.asarray(float(loss.detach())),
             denominator=np.asarray(den), info_names=json.dumps(names), info=np.asarray(info, dtype=np.float64),
             dpreds=x.grad.numpy())

    # ---- get_criterion(['lang', 'attribute']) over two successive batches of different size: the recorders' weighting
    over = dict(label_smoothing=0.1, language_generation_scale=0.8, attribute_prediction_scales=[0.3])
    opt = make_opt("msrvtt_care", **over)
    criterion = get_criterion(opt, override_opt={"calculate_mAP": True})
    criterion.reset_loss_recorder()
    arrays, losses = {}, []
    for b, (N, t, lengths, seed) in enumerate(((3, 6, [3, 1, 2], 301), (2, 5, [4, 2], 302))):
        logits, labels = lang_inputs(seed, N, t, t, 131, lengths)
        preds, labels_attr = attr_inputs(seed + 50, N, 520)
        x, p = logits.clone().requires_grad_(True), preds.clone().requires_grad_(True)
        loss = criterion.get_loss({"logits": x, "labels": labels, "preds_attr": p, "avg_prob_attr": p.mean(1), "labels_attr": labels_attr})
        loss.backward()
        losses.append(float(loss.detach()))
        arrays.update({"b%d_logits" % b: logits.numpy(), "b%d_labels" % b: labels.numpy(), "b%d_preds_attr" % b: preds.numpy(),
                       "b%d_labels_attr" % b: labels_attr.numpy(), "b%d_dlogits" % b: x.grad.numpy(), "b%d_dpreds" % b: p.grad.numpy()})
    info = criterion.get_loss_info()
    save("criterion_two_batches", kind="criterion", config="msrvtt_care", overrides=json.dumps(over), names=json.dumps(criterion.names),
         scales=np.asarray(criterion.scales, dtype=np.float64), loss=np.asarray(losses), info_json=json.dumps(info), **arrays)

    for name, size in written:
        print("{:32s} {:7d} bytes".format(name, size))


if __name__ == "__main__":
    main()

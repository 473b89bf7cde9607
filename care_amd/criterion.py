"""The training criteria on HIP kernels: `misc/Crit` of the reference behind the same interface.

    from care_amd.criterion import get_criterion          # instead of `from misc.Crit import get_criterion`
    criterion = get_criterion(opt)                        # Wrapper.py:417
    criterion.reset_loss_recorder()                       # before an epoch
    loss = criterion.get_loss({**model(batch), "labels": labels, "labels_attr": labels_attr})   # Wrapper.py:423-435
    loss.backward()
    criterion.get_loss_info()                             # after the epoch: {'Lang Loss': .., 'V-Attr': .., 'Word Acc0': .., ...}

* `LanguageGeneration` (crit_lang.py): label-smoothed NLL of the teacher-forced logits with the PAD mask, word accuracy and
  perplexity - care_lang_loss_fwd / care_lang_loss_bwd (csrc/loss.hip): the [N, t, V] logits are read once forward, once
  backward, PAD rows not at all; nothing of the size of the logits is allocated except their gradient.
* `NoisyOrMIL` (crit_attribute.py): BCE of the clamped concept probabilities over the number of positives, F1@k, mAP -
  care_noisy_or_bce_fwd / _bwd; F1@k / mAP with care_amd/metrics.py's formulas.
* `Criterion` (base.py:50-113): scales, sums and records them.

Both losses are torch.autograd.Functions, so `loss.backward()` feeds training.py's `_Linear.backward` of the vocabulary head
and of the concept head unchanged.

NO HOST SYNCHRONISATION in `get_loss`: where the reference calls `.item()` three times a step (accuracy, perplexity, the loss
recorder), the kernels add into a few doubles on the device; `get_loss_info()` reads them, once.  A label outside [0, V) is
never dereferenced; it is counted, and `get_loss_info()` raises ValueError with the count.

As everywhere in care_amd there is no CPU fallback: CPU tensors raise.  What the kernels do not cover is refused by name
(NotImplementedError): visual_word_generation, a `probs` entry, attribute_prediction_flags other than 'V',
attribute_prediction_sparse_sampling, prefix / pp guidance, crits other than lang / attribute.
"""
import copy
import math
from typing import Dict, List, Optional, Tuple, Union

import torch

from ._lib import call, ptr
from .constants import PAD
from .metrics import TOPK_LIST

__all__ = ["get_criterion", "Criterion", "CritBase", "LanguageGeneration", "NoisyOrMIL"]


def _need_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError("`{}` must be a tensor, got {}".format(what, type(t).__name__))
    if t.device.type != "cuda":
        raise RuntimeError("`{}` is on `{}`: the criteria run on the MI355X (there is no CPU fallback)".format(what, t.device))


def _rows_f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 with unit stride in the last dimension (the kernels take any leading dimension)."""
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.stride(-1) == 1 else t.contiguous()


class _LangLoss(torch.autograd.Function):
    """sum over the non-PAD label positions of (1 - eps) NLL + eps (lse - mean x) (crit_lang.py:57-71)."""

    @staticmethod
    def forward(ctx, logits, labels32, eps, acc):
        N, tl, V = logits.shape
        t = labels32.shape[1]
        # whole sequences at one stride, rows at another: [N, t + 1, V] is walked in place, its last position skipped
        if logits.stride(2) != 1 or logits.stride(1) < V or logits.stride(0) < t * logits.stride(1):
            logits = logits.contiguous()
        rows, dev = N * t, logits.device
        stats = torch.empty(5, rows, device=dev, dtype=torch.float32)   # lse, max, log sum exp(x - max), logp, row_loss
        pred = torch.empty(rows, device=dev, dtype=torch.int32)
        sums = torch.empty(2, device=dev, dtype=torch.float32)
        counts = torch.empty(3, device=dev, dtype=torch.int32)
        call("care_lang_loss_fwd", ptr(logits), logits.stride(1), logits.stride(0), t, V, ptr(labels32), eps, ptr(stats[0]),
             ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(pred), ptr(stats[4]), ptr(sums), ptr(counts), ptr(acc), rows)
        ctx.save_for_backward(logits, labels32, stats)
        ctx.eps = eps
        pred = pred.view(N, t)
        ctx.mark_non_differentiable(pred, counts)
        return sums[0], pred, counts

    @staticmethod
    def backward(ctx, g, _gp, _gc):
        logits, labels32, stats = ctx.saved_tensors
        N, tl, V = logits.shape
        t = labels32.shape[1]
        g = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernel reads it, the host never does
        d = torch.empty(N, tl, V, device=logits.device, dtype=torch.float32)
        call("care_lang_loss_bwd", ptr(logits), logits.stride(1), logits.stride(0), t, V, ptr(labels32), ptr(stats[1]), ptr(stats[2]), ctx.eps,
             ptr(g), ptr(d), V, tl * V, tl, N * t)
        return d, None, None, None


class _NoisyOrBCE(torch.autograd.Function):
    """sum over clips of -sum_c (y log p + (1 - y) log(1 - p)) / max(1, sum_c y), p = clamp(preds, 0.01, 0.99)."""

    @staticmethod
    def forward(ctx, preds, labels, acc):
        B, K = preds.shape
        dev = preds.device
        rl = torch.empty(2, B, device=dev, dtype=torch.float32)   # row_loss, denom
        sums = torch.empty(1, device=dev, dtype=torch.float32)
        call("care_noisy_or_bce_fwd", ptr(preds), preds.stride(0), ptr(labels), labels.stride(0), ptr(rl[0]), ptr(rl[1]), ptr(sums),
             ptr(acc), B, K)
        ctx.save_for_backward(preds, labels, rl)
        return sums[0]

    @staticmethod
    def backward(ctx, g):
        preds, labels, rl = ctx.saved_tensors
        B, K = preds.shape
        g = g.to(torch.float32).reshape(1).contiguous()
        d = torch.empty(B, K, device=preds.device, dtype=torch.float32)
        call("care_noisy_or_bce_bwd", ptr(preds), preds.stride(0), ptr(labels), labels.stride(0), ptr(rl[1]), ptr(g), ptr(d), K, B, K)
        return d, None, None


class CritBase(object):
    """misc/Crit/base.py:6-47 for one source per key (lists of sources belong to visual word generation, refused)."""

    def __init__(self, keys: List[str], weights: Union[List[float], float] = 1.0, batch_mean: bool = True):
        self.keys = keys
        self.weights = weights
        self.batch_mean = batch_mean

    def _step(self, index_indicator, *inputs) -> torch.Tensor:
        raise NotImplementedError()

    def __call__(self, kwargs: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, float]:
        src1, src2, *others = [kwargs.get(key, None) for key in self.keys]
        if isinstance(src1, (list, tuple)) or isinstance(src2, (list, tuple)):
            raise NotImplementedError("a list under `{}` / `{}` (several sources for one criterion: visual_word_generation) "
                                      "is not covered".format(self.keys[0], self.keys[1]))
        weight = self.weights[0] if isinstance(self.weights, list) else self.weights
        self._refuse(src1, src2, *others)
        _need_device(src1, self.keys[0])
        denominator = float(src1.size(0)) if self.batch_mean else 1.0
        loss = weight * self._step(0, src1, src2, *others) / denominator
        return loss, denominator

    def _refuse(self, *inputs) -> None:
        """Inputs this criterion does not cover raise NotImplementedError here, before anything runs."""

    # the device side of the recorders: a few doubles the kernels add into
    def device_state(self) -> Optional[torch.Tensor]:
        return getattr(self, "acc", None)

    def loss_sum(self, state) -> float:
        """sum over the calls since the reset of the step's loss (= loss * number of samples), from the state read back."""
        return float(state[0]) if state is not None else 0.0


class LanguageGeneration(CritBase):
    def __init__(self, opt):
        if opt.get("visual_word_generation", False):
            raise NotImplementedError("`visual_word_generation` (crit_lang.py:11-15: two logit sources, a second accuracy) "
                                      "is not covered by the HIP criteria")
        if opt.get("use_attr", False) and any(k in opt.get("use_attr_type", "") for k in ("prefix", "pp")):
            raise NotImplementedError("use_attr_type `{}`: prefix / pp guidance (crit_lang.py:43-48) is not covered by the HIP "
                                      "criteria".format(opt.get("use_attr_type")))
        super().__init__(keys=["logits", "labels", "probs"], weights=1.0)
        self.num_word_acc = 1
        self.label_smoothing = float(opt.get("label_smoothing", 0.0))   # opts.py:249: default 0
        self.ignore_index = PAD
        self.opt = opt
        self.reset_recorder()

    def _refuse(self, logits, labels, probs=None, *others):
        if probs is not None:
            raise NotImplementedError("a `probs` entry (crit_lang.py:39-40,54-55: log of given probabilities instead of "
                                      "log_softmax) is not covered by the HIP criteria")

    def _step(self, index_indicator, logits, labels, probs=None, *others):
        assert not len(others)
        assert logits.dim() == 3 and labels.dim() == 2 and logits.size(0) == labels.size(0)
        if logits.size(1) != labels.size(1) + 1:      # crit_lang.py:49-52
            assert logits.size(1) == labels.size(1), (tuple(logits.shape), tuple(labels.shape))
        labels32 = labels.to(device=logits.device, dtype=torch.int32).contiguous()
        if self.acc is None:
            self.acc = torch.zeros(5, device=logits.device, dtype=torch.float64)
        loss, pred, counts = _LangLoss.apply(_rows_f32(logits), labels32, self.label_smoothing, self.acc)
        self.last_pred, self.last_counts = pred, counts   # arg-max tokens [N, t]; (hits, words, bad labels) of this call
        return loss

    def get_fieldsnames(self):
        return ["Word Acc%d" % i for i in range(self.num_word_acc)] + ["Perplexity"]

    def get_info(self, state=None):
        """state: the device doubles read back by the caller (Criterion.get_loss_info reads every criterion's in one copy)."""
        if state is None and self.acc is not None:
            state = self.acc.cpu().tolist()
        if state is None:
            return self.get_fieldsnames(), [0, math.exp(0)]
        _, nlogp, hits, words, bad = state
        if bad > 0:
            raise ValueError("{} label(s) outside [0, vocab_size) since the last reset: their rows were left out of the loss".format(int(bad)))
        acc = hits / words if words else 0
        return self.get_fieldsnames(), [acc, math.exp(nlogp / words if words else 0)]

    def reset_recorder(self):
        self.acc = None
        self.last_pred = self.last_counts = None


class NoisyOrMIL(CritBase):
    def __init__(self, opt, keys=None):
        if opt.get("attribute_prediction_sparse_sampling", False):
            raise NotImplementedError("`attribute_prediction_sparse_sampling` (crit_attribute.py:22-23,51-56: the L1 term on "
                                      "avg_prob_attr) is not covered; training mode refuses that branch of the concept head too")
        super().__init__(keys=["preds_attr", "avg_prob_attr", "labels_attr"] if keys is None else keys, batch_mean=True)
        self.topk_list = list(TOPK_LIST)
        self.calculate_mAP = opt.get("calculate_mAP", False)
        self.acc = None

    def _step(self, index_indicator, preds_attr, avg_prob_attr, labels_attr, *others):
        assert not len(others)
        assert preds_attr.dim() == 2 and preds_attr.shape[1] <= labels_attr.shape[1]
        preds = _rows_f32(preds_attr)
        labels = _rows_f32(labels_attr.to(preds.device))      # [B, Kl >= K]: the kernels use the first K columns in place
        B, K = preds.shape
        if self.acc is None:
            self.acc = torch.zeros(1 + len(self.topk_list), device=preds.device, dtype=torch.float64)
        loss = _NoisyOrBCE.apply(preds, labels, self.acc)
        if hasattr(self, "f1_count"):   # (as in the reference: metrics only once reset_recorder() has been called)
            with torch.no_grad():
                p = torch.clamp(preds.detach(), 0.01, 0.99)
                y = labels[:, :K]
                _, cand = p.topk(max(self.topk_list), dim=1, sorted=True, largest=True)
                n_pos = y.sum(1)
                f1s = []
                for k in self.topk_list:   # metrics.concept_metrics' formulas, summed on the device
                    hit = y.gather(1, cand[:, :k]).sum(1)
                    hit = torch.where(hit.eq(0), torch.full_like(hit, 1e-3), hit)
                    precision, recall = hit / k, hit / n_pos
                    f1s.append((2 * precision * recall / (precision + recall)).sum())
                self.acc[1:] += torch.stack(f1s).double()
                self.f1_count += B
                if self.calculate_mAP:
                    self.ap_pending.append((p, y))
        return loss

    def get_fieldsnames(self, prefix=""):
        return ["%sF1-%02d" % (prefix, item) for item in self.topk_list] + (["%smAP" % prefix] if hasattr(self, "ap_pending") else [])

    def _mean_ap(self) -> float:
        """crit_attribute.py:72-86 over the batches since the reset (the row loop runs here, not inside the step)."""
        aps = []
        for p, y in self.ap_pending:
            _, idx = p.sort(dim=1, descending=True)
            _, rank = idx.sort(dim=1)
            rank, y = rank.cpu(), y.cpu()
            for i in range(y.shape[0]):
                pos = y[i].nonzero().squeeze(1)
                hit_rank, _ = rank[i][pos].sort()
                ids = torch.arange(len(pos))
                aps.append(float(((ids + 1).float() / (hit_rank + 1)).mean()))
        return sum(aps) / len(aps) if aps else 0

    def get_info(self, state=None):
        if not hasattr(self, "f1_count"):
            raise AttributeError("NoisyOrMIL.get_info() before reset_recorder()")
        if state is None and self.acc is not None:
            state = self.acc.cpu().tolist()
        f1 = [s / self.f1_count for s in state[1:]] if (state is not None and self.f1_count) else [0] * len(self.topk_list)
        return self.get_fieldsnames(), f1 + ([self._mean_ap()] if hasattr(self, "ap_pending") else [])

    def reset_recorder(self):
        self.acc = None
        self.f1_count = 0
        if self.calculate_mAP:
            self.ap_pending = []


class Criterion(object):
    """misc/Crit/base.py:50-113.  reset_loss_recorder() before an epoch, get_loss(results) per step, get_loss_info() after."""

    def __init__(self, crit_objects, names, scales):
        assert len(crit_objects) == len(names)
        assert len(names) == len(scales)
        self.crit_objects = crit_objects
        self.num_loss = len(crit_objects)
        self.names = names
        self.scales = scales
        self.n_current_round = 0
        self.reset_loss_recorder()

    def set_scales(self, new_scales):
        assert len(new_scales) == len(self.scales)
        self.scales = new_scales

    def reset_loss_recorder(self):
        self.loss_count = [0.0 for _ in range(self.num_loss)]
        for crit_object in self.crit_objects:
            if getattr(crit_object, "reset_recorder", None) is not None:
                crit_object.reset_recorder()

    def get_loss(self, results, **kwargs):
        loss = []
        for i in range(self.num_loss):
            assert isinstance(self.crit_objects[i], CritBase)
            i_loss, num_samples = self.crit_objects[i](results)
            loss.append(i_loss * self.scales[i])
            # (base.py:95 `update(i_loss.item(), num_samples)`: the kernel has added i_loss * num_samples on the device)
            self.loss_count[i] += num_samples
        return torch.stack(loss, dim=0).sum(0)

    def get_loss_info(self):
        # ONE copy to the host for every criterion's device doubles
        states = [c.device_state() for c in self.crit_objects]
        live = [s for s in states if s is not None]
        host = torch.cat(live).cpu().tolist() if live else []
        split, at = [], 0
        for s in states:
            split.append(None if s is None else host[at: at + s.numel()])
            at += 0 if s is None else s.numel()
        all_names = self.names.copy()
        all_info = []
        for c, st, n in zip(self.crit_objects, split, self.loss_count):   # AverageMeter.avg, weighted by sample count
            all_info.append(c.loss_sum(st) / n if n else 0)
        for c, st in zip(self.crit_objects, split):
            if getattr(c, "get_info", None) is not None:
                this_name, this_info = c.get_info(st)
                all_names += this_name
                all_info += this_info
        return {n: i for n, i in zip(all_names, all_info)}


def _crit_info_lang(opt):
    return [LanguageGeneration(opt)], ["Lang Loss"], [opt.get("language_generation_scale", 1.0)]


def _crit_info_attribute(opt):
    """prepare.py:17-52 for the visual flag `V` (the other flags score decoder states: NoisyOrMILWithEmbs, not covered)."""
    scales = opt.get("attribute_prediction_scales", 1.0)
    flags = opt["attribute_prediction_flags"]
    if not isinstance(scales, list):
        scales = [scales]
    elif len(scales) == 1:
        scales = scales * len(flags)
    else:
        assert len(scales) == len(flags), "#scales {} vs. #flags {}".format(len(scales), len(flags))
    objects, names = [], []
    for flag in flags:
        if flag != "V":
            raise NotImplementedError("attribute_prediction_flags `{}`: only 'V' (NoisyOrMIL on preds_attr) is covered by the HIP "
                                      "criteria, not flag '{}' (NoisyOrMILWithEmbs)".format(flags, flag))
        names.append("{}-Attr".format(flag))
        objects.append(NoisyOrMIL(opt))
    return objects, names, scales


_CRIT_INFO = {"lang": _crit_info_lang, "attribute": _crit_info_attribute}


def get_criterion(opt, skip_crit_list=[], override_opt={}):
    """misc/Crit/__init__.py:22-64."""
    if len(override_opt):
        _opt = copy.deepcopy(opt)
        _opt.update(override_opt)
    else:
        _opt = opt
    assert isinstance(_opt["crits"], list)
    crit_objects, names, scales = [], [], []
    for crit in [item for item in _opt["crits"] if item not in skip_crit_list]:
        if crit not in _CRIT_INFO:
            raise NotImplementedError("crit `{}`: the HIP criteria cover {} only".format(crit, sorted(_CRIT_INFO)))
        objs, nms, scs = _CRIT_INFO[crit](_opt)
        assert len(objs) == len(nms) == len(scs), "(object_func, name, scale) of {} do not have the same number of elements".format(crit)
        crit_objects.extend(objs)
        names.extend(nms)
        scales.extend(scs)
    if not len(crit_objects):
        return None
    return Criterion(crit_objects=crit_objects, names=names, scales=scales)

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
  With `model.set_fused_head(True)` (default off) the model hands over a `DeferredLogits` - the decoder's hidden states and
  the head's weight - instead of logits, and `_HeadLoss` runs the vocabulary projection (Head.py:26-32), the same loss, its
  metrics and its backward over the LIVE label positions only (about a quarter of a batch of captions): no [rows, V] fp32
  tensor exists at any point.  The head's products are then ALWAYS split products of pre-scaled fp16 hi / lo pieces (the
  `fp16x3` form of training.py), whatever TRAIN_GEMM says for the other layers.  Labels on the host (a loader's batch) are
  counted before their copy, so `get_loss` stays free of host synchronisation; for labels already on the device the count
  of live rows - 4 bytes - is read back: the one exception.
* `NoisyOrMIL` (crit_attribute.py): BCE of the clamped concept probabilities over the number of positives, F1@k, mAP -
  care_noisy_or_bce_fwd / _bwd; F1@k / mAP by care_concept_metrics (csrc/concept_metrics.hip) into the recorder's device
  doubles: no sort, no top-k, nothing kept between steps; equal probabilities rank by column.
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
from .metrics import TOPK_LIST, concept_metrics_device

__all__ = ["get_criterion", "Criterion", "CritBase", "LanguageGeneration", "NoisyOrMIL", "DeferredLogits", "head_chunks"]


def _need_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, (torch.Tensor, DeferredLogits)):
        raise TypeError("`{}` must be a tensor, got {}".format(what, type(t).__name__))
    if t.device.type != "cuda":
        raise RuntimeError("`{}` is on `{}`: the criteria run on the MI355X (there is no CPU fallback)".format(what, t.device))


def _rows_f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 with unit stride in the last dimension (the kernels take any leading dimension)."""
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.stride(-1) == 1 else t.contiguous()


def _seq_rows(logits: torch.Tensor, t: int):
    """Logits [N, t (+ 1), V] as the row kernels address them (csrc/vocab_row.h): whole sequences at one stride, rows at
    another, so [N, t + 1, V] is walked in place with its last position skipped; any other layout is made contiguous.
    Returns the logits to keep for the backward and the leading arguments of the four entry points
    (logits, ld, seq_stride, rows_per_seq, V)."""
    V = logits.shape[2]
    if logits.stride(2) != 1 or logits.stride(1) < V or logits.stride(0) < t * logits.stride(1):
        logits = logits.contiguous()
    return logits, (ptr(logits), logits.stride(1), logits.stride(0), t, V)


def _seq_rows_grad(logits: torch.Tensor, t: int):
    """For the backward, on the logits `_seq_rows` returned: a contiguous gradient [N, tl, V] (the kernels write every row of
    it), the same leading arguments, and the trailing ones of the two backward entry points
    (dlogits, ldd, dseq_stride, seq_rows, rows)."""
    N, tl, V = logits.shape
    d = torch.empty(N, tl, V, device=logits.device, dtype=torch.float32)
    return d, _seq_rows(logits, t)[1], (ptr(d), V, tl * V, tl, N * t)


class _LangLoss(torch.autograd.Function):
    """sum over the non-PAD label positions of (1 - eps) NLL + eps (lse - mean x) (crit_lang.py:57-71)."""

    @staticmethod
    def forward(ctx, logits, labels32, eps, acc):
        N, t = logits.shape[0], labels32.shape[1]
        logits, src = _seq_rows(logits, t)
        rows, dev = N * t, logits.device
        stats = torch.empty(5, rows, device=dev, dtype=torch.float32)   # lse, max, log sum exp(x - max), logp, row_loss
        pred = torch.empty(rows, device=dev, dtype=torch.int32)
        sums = torch.empty(2, device=dev, dtype=torch.float32)
        counts = torch.empty(3, device=dev, dtype=torch.int32)
        call("care_lang_loss_fwd", *src, ptr(labels32), eps, ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(pred),
             ptr(stats[4]), ptr(sums), ptr(counts), ptr(acc), rows)
        ctx.save_for_backward(logits, labels32, stats)
        ctx.eps = eps
        pred = pred.view(N, t)
        ctx.mark_non_differentiable(pred, counts)
        return sums[0], pred, counts

    @staticmethod
    def backward(ctx, g, _gp, _gc):
        logits, labels32, stats = ctx.saved_tensors
        t = labels32.shape[1]
        g = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernel reads it, the host never does
        d, src, dst = _seq_rows_grad(logits, t)
        call("care_lang_loss_bwd", *src, ptr(labels32), ptr(stats[1]), ptr(stats[2]), ctx.eps, ptr(g), *dst)
        return d, None, None, None


class DeferredLogits(object):
    """The logits a training forward with `set_fused_head(True)` did NOT compute: the decoder's hidden states [N, t, d] (an
    autograd tensor, after the final dropout) and `cls_head.tgt_word_prj.weight` [V, d].  LanguageGeneration runs head and loss
    fused on it (_HeadLoss); any other consumer calls `.materialize()` for the ordinary logits."""

    def __init__(self, hidden: torch.Tensor, weight: torch.Tensor):
        if hidden.dim() != 3 or weight.dim() != 2 or hidden.shape[2] != weight.shape[1]:
            raise ValueError("hidden [N, t, d] and weight [V, d] expected, got {} and {}".format(tuple(hidden.shape), tuple(weight.shape)))
        self.hidden, self.weight = hidden, weight

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.hidden.shape[0], self.hidden.shape[1], self.weight.shape[0]))

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self) -> int:
        return 3

    @property
    def device(self) -> torch.device:
        return self.hidden.device

    def materialize(self) -> torch.Tensor:
        """[N, t, V] logits through training.py's `_Linear` (differentiable like the unfused head's)."""
        from .training import _Linear
        N, t, d = self.hidden.shape
        return _Linear.apply(self.hidden.reshape(N * t, d), self.weight, None).view(N, t, -1)

    def __repr__(self):
        return "DeferredLogits(shape={}, device={})".format(tuple(self.shape), self.device)


# Live rows per pass of the fused head's backward: the gradient's fp16 pieces (8 bytes per live row and vocabulary column:
# [R, 2 ks] and its transpose) are allocated per chunk, so they stay bounded at any batch; dW adds up over the chunks in order.
# *Measured* on one MI355X (tools/loss_bench.py --head --chunk-rows 0,4096,2048; 512 clips = 3931 live rows; head + both criteria,
# forward + backward, median of 5 windows, min .. max): whole 1.830 ms (1.775 .. 1.991), 4096 1.777 ms (1.764 .. 1.983) - one chunk
# at this batch, the same launches as whole -, 2048 2.233 ms (2.166 .. 2.378): a second pass splits W's pieces again and leaves
# each product half the tiles.  4096: a batch of 512 clips in one pass, 8 x 4096 x 10560 = 346 MB of pieces at most beyond it.
HEAD_CHUNK_ROWS = 4096


def head_chunks(live_rows: int, chunk: Optional[int] = None) -> List[Tuple[int, int]]:
    """[(first, end), ...] of the live rows in chunks of at most `chunk` (HEAD_CHUNK_ROWS) rows, in order; none for 0 rows."""
    chunk = HEAD_CHUNK_ROWS if chunk is None else chunk
    if chunk <= 0:
        raise ValueError("chunk rows must be positive, got {}".format(chunk))
    return [(a, min(a + chunk, live_rows)) for a in range(0, max(live_rows, 0), chunk)]


def _ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


def _head_forward(hidden2d, W, labels32, eps, acc, live=None):
    """The forward of _HeadLoss on h [N * tl, d], W [V, d], labels [N, t] (tl >= t: positions past the labels are dead).
    Returns (sums [2], pred [N * t], counts [3], stats [5, N * t] = lse, max, log sum exp(x - max), logp, row loss per
    position (zeros at dead ones), saved): every sum in a fixed order, nothing of the size [rows, V]."""
    from .training import _absmax_slot, _f32c
    N, t = labels32.shape
    d, V = hidden2d.shape[1], W.shape[0]
    tl = hidden2d.shape[0] // N
    assert hidden2d.shape[0] == N * tl and tl >= t and W.shape[1] == d, (tuple(hidden2d.shape), tuple(W.shape), (N, t))
    h, Wc = _f32c(hidden2d), _f32c(W)
    dev, rows = h.device, N * t
    idx = torch.empty(3, rows, device=dev, dtype=torch.int32)       # live row -> row of h, label position, label
    cnt = torch.empty(2, device=dev, dtype=torch.int32)
    call("care_head_live_rows", ptr(labels32), N, t, tl, V, ptr(idx[0]), ptr(idx[1]), ptr(idx[2]), ptr(cnt))
    R = int(cnt[0].item()) if live is None else int(live)           # device labels: the one 4-byte read-back
    stats = torch.zeros(5, rows, device=dev, dtype=torch.float32)
    pred = torch.zeros(rows, device=dev, dtype=torch.int32)
    sums = torch.empty(2, device=dev, dtype=torch.float32)
    counts = torch.empty(3, device=dev, dtype=torch.int32)
    saved = None
    if R > 0:   # (an all-PAD batch launches nothing with M = 0)
        h_live = torch.empty(R, d, device=dev, dtype=torch.float32)
        call("care_gather_rows", ptr(h), h.stride(0) * 4, ptr(h_live), d * 4, ptr(idx[0]), R, d * 4)
        ksd, parts = _ceil64(d), (V + 63) // 64
        h_slot, w_slot = _absmax_slot(h_live), _absmax_slot(Wc)
        a2 = torch.empty(R, 2 * ksd, device=dev, dtype=torch.float16)
        w3 = torch.empty(V, 3 * ksd, device=dev, dtype=torch.float16)
        call("care_split_pieces", ptr(h_live), d, R, d, 0, 1, ksd, ptr(a2), 2, h_slot.data_ptr())
        call("care_split_pieces", ptr(Wc), Wc.stride(0), V, d, 0, 1, ksd, ptr(w3), 3, w_slot.data_ptr())
        cst = torch.empty(2, R, device=dev, dtype=torch.float32)    # max, log sum exp(x - max) per LIVE row: the backward's
        for a, b in head_chunks(R):
            n = b - a
            pf = torch.empty(4, n, parts, device=dev, dtype=torch.float32)
            pi = torch.empty(n, parts, device=dev, dtype=torch.int32)
            call("care_gemm_tile_split3_head_stats", ptr(a2[a:]), ptr(w3), h_slot.data_ptr(), w_slot.data_ptr(), ptr(idx[2][a:]),
                 ptr(pf[0]), ptr(pi), ptr(pf[1]), ptr(pf[2]), ptr(pf[3]), n, V, ksd)
            call("care_head_loss_finish", ptr(pf[0]), ptr(pi), ptr(pf[1]), ptr(pf[2]), ptr(pf[3]), parts, ptr(idx[2][a:]),
                 ptr(idx[1][a:]), V, eps, n, ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(pred), ptr(stats[4]),
                 ptr(cst[0][a:]), ptr(cst[1][a:]))
        # W's pieces (6 bytes per weight) are not kept for the backward: split again there from the same |max| - the same bits
        saved = (h_live, Wc, a2, idx, cst, h_slot, w_slot)
    call("care_lang_loss_reduce", ptr(stats[4]), ptr(stats[3]), ptr(pred), ptr(labels32), V, rows, ptr(sums), ptr(counts), ptr(acc))
    return sums, pred, counts, stats, R, saved


class _HeadLoss(torch.autograd.Function):
    """_LangLoss with the vocabulary head inside (Head.py:26-32 + crit_lang.py:49-71): hidden2d [N * tl, d], W [V, d] ->
    (loss, pred [N, t], counts); backward -> (dhidden [N * tl, d] with dead rows exactly zero, dW [V, d]).  `live`: the number
    of live label positions when the host knows it (labels counted before their copy); None: read back from the device."""

    @staticmethod
    def forward(ctx, hidden2d, W, labels32, eps, acc, live=None):
        N, t = labels32.shape
        sums, pred, counts, _, R, saved = _head_forward(hidden2d, W, labels32, eps, acc, live)
        ctx.R, ctx.eps, ctx.h_shape, ctx.w_shape = R, eps, tuple(hidden2d.shape), tuple(W.shape)
        if saved is not None:
            ctx.save_for_backward(*saved)
        pred = pred.view(N, t)
        ctx.mark_non_differentiable(pred, counts)
        return sums[0], pred, counts

    @staticmethod
    def backward(ctx, g, _gp, _gc):
        from .training import _strided_sum, _x3_slabs
        (rows_h, d), (V, _) = ctx.h_shape, ctx.w_shape
        R, eps, dev = ctx.R, ctx.eps, g.device
        need_dh, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)   # (a fill kernel, not a memset node)
        if R == 0:
            return (zeros(rows_h, d) if need_dh else None), (zeros(V, d) if need_dw else None), None, None, None, None
        h_live, Wc, a2, idx, cst, h_slot, w_slot = ctx.saved_tensors
        g32 = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernels read it, the host never does
        gslot = torch.empty(1, device=dev, dtype=torch.int32)
        call("care_head_grad_scale", ptr(g32), gslot.data_ptr())
        ksd, ksv = _ceil64(d), _ceil64(V)
        dh_live = torch.empty(R, d, device=dev, dtype=torch.float32) if need_dh else None
        plan = [(a, b, _x3_slabs(V, d, b - a)) for a, b in head_chunks(R)]
        terms = sum(s for _, _, s in plan)
        dw_terms, at = None, 0
        for a, b, slabs in plan:
            # one buffer of the size of W's pieces or of the chunk's at a time: W's pieces in either orientation are split per
            # chunk (a sweep of W - microseconds against the chunk's products) and dropped before the next buffer is taken
            n = b - a
            w3 = torch.empty(V, 3 * ksd, device=dev, dtype=torch.float16)
            call("care_split_pieces", ptr(Wc), Wc.stride(0), V, d, 0, 1, ksd, ptr(w3), 3, w_slot.data_ptr())
            dl2 = torch.empty(n, 2 * ksv, device=dev, dtype=torch.float16)
            call("care_gemm_tile_split3_head_grad", ptr(a2[a:]), ptr(w3), h_slot.data_ptr(), w_slot.data_ptr(), ptr(idx[2][a:]),
                 ptr(cst[0][a:]), ptr(cst[1][a:]), ptr(g32), gslot.data_ptr(), eps, ptr(dl2), n, V, ksd)
            del w3
            if need_dh:   # dh = dl W: W^T as the [d, V] operand, pieces with the forward's |max| of W
                wt3 = torch.empty(d, 3 * ksv, device=dev, dtype=torch.float16)
                call("care_split_pieces", ptr(Wc), Wc.stride(0), d, V, 1, 1, ksv, ptr(wt3), 3, w_slot.data_ptr())
                call("care_gemm_tile_split3_scaled", ptr(dl2), ptr(wt3), None, ptr(dh_live[a:]), d, n, d, ksv, gslot.data_ptr(),
                     w_slot.data_ptr(), 1)
                del wt3
            if need_dw:   # dW = dl^T h: the reduction runs over the chunk's rows, in slabs when the output has few tiles
                ksr = _ceil64((n + slabs - 1) // slabs)
                dlt = torch.empty(slabs * V, 2 * ksr, device=dev, dtype=torch.float16)
                call("care_pieces_transpose", ptr(dl2), n, V, ksv, slabs, ksr, ptr(dlt))
                del dl2
                if dw_terms is None:   # (taken here, not up front: W's pieces and dl's are gone by now - the peak stays at the pieces)
                    dw_terms = torch.empty(terms * V, d, device=dev, dtype=torch.float32)
                ht3 = torch.empty(slabs * d, 3 * ksr, device=dev, dtype=torch.float16)
                call("care_split_pieces", ptr(h_live[a:]), d, d, n, 1, slabs, ksr, ptr(ht3), 3, h_slot.data_ptr())
                call("care_gemm_tile_split3_scaled", ptr(dlt), ptr(ht3), None, ptr(dw_terms[at * V:]), d, V, d, ksr, gslot.data_ptr(),
                     h_slot.data_ptr(), slabs)
                at += slabs
                del dlt, ht3
        dW = None
        if need_dw:   # slabs and chunks added in order: one grouping, the same bits every time
            dW = dw_terms if terms == 1 else _strided_sum(dw_terms, V, terms, 1, V)
        dhid = None
        if need_dh:
            dhid = zeros(rows_h, d)
            call("care_scatter_rows", ptr(dh_live), d * 4, ptr(dhid), d * 4, ptr(idx[0]), R, d * 4)
        return dhid, dW, None, None, None, None


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
        live = None
        if isinstance(logits, DeferredLogits) and labels.device.type == "cpu":   # a loader's batch: counted before the copy
            live = int(((labels > 0) & (labels < logits.size(2))).sum())
        labels32 = labels.to(device=logits.device, dtype=torch.int32).contiguous()
        if self.acc is None:
            self.acc = torch.zeros(5, device=logits.device, dtype=torch.float64)
        if isinstance(logits, DeferredLogits):   # set_fused_head(True): head + loss over the live label positions
            hidden = logits.hidden
            loss, pred, counts = _HeadLoss.apply(hidden.reshape(hidden.shape[0] * hidden.shape[1], hidden.shape[2]), logits.weight,
                                                 labels32, self.label_smoothing, self.acc, live)
        else:
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
        self.acc = self.acc_clips = None

    def _step(self, index_indicator, preds_attr, avg_prob_attr, labels_attr, *others):
        assert not len(others)
        assert preds_attr.dim() == 2 and preds_attr.shape[1] <= labels_attr.shape[1]
        preds = _rows_f32(preds_attr)
        labels = _rows_f32(labels_attr.to(preds.device))      # [B, Kl >= K]: the kernels use the first K columns in place
        B, K = preds.shape
        if self.acc is None:   # the loss, sum F1@k for each k, sum AP; beside them the kernel's (clips, clips without a positive)
            self.acc = torch.zeros(2 + len(self.topk_list), device=preds.device, dtype=torch.float64)
            self.acc_clips = torch.zeros(2, device=preds.device, dtype=torch.int64)
        loss = _NoisyOrBCE.apply(preds, labels, self.acc)
        if hasattr(self, "f1_count"):   # (as in the reference: metrics only once reset_recorder() has been called)
            # F1@k and AP of every clip and their sums in ONE call (csrc/concept_metrics.hip): acc[1:] = sum F1@k .., sum AP
            concept_metrics_device(preds, labels, self.topk_list, totals=(self.acc[1:], self.acc_clips))
            self.f1_count += B
        return loss

    def get_fieldsnames(self, prefix=""):
        return ["%sF1-%02d" % (prefix, item) for item in self.topk_list] + (["%smAP" % prefix] if getattr(self, "ap_on", False) else [])

    def get_info(self, state=None):
        if not hasattr(self, "f1_count"):
            raise AttributeError("NoisyOrMIL.get_info() before reset_recorder()")
        if state is None and self.acc is not None:
            state = self.acc.cpu().tolist()
        n = len(self.topk_list)
        avg = [s / self.f1_count for s in state[1:]] if (state is not None and self.f1_count) else [0] * (n + 1)
        return self.get_fieldsnames(), avg[:n] + ([avg[n]] if self.ap_on else [])

    def reset_recorder(self):
        self.acc = self.acc_clips = None
        self.f1_count = 0
        self.ap_on = bool(self.calculate_mAP)


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

"""The validation epoch on the MI355X: decode a split, score it where it lies, read the result once.

    from care_amd import MetricBank, ValidationEpoch
    bank = MetricBank(refs, vocab_size, video_ids=names)          # the references of the validation split
    scores = ValidationEpoch(opt, captioner, bank).run(loader)    # {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr", "Sum", ...}

The validation-side counterpart of SelfCriticalStep and InterplayStep - what `Wrapper.validation_epoch_end` -> `evaluation()`
(models/Wrapper.py:214-273) computes for `--monitor_metric` / `--lr_monitor_metric`, METEOR apart.  Per batch: the greedy decode
(HipEngine.translate_greedy) or the beam search (translate_beam) and the caption translate_batch would return first
(care_beam_winner: the best normalised score, the earliest among equals), the caption's statistics and CIDEr
(MetricBank.score) and their addition into the epoch's totals (MetricBank.accumulate) - all on the engine's stream, behind one
another, so the engine's workspaces are consumed before the next decode overwrites them.  No token, length or score is read on
the host during the epoch; `run` ends with ONE read of 15 words.

A captioner with a concept head whose batches carry `labels_attr` (ClipStore's validate batches do) is also scored as the
reference's eval criterion scores it (models/Wrapper.py:182-184, :421: get_criterion(opt, skip_crit_list=['lang'],
override_opt={'calculate_mAP': True})): the decode's own `preds_attr` - in eval mode the one `feedforward_step` would produce -
goes through care_concept_metrics and care_noisy_or_bce_fwd into totals of their own beside the state, in the same
`engine.lock` section; the scores gain `mAP` (Wrapper.py:245-248), `F1-05` .. `F1-50`, `V-Attr Loss` and `n_no_positive`, for
one more read at the epoch's end.  Without a concept head or without `labels_attr`: nothing new, no launch and no key.

A resident launch that gives up reports non-positive lengths; such rows count as invalid.  If the epoch ends with any, it is
run once more with the resident decodes switched off (the Translator's own retry, applied to the epoch), and the Translator's
error is raised if rows are still without a caption.

What it does not do: ensembles, METEOR, and the split of a validation set over ranks - the twelve integer totals
and the two sums simply add across ranks, which is the one exchange that would need.
"""
import torch

from . import _lib
from .capmetrics import METRIC_SUM, TOTALS, MetricBank, check_metric_sum
from .metrics import TOPK_LIST, concept_metrics_device, concept_scores, concept_totals
from .framework import TransformerSeq2Seq
from .translator import Translator_ARFormer

__all__ = ["ValidationEpoch"]


class ValidationEpoch(object):
    """A `captioner` (one care_amd framework module) and the `MetricBank` of the split it is validated on.  beam_size /
    beam_alpha default to `opt`'s, as the Translator takes them (5 and 1.0 without); beam_size 1 is the greedy decode."""

    def __init__(self, opt, captioner, bank, beam_size=None, beam_alpha=None, metric_sum=METRIC_SUM):
        if isinstance(captioner, (list, tuple)):
            raise NotImplementedError("an ensemble of {} captioners: the validation epoch takes ONE model".format(len(captioner)))
        if not isinstance(bank, MetricBank):
            raise TypeError("`bank` must be a care_amd.MetricBank, got {}".format(type(bank).__name__))
        if not isinstance(captioner, TransformerSeq2Seq):
            raise TypeError("`captioner` must be a care_amd framework module with an inference engine (get_framework), got {}: a "
                            "module that only runs in training mode cannot decode".format(type(captioner).__name__))
        self.metric_sum = check_metric_sum(metric_sum)   # (a set METEOR flag is refused here, by name)
        over = dict(opt)
        if beam_size is not None:
            over["beam_size"] = beam_size
        if beam_alpha is not None:
            over["beam_alpha"] = beam_alpha
        self.translator = Translator_ARFormer(over)      # (refuses a beam_size translate_batch does not accept, and holds len_pow)
        self.opt, self.captioner, self.bank = opt, captioner, bank
        self.beam_size, self.beam_alpha = int(self.translator.beam_size), self.translator.beam_alpha
        self._len_pow = None
        self.concept = None   # the concept totals of the last accumulate(): (doubles [n_topk + 1], int64 [2], loss double [1])
        self.last = {}

    # ------------------------------------------------------------------ one batch: decode, score, accumulate
    def _decode(self, engine, feats):
        """(tokens int32 [B, <= 64] without BOS, length int32 [B]) of the caption translate_batch returns first, on the device,
        and the encoder's outputs of the pass."""
        T = engine.T
        if self.beam_size == 1:
            enc, fed, length, _ = engine.translate_greedy(feats, use_graph=False, early_exit=False)
            return fed[:, 1: T + 1], length, enc
        need = max(self.beam_size, int(self.translator.topk))
        enc, nfin, fscore, flen, fhyp = engine.translate_beam(feats, self.beam_size, need, use_graph=False, early_exit=False)
        B, cap, w = fhyp.shape
        if self._len_pow is None or self._len_pow.device != fhyp.device:
            self._len_pow = torch.from_numpy(self.translator._len_pow).to(fhyp.device)
        tokens = torch.empty(B, w, dtype=torch.int32, device=fhyp.device)
        length = torch.empty(B, dtype=torch.int32, device=fhyp.device)
        _lib.call("care_beam_winner", _lib.ptr(nfin), _lib.ptr(fscore), _lib.ptr(flen), _lib.ptr(fhyp), B, cap, w,
                  _lib.ptr(self._len_pow), self._len_pow.numel(), _lib.ptr(tokens), _lib.ptr(length), tag="beam_winner")
        return tokens, length, enc

    def _score_concepts(self, enc, labels_attr):
        """F1@k / AP of the batch's `preds_attr` and the eval criterion's BCE (crit_attribute.py:38-48, :58-89) into the
        epoch's concept totals: three small launches, nothing read."""
        preds = enc["preds_attr"]
        labels = labels_attr.to(preds.device)
        labels = labels if labels.dtype == torch.float32 else labels.float()
        labels = labels if labels.stride(-1) == 1 else labels.contiguous()
        B, K = preds.shape
        if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] < K:
            raise ValueError("`labels_attr` {} for concept probabilities {}".format(tuple(labels.shape), (B, K)))
        if self.concept is None:
            self.concept = concept_totals(len(TOPK_LIST), preds.device) + (torch.zeros(1, dtype=torch.float64, device=preds.device),)
        concept_metrics_device(preds, labels, TOPK_LIST, totals=self.concept[:2])
        rl = torch.empty(2, B, device=preds.device, dtype=torch.float32)
        sums = torch.empty(1, device=preds.device, dtype=torch.float32)
        _lib.call("care_noisy_or_bce_fwd", _lib.ptr(preds), preds.stride(0), _lib.ptr(labels), labels.stride(0), _lib.ptr(rl[0]),
                  _lib.ptr(rl[1]), _lib.ptr(sums), _lib.ptr(self.concept[2]), B, K, tag="concept_bce")

    def _pass(self, model, batches, state):
        engine = model.engine()
        if engine.T + 1 > 64:
            raise ValueError("max_len {}: care_caption_stats holds captions of 64 tokens".format(engine.T + 1))
        if engine.T != self.translator.max_len - 1:
            raise ValueError("translator max_len {} != model max_len {}".format(self.translator.max_len, engine.T + 1))
        for batch in batches:
            if "video_ids" not in batch:
                raise KeyError("the batch has no `video_ids`: a caption is scored against its own clip's references")
            feats = list(batch["feats"])
            if feats and isinstance(feats[0], (list, tuple)):
                raise NotImplementedError("one feature list per model is an ensemble's batch: the validation epoch takes ONE model")
            if any(f.device.type != "cuda" for f in feats):
                raise RuntimeError("the features are on the CPU: the validation epoch runs on the MI355X (no CPU fallback)")
            with engine.lock:
                video = self.bank.rows(batch["video_ids"])
                if video.numel() != feats[0].shape[0]:
                    raise ValueError("{} `video_ids` for {} clips".format(video.numel(), feats[0].shape[0]))
                tokens, length, enc = self._decode(engine, feats)
                self.bank.accumulate(self.bank.score(tokens, length, video), state[:TOTALS])
                state[TOTALS] += (length <= 0).sum()   # rows a resident launch gave up on (on the device, like the rest)
                if batch.get("labels_attr") is not None and "preds_attr" in enc:   # a concept head and its labels
                    self._score_concepts(enc, batch["labels_attr"])

    def accumulate(self, batches, resident: bool = True) -> torch.Tensor:
        """Decodes and scores `batches` and returns the epoch's state - int64 [15] on the device: MetricBank's totals and the
        number of rows that came back without a caption - WITHOUT reading anything on the host.  resident False: with the
        resident decodes switched off.  The model is put into eval mode and comes back as it was.  The concept totals of the
        pass (None when nothing was scored) are `self.concept`, zero at the start of every call like the state."""
        if self.bank.desc is None:
            raise RuntimeError("the bank was built with device=None (host tables only): the validation epoch runs on the MI355X")
        model = self.captioner
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad(), model._on_device():
                engine = model.engine()
                keep = engine.resident_max_rows, engine.resident_beam_max_rows
                if not resident:
                    engine.resident_max_rows = engine.resident_beam_max_rows = 0
                try:
                    state = torch.zeros(TOTALS + 1, dtype=torch.int64, device=self.bank.device)
                    self.concept = None
                    self._pass(model, batches, state)
                finally:
                    engine.resident_max_rows, engine.resident_beam_max_rows = keep
        finally:
            model.train(was_training)
        return state

    def scores(self, state: torch.Tensor):
        """(MetricBank.scores' dict, rows without a caption) of an epoch's state: the ONE host read - and one more, of 10
        doubles, when the epoch scored concepts: `mAP`, `F1-05` .. `F1-50`, `V-Attr Loss` (the sum of the clips' BCE over the
        clip count: base.py:95's batch-mean recorder) and `n_no_positive` (clips whose F1 / AP are NaN) join the scores."""
        host = state.cpu()
        scores = self.bank.scores(host[:TOTALS], self.metric_sum)
        if self.concept is not None:
            d, i, loss = self.concept
            c = torch.cat([d, loss, i.double()]).cpu().tolist()   # (counts below 2^53: exact as doubles)
            n = len(TOPK_LIST)
            scores.update(concept_scores(c[:n + 1], [int(c[n + 2]), int(c[n + 3])], TOPK_LIST))
            scores["V-Attr Loss"] = c[n + 1] / c[n + 2] if c[n + 2] else 0
        return scores, int(host[TOTALS])

    def run(self, batches) -> dict:
        """The scores of the epoch over `batches` (dicts with `feats` on the device and `video_ids`): MetricBank.scores' dict of
        Python floats."""
        if iter(batches) is batches:
            batches = list(batches)   # (a one-shot iterator: the retry below needs the batches again)
        scores, gave_up = self.scores(self.accumulate(batches))
        if gave_up > 0:   # a resident launch gave up: once more through the multi-launch decodes, which need no co-residency
            scores, gave_up = self.scores(self.accumulate(batches, resident=False))
        if gave_up > 0:
            raise _lib.CareHipError(Translator_ARFormer._ABORTED)
        if scores["n_invalid"] > 0:
            raise ValueError("{} clips have no references: their `video_ids` lie outside the bank or name a video without "
                             "captions".format(int(scores["n_invalid"])))
        self.last = scores
        return scores

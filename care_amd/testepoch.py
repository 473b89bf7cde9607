"""The test epoch on the MI355X: decode a split, score it, keep every caption's record and analyse the captions where they lie.

    from care_amd import CorpusBank, MetricBank, TestEpoch
    bank = MetricBank(refs, vocab_size, video_ids=names)             # the references of the test split
    corpus = CorpusBank(train_captions, vocab_size)                  # every training caption, ids without BOS / EOS
    epoch = TestEpoch(opt, captioner, bank, corpus)
    scores, detail_scores, pred_captions = epoch.run(loader, vocab=itow)
    epoch.write_predictions("preds.json"); epoch.write_detail_scores("detail.json")

The counterpart of `translate.py` -> `run_eval` -> `Wrapper.test_epoch_end` (models/Wrapper.py:75-149), METEOR apart: the corpus
scores of ValidationEpoch, plus
    `detail_scores[video_id]` = {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr"} of the clip's own caption (COCOScorer.imgToEval),
    the caption analysis `ave_length`, `novel`, `unique`, `usage` (care_amd/corpusstats.py) and the `opt` keys added by name,
    `pred_captions[video_id]` = [{"image_id", "caption", "score"}] (Wrapper.translate_step, :206-210).
It IS a ValidationEpoch (a subclass; validation.py is untouched): per batch the same decode and `MetricBank.score`, then plain
device copies of the batch's stats / rouge / cider / bank row / model score (care_caption_model_score) into epoch-sized
arrays, `EpochCaptions.insert` (which also keeps the cut tokens and lengths), and `MetricBank.accumulate` as before - all on the
engine's stream, nothing read per batch.

Host reads of one pass over the split: THREE - ValidationEpoch's 15 words, the 8 words of the analysis, and one bulk read of the
per-caption arrays (one byte buffer).  An epoch that scored concepts adds ValidationEpoch's read of 10 doubles.

A caption in `pred_captions` and in the analysis is the row cut at the first EOS or PAD - `to_sentence`'s words; with `vocab`
(id -> word) they are joined with blanks, without it the caption is the list of ids.  The per-sentence BLEU is
capmetrics.corpus_scores' arithmetic on the caption's own record, row by row in Python floats (its `**` and `exp` are the
reference's: a numpy power may differ in the last bit); ROUGE_L and CIDEr are the stored values.

Refused by name: ensembles, `topk` > 1 (the reference skips scoring then), a set METEOR flag, CPU tensors, an epoch larger than
`capacity`, a CorpusBank whose vocab_size differs from the MetricBank's.  `--save_csv` is a pandas call on `scores` and stays
with the caller.
"""
import json
import math

import numpy as np
import torch

from . import _lib
from .capmetrics import METRIC_SUM, REC, SMALL, TINY, TOTALS
from .corpusstats import CorpusBank, EpochCaptions
from .reward import MAX_CAPTION, ORDERS
from .translator import Translator_ARFormer
from .validation import ValidationEpoch

__all__ = ["TestEpoch", "sentence_scores"]

def sentence_scores(stats, rouge, cider) -> list:
    """One {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr"} per row of `stats` (int [rows, 12], care_caption_stats' records): coco-caption's
    per-sentence BLEU - the corpus formula with the row's own (testlen, reflen, guess, correct) - in Python floats."""
    out = []
    for rec, r, c in zip(np.asarray(stats).tolist(), np.asarray(rouge, dtype=np.float64).tolist(), np.asarray(cider).tolist()):
        testlen, reflen, guess, correct = rec[1], rec[2], rec[3:7], rec[7:11]
        bleu, bleus = 1.0, []
        for k in range(ORDERS):
            bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
            bleus.append(bleu ** (1.0 / (k + 1)))
        ratio = (testlen + TINY) / (reflen + SMALL)
        if ratio < 1:
            bleus = [b * math.exp(1 - 1 / ratio) for b in bleus]
        d = {"Bleu_%d" % (k + 1): bleus[k] for k in range(ORDERS)}
        d["ROUGE_L"], d["CIDEr"] = float(r), float(c)
        out.append(d)
    return out


def _pow2_at_least(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


class TestEpoch(ValidationEpoch):
    """A `captioner`, the `MetricBank` of the split it is tested on and the `CorpusBank` of the training captions.
    capacity: the largest number of clips of an epoch (the per-caption arrays; the caption set gets the next power of two of
    twice as many slots, so that its probe chains stay short).  beam_size / beam_alpha / metric_sum as ValidationEpoch takes them."""
    __test__ = False   # (not a test class, whatever its name says to a test collector)

    def __init__(self, opt, captioner, bank, corpus, capacity: int = 4096, beam_size=None, beam_alpha=None, metric_sum=METRIC_SUM):
        super().__init__(opt, captioner, bank, beam_size=beam_size, beam_alpha=beam_alpha, metric_sum=metric_sum)
        if not isinstance(corpus, CorpusBank):
            raise TypeError("`corpus` must be a care_amd.CorpusBank, got {}".format(type(corpus).__name__))
        if int(self.translator.topk) > 1:
            raise NotImplementedError("topk {} > 1: the reference's test epoch skips scoring when a clip has several captions "
                                      "(Wrapper.py:106-112); use translate_batch for those".format(self.translator.topk))
        if corpus.vocab_size != bank.vocab_size:
            raise ValueError("the corpus bank's vocab_size {} != the metric bank's {}: build both over the same ids".format(
                corpus.vocab_size, bank.vocab_size))
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError("`capacity` must be a positive integer, got {!r}".format(capacity))
        self.corpus, self.capacity = corpus, capacity
        self.captions = None     # EpochCaptions, built with the first pass (on the bank's device)
        self.arrays = None       # the epoch-sized device arrays of the per-caption records
        self.count = 0           # captions of the pass so far (a host integer: every batch's row count is known)
        self.last_detail, self.last_predictions = {}, {}

    # ------------------------------------------------------------------ the epoch's device state
    def _begin(self):
        if self.corpus.desc is None:
            raise RuntimeError("the corpus bank was built with device=None (host tables only): the test epoch runs on the MI355X")
        if self.captions is None:
            dev, n = self.bank.device, self.capacity
            self.captions = EpochCaptions(_pow2_at_least(2 * n), self.bank.vocab_size, self.corpus)
            self.arrays = {"stats": torch.zeros(n, REC, dtype=torch.int32, device=dev), "rouge": torch.zeros(n, dtype=torch.float64, device=dev),
                           "cider": torch.zeros(n, dtype=torch.float32, device=dev), "video": torch.zeros(n, dtype=torch.int32, device=dev),
                           "score": torch.zeros(n, dtype=torch.float64, device=dev)}
        self.captions.reset()
        self.count = 0

    def _decode(self, engine, feats):
        """ValidationEpoch._decode, and the model's score of the returned caption (double [B], on the device) in
        `self._model_score`: score / length ** alpha, the division translate_batch does on the host."""
        if self._len_pow is None or self._len_pow.device != feats[0].device:
            self._len_pow = torch.from_numpy(self.translator._len_pow).to(feats[0].device)
        pw = self._len_pow
        T = engine.T
        if self.beam_size == 1:
            enc, fed, length, score = engine.translate_greedy(feats, use_graph=False, early_exit=False)
            B = length.numel()
            out = torch.empty(B, dtype=torch.float64, device=length.device)
            _lib.call("care_caption_model_score", None, _lib.ptr(score.contiguous()), _lib.ptr(length.contiguous()), B, 1, _lib.ptr(pw),
                      pw.numel(), _lib.ptr(out), tag="caption_model_score")
            self._model_score = out
            return fed[:, 1: T + 1], length, enc
        need = max(self.beam_size, int(self.translator.topk))
        enc, nfin, fscore, flen, fhyp = engine.translate_beam(feats, self.beam_size, need, use_graph=False, early_exit=False)
        B, cap, w = fhyp.shape
        tokens = torch.empty(B, w, dtype=torch.int32, device=fhyp.device)
        length = torch.empty(B, dtype=torch.int32, device=fhyp.device)
        out = torch.empty(B, dtype=torch.float64, device=fhyp.device)
        _lib.call("care_beam_winner", _lib.ptr(nfin), _lib.ptr(fscore), _lib.ptr(flen), _lib.ptr(fhyp), B, cap, w, _lib.ptr(pw),
                  pw.numel(), _lib.ptr(tokens), _lib.ptr(length), tag="beam_winner")
        _lib.call("care_caption_model_score", _lib.ptr(nfin), _lib.ptr(fscore), _lib.ptr(flen), B, cap, _lib.ptr(pw), pw.numel(),
                  _lib.ptr(out), tag="caption_model_score")
        self._model_score = out
        return tokens, length, enc

    def _pass(self, model, batches, state):
        """ValidationEpoch._pass with the batch's records kept: the same checks, decode, score and accumulate."""
        engine = model.engine()
        if engine.T + 1 > MAX_CAPTION:
            raise ValueError("max_len {}: care_caption_stats holds captions of 64 tokens".format(engine.T + 1))
        if engine.T != self.translator.max_len - 1:
            raise ValueError("translator max_len {} != model max_len {}".format(self.translator.max_len, engine.T + 1))
        self._begin()
        for batch in batches:
            if "video_ids" not in batch:
                raise KeyError("the batch has no `video_ids`: a caption is scored against its own clip's references")
            feats = list(batch["feats"])
            if feats and isinstance(feats[0], (list, tuple)):
                raise NotImplementedError("one feature list per model is an ensemble's batch: the test epoch takes ONE model")
            if any(f.device.type != "cuda" for f in feats):
                raise RuntimeError("the features are on the CPU: the test epoch runs on the MI355X (no CPU fallback)")
            B = feats[0].shape[0]
            if self.count + B > self.capacity:
                raise ValueError("{} clips after {}: the epoch is larger than its capacity {}".format(B, self.count, self.capacity))
            with engine.lock:
                video = self.bank.rows(batch["video_ids"])
                if video.numel() != B:
                    raise ValueError("{} `video_ids` for {} clips".format(video.numel(), B))
                tokens, length, enc = self._decode(engine, feats)
                rec = self.bank.score(tokens, length, video)
                lo, hi = self.count, self.count + B
                for k, src in (("stats", rec["stats"]), ("rouge", rec["rouge"]), ("cider", rec["cider"]), ("video", video),
                               ("score", self._model_score)):
                    self.arrays[k][lo:hi].copy_(src)
                self.captions.insert(tokens, length)
                self.count = hi
                self.bank.accumulate(rec, state[:TOTALS])
                state[TOTALS] += (length <= 0).sum()
                if batch.get("labels_attr") is not None and "preds_attr" in enc:
                    self._score_concepts(enc, batch["labels_attr"])

    # ------------------------------------------------------------------ the end of the epoch
    def _fetch_records(self) -> dict:
        """The per-caption arrays of the pass on the host: ONE read of one byte buffer."""
        n, a, c = self.count, self.arrays, self.captions
        parts = [("stats", a["stats"][:n], np.int32, (n, REC)), ("rouge", a["rouge"][:n], np.float64, (n,)),
                 ("cider", a["cider"][:n], np.float32, (n,)), ("video", a["video"][:n], np.int32, (n,)),
                 ("score", a["score"][:n], np.float64, (n,)), ("length", c.length[:n], np.int32, (n,)),
                 ("tokens", c.tokens[:n], np.int32, (n, MAX_CAPTION))]
        blob = torch.cat([t.contiguous().view(-1).view(torch.uint8) for _, t, _, _ in parts]).cpu().numpy()
        out, off = {}, 0
        for name, t, dtype, shape in parts:
            size = t.numel() * t.element_size()
            out[name] = blob[off: off + size].view(dtype).reshape(shape)
            off += size
        return out

    def _video_names(self, rows) -> list:
        row_of = self.bank.cider._row_of
        if row_of is None:
            return [int(v) for v in rows]
        names = [None] * len(row_of)
        for name, i in row_of.items():
            names[i] = name
        return [names[int(v)] for v in rows]

    def _refuse(self, batches) -> None:
        """What can be seen from the batches alone is refused before anything runs: an ensemble's batch, features on the CPU,
        more clips than `capacity` (`_pass` holds every batch to the same rules as it comes)."""
        total = 0
        for batch in batches:
            feats = list(batch.get("feats") or ()) if isinstance(batch, dict) else []
            if feats and isinstance(feats[0], (list, tuple)):
                raise NotImplementedError("one feature list per model is an ensemble's batch: the test epoch takes ONE model")
            if any(isinstance(f, torch.Tensor) and f.device.type != "cuda" for f in feats):
                raise RuntimeError("the features are on the CPU: the test epoch runs on the MI355X (no CPU fallback)")
            total += int(feats[0].shape[0]) if feats else 0
        if total > self.capacity:
            raise ValueError("{} clips: the epoch is larger than its capacity {}".format(total, self.capacity))

    def run(self, batches, vocab=None, keys_added_to_scores=("seed",)):
        """(scores, detail_scores, pred_captions) of the epoch over `batches` (dicts with `feats` on the device and `video_ids`),
        like Wrapper.test_epoch_end.  scores: ValidationEpoch.run's dict, `ave_length` / `novel` / `unique` / `usage` and
        opt[key] for every key of `keys_added_to_scores` (a list or tuple joined with '-', Wrapper.py:114-119).  vocab: id ->
        word for the captions of `pred_captions`; None leaves them as lists of ids.  Three host reads at the end of the pass
        (see the module's docstring), none per batch.  Every call starts from zero."""
        added = {}
        for key in keys_added_to_scores:
            value = self.opt[key]
            added[key] = "-".join(str(item) for item in value) if isinstance(value, (tuple, list)) else value
        if iter(batches) is batches:
            batches = list(batches)   # (a one-shot iterator: the retry below needs the batches again)
        self._refuse(batches)
        scores, gave_up = self.scores(self.accumulate(batches))
        if gave_up > 0:   # a resident launch gave up: once more through the multi-launch decodes (ValidationEpoch.run)
            scores, gave_up = self.scores(self.accumulate(batches, resident=False))
        if gave_up > 0:
            raise _lib.CareHipError(Translator_ARFormer._ABORTED)
        if scores["n_invalid"] > 0:
            raise ValueError("{} clips have no references: their `video_ids` lie outside the bank or name a video without "
                             "captions".format(int(scores["n_invalid"])))
        scores.update(added)
        analysis = self.captions.totals()
        scores.update({k: analysis[k] for k in ("ave_length", "novel", "unique", "usage")})
        host = self._fetch_records()
        names = self._video_names(host["video"].tolist())
        per_row = sentence_scores(host["stats"], host["rouge"], host["cider"])
        lengths, model_scores = host["length"].tolist(), host["score"].tolist()
        tokens = host["tokens"][:, :max(lengths, default=0)].tolist()
        detail_scores, pred_captions = {}, {}
        for name, d, toks, n, s in zip(names, per_row, tokens, lengths, model_scores):
            ids = toks[:n]
            caption = ids if vocab is None else " ".join(vocab[t] for t in ids)
            detail_scores[name] = d
            pred_captions.setdefault(name, []).append({"image_id": name, "caption": caption, "score": s})
        self.last, self.last_detail, self.last_predictions = scores, detail_scores, pred_captions
        return scores, detail_scores, pred_captions

    # ------------------------------------------------------------------ the two files translate.py writes
    def write_predictions(self, path: str) -> None:
        """--json_path / --json_name: the last run's `pred_captions` (Wrapper.py:136-140)."""
        with open(path, "w") as fh:
            json.dump(self.last_predictions, fh)

    def write_detail_scores(self, path: str) -> None:
        """--save_detailed_scores_path: the last run's `detail_scores`."""
        with open(path, "w") as fh:
            json.dump(self.last_detail, fh)

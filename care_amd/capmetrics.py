"""The validation metrics on the MI355X (csrc/capmetrics.hip): corpus BLEU-1..4, ROUGE-L and CIDEr over token ids.

    from care_amd.capmetrics import MetricBank
    bank = MetricBank(refs, vocab_size)                 # the references of the split being evaluated
    totals = bank.new_totals()
    for tokens, length, video in decoded_batches:       # device tensors, e.g. fed[:, 1:], length of translate_greedy
        bank.accumulate(bank.score(tokens, length, video), totals)
    scores = bank.scores(totals)                        # the ONE host read: Bleu_1..4, ROUGE_L, CIDEr, Sum

What the reference's validation epoch reports (models/Wrapper.py:214-273 through misc/cocoeval.py) except METEOR, with
coco-caption's definitions (restated in float64 in tests/capmetrics_reference.py): BLEU from the clipped n-gram counts and the
closest reference length, summed over the corpus; ROUGE-L with beta = 1.2 from the longest common subsequence, averaged; CIDEr -
the arithmetic of care_cider_score (csrc/reward.hip: clipping by `min`, a Gaussian length penalty with sigma = 6, times 10, df
over the evaluated set) - averaged.  `bank.score` is two launches, a workgroup per caption each; `bank.accumulate` adds a batch
into 14 words that stay on the device; nothing is read on the host before `bank.scores`.

Exact and not: the twelve integer totals (captions, lengths, guesses, clipped matches) are exact for any split of the epoch into
batches, so the four BLEU values do not depend on the batching at all; a caption's ROUGE-L is a handful of double operations and
its CIDEr is rounded once to fp32; their two SUMS are doubles added in a fixed order per batch and depend on the split in their
last bits.

Ids and words: the reference's corpus stores every out-of-vocabulary word as `<unk>`, but its scorers see the words
themselves.  `MetricBank.from_words` gives every word outside the model's vocabulary an id of its own above it, so matching ids
is matching pre-tokenised words and the numbers are coco-caption's.  A bank built from token ids instead scores ids: there
`<unk>` matches `<unk>`, which can only raise the scores of captions and references that both hold unknown words.

A bank must hold exactly the split being evaluated: `df` and `ln N` of CIDEr are that split's, as in coco-caption.  METEOR (Java,
on words) and the PTB tokenizer stay external.  As everywhere in care_amd there is no CPU fallback: CPU tensors raise.
"""
import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .constants import EOS
from .captions import caption_rows, need_device, number_words, strip_eos, upload
from .reward import ORDERS, CiderBank, pack_ngrams

__all__ = ["MetricBank", "corpus_scores", "check_metric_sum", "METRIC_SUM", "REC", "TOTALS"]

REC = 12          # ints of a caption's record: valid, testlen, reflen, guess 1..4, correct 1..4, 0
TOTALS = 14       # words of the running totals: 12 int64 (n_valid, n_invalid, testlen, reflen, guess, correct), 2 doubles
METRIC_SUM = (1, 0, 1, 1)   # the reference's --metric_sum: Bleu_4, METEOR, ROUGE_L, CIDEr
TINY, SMALL = 1e-15, 1e-9   # coco-caption's bleu_scorer.py


def check_metric_sum(metric_sum) -> tuple:
    """The four flags (Bleu_4, METEOR, ROUGE_L, CIDEr) of the reference's --metric_sum; a set METEOR flag is refused by name."""
    flags = tuple(metric_sum)
    if len(flags) != 4:
        raise ValueError("`metric_sum` holds 4 flags (Bleu_4, METEOR, ROUGE_L, CIDEr), got {!r}".format(metric_sum))
    if flags[1]:
        raise NotImplementedError("`metric_sum` asks for METEOR: METEOR is a Java tool that works on words and is not computed here")
    return flags


def corpus_scores(ints: Sequence[int], rouge_sum: float, cider_sum: float, metric_sum=METRIC_SUM) -> Dict[str, float]:
    """The corpus scores of the totals (n_valid, n_invalid, testlen, reflen, guess 1..4, correct 1..4) and the two sums, in
    float64: coco-caption's corpus BLEU with its brevity penalty, the means of ROUGE-L and CIDEr, and the reference's `Sum`."""
    flags = check_metric_sum(metric_sum)
    ints = [int(x) for x in ints]
    n_valid, n_invalid, testlen, reflen = ints[:4]
    guess, correct = ints[4:8], ints[8:12]
    out, bleu, bleus = {}, 1.0, []
    for k in range(ORDERS):
        bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        bleus.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        bleus = [b * math.exp(1 - 1 / ratio) for b in bleus]
    for k in range(ORDERS):
        out["Bleu_%d" % (k + 1)] = bleus[k]
    out["ROUGE_L"] = float(rouge_sum) / n_valid if n_valid else 0.0
    out["CIDEr"] = float(cider_sum) / n_valid if n_valid else 0.0
    out["Sum"] = sum(out[k] for k, f in zip(("Bleu_4", "METEOR", "ROUGE_L", "CIDEr"), flags) if f)
    out["n_captions"], out["n_invalid"] = float(n_valid), float(n_invalid)
    return out


class MetricBank(object):
    """The reference captions of the evaluated split, on the device.  The arguments and refusals of care_amd.CiderBank, which it
    composes over the same references (`bank.cider`); on top of it the per-video clip table of BLEU - the sorted unique n-gram
    keys of a video's references with each one's largest count in one reference - and the references' tokens for ROUGE-L."""

    def __init__(self, refs: Sequence[Sequence[Sequence[int]]], vocab_size: int, with_eos: bool = False, device="cuda",
                 video_ids: Optional[Sequence] = None):
        refs = [[list(r) for r in video] for video in refs]
        self.cider = CiderBank(refs, vocab_size, with_eos=with_eos, device=device, video_ids=video_ids)
        c = self.cider
        self.vocab_size, self.with_eos, self.n_videos, self.n_refs, self.device = c.vocab_size, c.with_eos, c.n_videos, c.n_refs, c.device
        self.extra_words = {}
        clip_keys, clip_max, clip_start, ref_tok, ref_tok_start = [], [], [0], [], [0]
        for video in refs:
            keys, counts = [], []
            for ref in video:
                toks = strip_eos(ref, self.with_eos)
                ref_tok.append(toks.astype(np.int32))
                ref_tok_start.append(ref_tok_start[-1] + toks.size)
                u, n = np.unique(np.concatenate([pack_ngrams(toks, k) for k in range(1, ORDERS + 1)]), return_counts=True)
                keys.append(u)
                counts.append(n)
            if keys:
                u, inv = np.unique(np.concatenate(keys), return_inverse=True)
                most = np.zeros(u.size, dtype=np.int64)
                np.maximum.at(most, inv.reshape(-1), np.concatenate(counts))
                clip_keys.append(u)
                clip_max.append(most.astype(np.int32))
            clip_start.append(clip_start[-1] + (clip_keys[-1].size if keys else 0))
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)   # noqa: E731
        self.host = {"clip_keys": cat(clip_keys, np.uint64), "clip_max": cat(clip_max, np.int32),
                     "clip_start": np.asarray(clip_start, dtype=np.int64), "ref_tok": cat(ref_tok, np.int32),
                     "ref_tok_start": np.asarray(ref_tok_start, dtype=np.int64)}
        self.dev = self.desc = None
        if self.device is None:
            return

        self.dev = {k: upload(a, self.device) for k, a in self.host.items()}
        self.desc = _lib.MetricBankDesc()
        ctypes.memmove(ctypes.addressof(self.desc), ctypes.addressof(c.desc), ctypes.sizeof(_lib.CiderBankDesc))
        for k, t in self.dev.items():
            setattr(self.desc, k, t.data_ptr())

    @classmethod
    def from_words(cls, refs_words: Sequence[Sequence[Sequence[str]]], word_to_id: dict, vocab_size: Optional[int] = None,
                   with_eos: bool = False, device="cuda", video_ids: Optional[Sequence] = None) -> "MetricBank":
        """A bank from references given as lists of WORDS: a word of the model's vocabulary (`word_to_id`) gets its id, every
        other word a fresh id from `vocab_size` (default: the largest id of `word_to_id` + 1) upwards - `bank.extra_words`.
        More than 65536 ids in all is a ValueError (an n-gram's key holds 16 bits a token)."""
        videos = [list(video) for video in refs_words]
        ids, extra, total = number_words([ref for video in videos for ref in video], word_to_id, vocab_size)
        ids = iter(ids)
        refs = [[next(ids) for _ in video] for video in videos]   # (video by video again)
        bank = cls(refs, total, with_eos=with_eos, device=device, video_ids=video_ids)
        bank.extra_words = extra
        return bank

    def rows(self, video_ids) -> torch.Tensor:
        """CiderBank.rows: the bank rows (int32, on the bank's device) of a batch's `video_ids`."""
        return self.cider.rows(video_ids)

    def _need_bank(self) -> None:
        if self.desc is None:
            raise RuntimeError("this bank was built with device=None (host tables only): the metrics are scored on the MI355X")

    def score(self, tokens: torch.Tensor, length: torch.Tensor, video: torch.Tensor, with_cider: bool = True, offset: int = 0) -> dict:
        """{"stats": int32 [rows, 12], "rouge": float64 [rows], "cider": fp32 [rows] or None} of caption r =
        tokens[r, offset : offset + length[r]] against the references of bank row video[r] - device tensors, nothing is waited
        for.  tokens: int32 [rows, width <= 64 behind the offset] with unit stride in the last dimension and any row stride: a
        view such as fed[:, 1:] is scored in place (the rules of CiderBank.score)."""
        self._need_bank()
        rows, width, ld, length = caption_rows(tokens, length, offset, "care_caption_stats", also=(("video", video),))
        video = video.contiguous()
        stats = torch.empty(rows, REC, dtype=torch.int32, device=tokens.device)
        rouge = torch.empty(rows, dtype=torch.float64, device=tokens.device)
        with torch.cuda.device(tokens.device):
            _lib.call("care_caption_stats", _lib.ptr(tokens), ld, int(offset), width, _lib.ptr(length), _lib.ptr(video), rows,
                      int(self.with_eos), EOS, ctypes.addressof(self.desc), _lib.ptr(stats), _lib.ptr(rouge), tag="caption_stats")
        cider = self.cider.score(tokens, length, video, offset=offset) if with_cider else None
        return {"stats": stats, "rouge": rouge, "cider": cider}

    def new_totals(self) -> torch.Tensor:
        """The running totals of an epoch, zeroed: int64 [14] on the bank's device - (n_valid, n_invalid, testlen, reflen,
        guess 1..4, correct 1..4) and, as the bits of two doubles, (sum of ROUGE-L, sum of CIDEr)."""
        return torch.zeros(TOTALS, dtype=torch.int64, device=self.device if self.device is not None else "cpu")

    def accumulate(self, rec: dict, totals: torch.Tensor) -> torch.Tensor:
        """Adds a batch (what `score` returned) into `totals`, on the device: the integers exactly, whatever the split into
        batches; the two sums of doubles in a fixed order per batch, so they depend on the split in their last bits."""
        self._need_bank()
        stats, rouge, cider = rec["stats"], rec["rouge"], rec.get("cider")
        need_device(totals, "totals", "care_caption_totals")
        if totals.dtype != torch.int64 or totals.numel() != TOTALS or not totals.is_contiguous():
            raise ValueError("`totals` must be what new_totals() returned: a contiguous int64 tensor of {} words".format(TOTALS))
        rows = stats.shape[0]
        if stats.dtype != torch.int32 or tuple(stats.shape) != (rows, REC) or not stats.is_contiguous() or rouge.dtype != torch.float64 \
                or rouge.numel() != rows or (cider is not None and (cider.dtype != torch.float32 or cider.numel() != rows)):
            raise ValueError("`rec` must be what score() returned: stats int32 [rows, {}], rouge float64 [rows], cider fp32 [rows]".format(REC))
        with torch.cuda.device(totals.device):
            _lib.call("care_caption_totals", _lib.ptr(stats), _lib.ptr(rouge.contiguous()), _lib.ptr(None if cider is None else cider.contiguous()),
                      rows, _lib.ptr(totals), totals.data_ptr() + 8 * REC, tag="caption_totals")
        return totals

    def scores(self, totals: torch.Tensor, metric_sum=METRIC_SUM) -> Dict[str, float]:
        """The epoch's scores as Python floats - Bleu_1..4, ROUGE_L, CIDEr, Sum (the flags of the reference's --metric_sum, in its
        order: Bleu_4, METEOR, ROUGE_L, CIDEr; a set METEOR flag is refused), n_captions, n_invalid.  The ONE host read."""
        check_metric_sum(metric_sum)   # (refused by name before anything is read)
        host = totals.detach().cpu().contiguous()
        return corpus_scores(host[:REC].tolist(), *host[REC:].view(torch.float64).tolist(), metric_sum=metric_sum)

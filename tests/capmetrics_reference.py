"""coco-caption's BLEU, ROUGE-L and CIDEr over integer token ids, in float64 and plain Python: the yardstick of
care_caption_stats / care_caption_totals (csrc/capmetrics.hip), of care_amd.capmetrics.MetricBank and of the validation epoch.
No packing and no numpy in the arithmetic; pycocoevalcap's definitions restated, as tests/cider_reference.py restates CIDEr-D.

A caption is `tokens[:length]` with one trailing EOS dropped unless with_eos (cider_reference.caption); L its length.

BLEU (bleu_scorer.py), per caption the components
    guess_n   = max(0, L - n + 1)
    correct_n = sum over the caption's distinct n-grams g of min(count_h(g), max over the references of count_r(g))
    reflen    = the reference length closest to L, the smaller one of two equally close: min((abs(l - L), l))
and over any set of captions, with the components summed, tiny = 1e-15 and small = 1e-9:
    Bleu_n = (prod_{k <= n} (correct_k + tiny) / (guess_k + small)) ** (1 / n),
             times exp(1 - 1 / ratio) when ratio = (testlen + tiny) / (reflen + small) < 1.
ROUGE-L (rouge.py, beta = 1.2): with lcs the longest common subsequence by the textbook DP,
    P = max_r lcs(r, h) / L,  R = max_r lcs(r, h) / len(r)   (the maxima independent of each other),
    score = (1 + beta^2) P R / (R + beta^2 P) when both are non-zero, else 0;
an empty caption scores 0 and a reference without tokens adds to neither maximum (the original would divide by zero).
CIDEr: cider_reference.Corpus.score."""
import math
from collections import Counter

import cider_reference as C

EOS = C.EOS
ORDERS = 4
BETA = 1.2
TINY, SMALL = 1e-15, 1e-9
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")


def lcs(a, b):
    """The length of the longest common subsequence of two sequences: the plain (len(a) + 1) x (len(b) + 1) table."""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def closest(ref_lens, L):
    return min((abs(l - L), l) for l in ref_lens)[1]


def bleu_components(hyp, refs):
    """(testlen, reflen, [guess_1..4], [correct_1..4]) of one caption against its references (token lists)."""
    guess, correct = [], []
    for n in range(1, ORDERS + 1):
        counts = C.ngrams(hyp, n)
        most = Counter()
        for ref in refs:
            for g, c in C.ngrams(ref, n).items():
                most[g] = max(most[g], c)
        guess.append(max(0, len(hyp) - n + 1))
        correct.append(sum(min(c, most[g]) for g, c in counts.items() if g in most))
    return len(hyp), closest([len(r) for r in refs], len(hyp)), guess, correct


def bleu(testlen, reflen, guess, correct):
    """[Bleu_1..4] of summed components (one caption's or a corpus')."""
    out, b = [], 1.0
    for k in range(ORDERS):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


def rouge_l(hyp, refs):
    if not hyp:
        return 0.0
    prec, rec = [], []
    for ref in refs:
        n = lcs(ref, hyp) if ref else 0
        prec.append(n / float(len(hyp)))
        rec.append(n / float(len(ref)) if ref else 0.0)
    p, r = max(prec), max(rec)
    if p != 0 and r != 0:
        return ((1 + BETA ** 2) * p * r) / float(r + BETA ** 2 * p)
    return 0.0


class Corpus(object):
    """The references of a split (one list of token lists per video).  `record` is what care_caption_stats writes for a
    row, `corpus` what MetricBank.scores returns for a set of rows."""

    def __init__(self, refs, with_eos=False, eos=EOS):
        self.with_eos, self.eos = with_eos, eos
        self.refs = [[C.caption(r, None, with_eos, eos) for r in video] for video in refs]
        self.cider = C.Corpus(refs, with_eos=with_eos, eos=eos)

    def valid(self, length, video):
        return length > 0 and 0 <= video < len(self.refs) and len(self.refs[video]) > 0

    def record(self, tokens, length, video):
        """([valid, testlen, reflen, guess_1..4, correct_1..4, 0], rouge, cider) of one row; an invalid row is all zeros."""
        if not self.valid(length, video):
            return [0] * 12, 0.0, 0.0
        hyp = C.caption(tokens, length, self.with_eos, self.eos)
        testlen, reflen, guess, correct = bleu_components(hyp, self.refs[video])
        return [1, testlen, reflen] + guess + correct + [0], rouge_l(hyp, self.refs[video]), self.cider.score(tokens, length, video)

    def records(self, tokens, lengths, videos):
        return [self.record(list(t), int(l), int(v)) for t, l, v in zip(tokens, lengths, videos)]

    @staticmethod
    def totals(records):
        """([n_valid, n_invalid, testlen, reflen, guess_1..4, correct_1..4], sum rouge, sum cider) of records, added in order."""
        ints, rouge, cider = [0] * 12, 0.0, 0.0
        for rec, r, c in records:
            if rec[0]:
                ints[0] += 1
                for k in range(10):
                    ints[2 + k] += rec[1 + k]
                rouge += r
                cider += c
            else:
                ints[1] += 1
        return ints, rouge, cider

    def corpus(self, records, metric_sum=(1, 0, 1, 1)):
        ints, rouge, cider = self.totals(records)
        b = bleu(ints[2], ints[3], ints[4:8], ints[8:12])
        out = {"Bleu_%d" % (k + 1): b[k] for k in range(ORDERS)}
        out["ROUGE_L"] = rouge / ints[0] if ints[0] else 0.0
        out["CIDEr"] = cider / ints[0] if ints[0] else 0.0
        out["Sum"] = sum(out[k] for k, f in zip(("Bleu_4", "METEOR", "ROUGE_L", "CIDEr"), metric_sum) if f)
        out["n_captions"], out["n_invalid"] = float(ints[0]), float(ints[1])
        return out

"""The coco-caption CIDEr-D over integer token ids, in float64 and plain Python: the yardstick of care_cider_score
(csrc/reward.hip) and of care_amd.reward.CiderBank.

An n-gram is a TUPLE of token ids here (no packing), a caption a list of ints.  With `tf` the count of an n-gram in a caption,
`df` the number of videos whose reference set holds it (once per video) and N the number of videos:

    w(g)    = tf(g) * (ln N - ln max(1, df(g)))
    norm_n  = sqrt(sum of w^2 over the caption's n-grams of order n)
    sim_n   = sum over g in the candidate of min(w_h(g), w_r(g)) * w_r(g),
              divided by norm_n(h) * norm_n(r) when both are non-zero,
              times exp(-(len_h - len_r)^2 / (2 * 6^2))
    score   = 10 * mean over n = 1..4 of (mean over the video's references of sim_n)

A caption is `tokens[:length]` with one trailing EOS dropped; with `with_eos` the EOS stays an ordinary token, in candidates and
references alike."""
import math
from collections import Counter

EOS = 3
SIGMA = 6.0
ORDERS = 4


def caption(tokens, length=None, with_eos=False, eos=EOS):
    toks = [int(t) for t in (tokens if length is None else tokens[:max(0, int(length))])]
    if toks and not with_eos and toks[-1] == eos:
        toks = toks[:-1]
    return toks


def ngrams(toks, n):
    return Counter(tuple(toks[i:i + n]) for i in range(len(toks) - n + 1))


def document_frequency(refs, with_eos=False, eos=EOS):
    """df[g]: the number of videos whose references hold the n-gram g (any order), each video counted once."""
    df = Counter()
    for video in refs:
        seen = set()
        for ref in video:
            toks = caption(ref, None, with_eos, eos)
            for n in range(1, ORDERS + 1):
                seen.update(ngrams(toks, n))
        df.update(seen)
    return df


def weights(toks, n, df, ln_n):
    return {g: tf * (ln_n - math.log(max(1, df.get(g, 0)))) for g, tf in ngrams(toks, n).items()}


def norm(w):
    return math.sqrt(sum(x * x for x in w.values()))


class Corpus(object):
    def __init__(self, refs, with_eos=False, eos=EOS):
        self.with_eos, self.eos = with_eos, eos
        self.refs = [[caption(r, None, with_eos, eos) for r in video] for video in refs]
        self.df = document_frequency(refs, with_eos, eos)
        self.ln_n = math.log(len(refs))
        self._ref = {}   # (video, reference, n) -> (weights, norm): computed once, left unchanged

    def _ref_weights(self, video, i, n):
        if (video, i, n) not in self._ref:
            wr = weights(self.refs[video][i], n, self.df, self.ln_n)
            self._ref[video, i, n] = (wr, norm(wr))
        return self._ref[video, i, n]

    def score(self, tokens, length, video):
        """CIDEr-D of one candidate against the references of `video` (a row of the corpus); 0 outside the corpus."""
        hyp = caption(tokens, length, self.with_eos, self.eos)
        if not (0 <= video < len(self.refs)) or not hyp or not self.refs[video]:
            return 0.0
        total = 0.0
        for n in range(1, ORDERS + 1):
            wh = weights(hyp, n, self.df, self.ln_n)
            nh = norm(wh)
            over_refs = 0.0
            for i, ref in enumerate(self.refs[video]):
                wr, nr = self._ref_weights(video, i, n)
                sim = sum(min(w, wr[g]) * wr[g] for g, w in wh.items() if g in wr)
                if nh != 0.0 and nr != 0.0:
                    sim /= nh * nr
                delta = float(len(hyp) - len(ref))
                over_refs += sim * math.exp(-(delta * delta) / (2.0 * SIGMA * SIGMA))
            total += over_refs / len(self.refs[video])
        return 10.0 * total / ORDERS

    def scores(self, tokens, lengths, videos):
        return [self.score(list(t), l, v) for t, l, v in zip(tokens, lengths, videos)]

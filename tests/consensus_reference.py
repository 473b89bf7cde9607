"""Consensus among a clip's own candidate captions, in float64 and plain Python: the yardstick of care_consensus_score
(csrc/consensus.hip) and of care_amd.consensus_select.  The pieces are those of tests/cider_reference.py.

A clip has n candidate rows of which the first m are valid.  With a candidate's weights w(g) = tf(g) (ln N - ln max(1, df(g)))
from the CORPUS the bank was built over (df = 0 for an n-gram the corpus does not hold) and its norms per order, for j != i,
both < m:

    t_o(j, i)   = sim_o(j -> i) * exp(-(len_j - len_i)^2 / 72)
    sim_o(j->i) = sum over g in j of min(w_j(g), w_i(g)) * w_i(g),  divided by norm_o(j) * norm_o(i) when both are non-zero
    pair[j][i]  = 10 * (t_1 + t_2 + t_3 + t_4) / 4
    score[j]    = 10 * (sum over o of (sum over i != j, i < m, in ascending i, of t_o(j, i)) / (m - 1)) / 4

- the CIDEr-D of candidate j with the clip's other valid candidates as its reference set.  pair[j][j] = 0, entries with j >= m
or i >= m are 0, m <= 1 gives scores 0.  winner = the j < m with the largest score, the lower j among equals; -1 when m == 0.
(Here the doubles are compared; the kernel compares the fp32 values it writes - copies of one caption may differ in the last
bit of a double, see include/care_hip.h - so the tests hold the kernel's winner to this one only where the gap exceeds 1e-6, and
everywhere to a score within 1e-9 of the best.)"""
import math

from cider_reference import ORDERS, SIGMA, Corpus, caption, norm, weights


def clip(corpus: Corpus, candidates, lengths=None, m=None):
    """(score [n], pair [n][n], winner) of one clip: candidates = n token lists (cut to lengths[j] when given, the trailing
    EOS by the corpus' rule), of which the first m (default all) are valid."""
    n = len(candidates)
    m = n if m is None else max(0, min(int(m), n))
    caps = [caption(c, None if lengths is None else lengths[j], corpus.with_eos, corpus.eos) for j, c in enumerate(candidates)]
    table = []
    for toks in caps[:m]:
        per_order = [weights(toks, o, corpus.df, corpus.ln_n) for o in range(1, ORDERS + 1)]
        table.append([(w, norm(w)) for w in per_order])
    score, pair = [0.0] * n, [[0.0] * n for _ in range(n)]
    for j in range(m):
        acc = [0.0] * ORDERS
        for i in range(m):
            if i == j:
                continue
            delta = float(len(caps[j]) - len(caps[i]))
            pen = math.exp(-(delta * delta) / (2.0 * SIGMA * SIGMA))
            terms = []
            for o in range(ORDERS):
                (wj, nj), (wi, ni) = table[j][o], table[i][o]
                sim = sum(min(w, wi[g]) * wi[g] for g, w in wj.items() if g in wi)
                if nj != 0.0 and ni != 0.0:
                    sim /= nj * ni
                terms.append(sim * pen)
                acc[o] += terms[o]
            pair[j][i] = 10.0 * (sum(terms) / ORDERS)
        if m > 1:
            score[j] = 10.0 * (sum(a / (m - 1) for a in acc) / ORDERS)
    winner = -1
    for j in range(m):
        if winner < 0 or score[j] > score[winner]:
            winner = j
    return score, pair, winner


def clips(corpus: Corpus, tokens, lengths, n, counts=None):
    """`clip` over rows b n + j of `tokens` / `lengths`: lists (score [B][n], pair [B][n][n], winner [B])."""
    B = len(tokens) // n
    out = [clip(corpus, [list(t) for t in tokens[b * n: b * n + n]], list(lengths[b * n: b * n + n]),
                None if counts is None else counts[b]) for b in range(B)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]

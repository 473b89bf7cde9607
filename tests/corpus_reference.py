"""The caption analysis of the reference's test run over integer token ids, in plain Python (dicts and sets, no hashing tricks):
the yardstick of care_corpus_insert / care_corpus_totals (csrc/corpus_stats.hip), of care_amd.corpusstats and of the test
epoch; and coco-caption's per-sentence BLEU on top of tests/capmetrics_reference.py.

misc/utils.py restated (cal_n_gram :390-403, cal_gt_n_gram :375-387, analyze_length_novel_unique :406-419, n = 1):
    a prediction is a token row cut at the first EOS or PAD (to_sentence :117-137) and joined with blanks; `.split(' ')` of it
    gives the words back - except that the EMPTY caption gives [''], ONE (empty) word;
    ave_length = sum of len(words) / captions;  unique = distinct captions / captions;
    novel = distinct captions that are no training caption / captions - a training caption is the ids tmp[1:-1], whole;
    usage = distinct words over all captions.
Over ids a word is its id and the empty word is None."""
import capmetrics_reference as M

EOS, PAD = M.EOS, 0
KEYS = ("ave_length", "novel", "unique", "usage")


def cut(tokens, length=None, eos=EOS, pad=PAD):
    out = []
    for t in list(tokens)[:None if length is None else max(int(length), 0)]:
        if t == eos or t == pad:
            break
        out.append(int(t))
    return tuple(out)


def totals(train_captions, captions):
    """The integers (dict) of captions already cut (tuples of ids) against the training captions (sequences of ids)."""
    train = {}
    for c in train_captions:
        train[tuple(int(t) for t in c)] = train.get(tuple(int(t) for t in c), 0) + 1
    sents, words, length_sum, count, empty = {}, {}, 0, 0, 0
    for cap in captions:
        cap = tuple(cap)
        sents[cap] = sents.get(cap, 0) + 1
        split = list(cap) if cap else [None]   # ''.split(' ') == ['']
        length_sum += len(split)
        count += 1
        empty += 0 if cap else 1
        for w in split:
            words[w] = words.get(w, 0) + 1
    novel = sum(1 for c in sents if c not in train)
    return {"n_captions": count, "length_sum": length_sum, "n_distinct": len(sents), "n_novel": novel, "n_empty": empty,
            "usage": len(words)}


def analyze(train_captions, rows, lengths=None):
    """(ave_length, novel, unique, usage) of predicted token rows (cut here) - analyze_length_novel_unique's tuple."""
    caps = [cut(r, None if lengths is None else lengths[i]) for i, r in enumerate(rows)]
    t = totals(train_captions, caps)
    n = t["n_captions"]
    return t["length_sum"] / n, t["n_novel"] / n, t["n_distinct"] / n, t["usage"]


def sentence_bleu(rec):
    """[Bleu_1..4] of ONE caption's record (valid, testlen, reflen, guess 1..4, correct 1..4, 0): bleu_scorer.py's per-sentence
    list - the corpus formula on the caption's own components."""
    return M.bleu(rec[1], rec[2], rec[3:7], rec[7:11])


def detail(rec, rouge, cider):
    b = sentence_bleu(rec)
    out = {"Bleu_%d" % (k + 1): b[k] for k in range(4)}
    out["ROUGE_L"], out["CIDEr"] = rouge, cider
    return out

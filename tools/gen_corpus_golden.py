"""Record tests/golden/corpus/*.json: the genuine reference's caption analysis on small cases (CPU).

    python tools/gen_corpus_golden.py

Imports misc/utils.py's own `to_sentence` (:117-137), `cal_gt_n_gram` (:375-387) and `analyze_length_novel_unique` (:406-419, the
live definition) through oracle.ref_import's path handling, builds the structures they take - a corpus {"video%d": [[BOS, ids..,
EOS], ..]} with every video in splits["train"], predictions {video: [{"caption": to_sentence(row, vocab)}]} - and records what
they return.  Stores DATA only, one file per case: {"name", "vocab" (the word of every id), "train" (the ids tmp[1:-1] of every
training caption), "rows" (predicted token rows, EOS / PAD included), "captions" (to_sentence's strings), "n_train_distinct"
(len of cal_gt_n_gram's gt_sents), "expected": [ave_length, novel, unique, usage]}.  tests/test_corpus_stats_cpu.py holds
tests/corpus_reference.py to these files, tests/test_gpu_corpus_kernels.py the kernels.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "corpus")
PAD, UNK, BOS, EOS, MASK, VIS = range(6)
SPECIAL = ["<pad>", "<unk>", "<bos>", "<eos>", "<mask>", "<vis>"]


def pad_rows(caps, width=None, tail=()):
    """Token rows of one width: a caption, EOS, PAD behind it."""
    width = width or max(len(c) for c in caps) + 1
    return [list(c) + [EOS] * (len(c) < width) + [PAD] * (width - len(c) - 1) for c in caps]


def cases():
    a, man, b = 6, 7, 8
    words = SPECIAL + ["a", "man", "b", "c", "d", "e", "f", "g"]
    yield "toy", words, [[a, man], [], [a]], pad_rows([[a, man], [], [a, man], [b, b]])
    yield "all_distinct_novel", words, [[a, man], [b], [a, man, b, 9]], pad_rows([[a], [man], [a, b], [b, a], [a, man, b], [9, 10, 11, 12, 13]])
    yield "all_identical", words, [[a, man, b], [a]], pad_rows([[a, man, b]] * 9)
    yield ("prefixes", words, [[a, man], [a, man, b, 9], [a, man, b, 10, 11], [man]],
           pad_rows([[a], [a, man], [a, man, b], [a, man, b, 9], [a, man, b, 10], [a, man, b, 9, 10], [a, man, b, 10, 11], [a, man, 9],
                     [a, man, b], [man, a], [a, man]]))
    # an EOS in the middle (what stands behind it is not part of the caption), PAD before EOS, PAD or EOS in front
    yield ("eos_pad", words, [[a, man], [a], [b, 9]],
           [[a, man, EOS, b, 9, EOS], [a, PAD, man, EOS, PAD, PAD], [PAD, a, man, EOS, PAD, PAD], [EOS, a, man, b, 9, 10],
            [b, 9, EOS, EOS, EOS, EOS], [b, 9, 10, 11, 12, 13], [b, 9, PAD, PAD, PAD, EOS], [a, man, b, EOS, 9, PAD]])
    # ~200 seeded random captions over a 40-word vocabulary against ~500 training captions
    rng = np.random.RandomState(2024)
    words40 = SPECIAL + ["w%d" % i for i in range(40)]
    train = [rng.randint(6, 46, size=int(rng.randint(1, 6))).tolist() for _ in range(500)]
    train[17] = []
    caps = []
    for i in range(200):
        kind = i % 4
        if kind == 0:                       # a training caption: not novel
            caps.append(list(train[int(rng.randint(len(train)))]))
        elif kind == 1 and caps:            # an earlier prediction again: a duplicate
            caps.append(list(caps[int(rng.randint(len(caps)))]))
        else:                               # long enough to be novel almost surely
            caps.append(rng.randint(6, 46, size=int(rng.randint(4, 12))).tolist())
    caps[5], caps[150] = [], []
    yield "random200", words40, train, pad_rows(caps, width=14)


def main():
    from oracle import ref_import

    if not ref_import.reference_available():
        raise RuntimeError("reference tree not found at {}".format(ref_import.REFERENCE_ROOT))
    ref_import._stub_modules()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from misc.utils import analyze_length_novel_unique, cal_gt_n_gram, to_sentence

    os.makedirs(OUT, exist_ok=True)
    for name, words, train, rows in cases():
        vocab = {i: w for i, w in enumerate(words)}
        gt_data = {"video%d" % i: [[BOS] + list(c) + [EOS]] for i, c in enumerate(train)}
        splits = {"train": list(range(len(train)))}
        captions = [to_sentence(r, vocab) for r in rows]
        preds = {"video%d" % (10000 + i): [{"image_id": "video%d" % (10000 + i), "caption": c}] for i, c in enumerate(captions)}
        ave_length, novel, unique, usage = analyze_length_novel_unique(gt_data, preds, vocab, splits, n=1)
        _, gt_sents = cal_gt_n_gram(gt_data, vocab, splits, 1)
        if name == "toy":
            assert (ave_length, novel, unique, usage) == (1.75, 0.25, 0.75, 4), (ave_length, novel, unique, usage)
        if name == "random200":   # duplicates, novel captions and captions of the training set all occur
            distinct = set(captions)
            assert len(distinct) < len(captions) and any(c in gt_sents for c in distinct) and any(c not in gt_sents for c in distinct)
            assert 0 < novel < unique < 1
        case = {"name": name, "source": "misc/utils.py:406-419 analyze_length_novel_unique, :375-387 cal_gt_n_gram, :117-137 to_sentence",
                "vocab": words, "train": [list(map(int, c)) for c in train], "rows": [list(map(int, r)) for r in rows],
                "captions": captions, "n_train_distinct": len(gt_sents), "expected": [ave_length, novel, unique, int(usage)]}
        path = os.path.join(OUT, name + ".json")
        with open(path, "w") as fh:
            json.dump(case, fh)
            fh.write("\n")
        print("{}: {} rows, {} training captions -> {}".format(os.path.relpath(path, ROOT), len(rows), len(train), case["expected"]))


if __name__ == "__main__":
    main()

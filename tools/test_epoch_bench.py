"""The test epoch, timed (one JSON line):

    python tools/test_epoch_bench.py [--videos 2990] [--refs 20] [--train-videos 6513] [--batch 128] [--repeats 3]

tools/validation_bench.py's set-up - a synthetic MSRVTT-test-shaped split (2990 videos x 20 references, V = 10547), the
msrvtt_care model with synthetic weights, batch 128, greedy and beam 5 - plus a training corpus of 6513 x 20 = 130 260 captions
of the same law (another seed) for the caption analysis.  Wall clock around a synchronised epoch, the median of `repeats` after
one warm-up:

(a) `TestEpoch.run` against `ValidationEpoch.run` on the same loader: what the new parts add, per epoch and per batch;
(b) `TestEpoch.run` against the host route it replaces - `Translator.translate_batches`, then the Python scorer of the tests per
    caption (tests/capmetrics_reference.py: corpus scores and per-sentence records) and tests/corpus_reference.py's analysis
    over the 130 k training captions (dicts of tuples, rebuilt per call as cal_gt_n_gram rebuilds its dict of strings);
(c) `care_corpus_insert` alone (its two launches, HIP events around them, the set emptied before each) at 128 and 512 rows
    against the 130 k bank: rows of which half are training captions (found: the token-wise compare runs), a quarter repeat
    an earlier row (duplicates) and a quarter are new (the binary search ends without a hit).

(a) is also split: `accumulate` alone (the device pass up to a synchronisation, nothing read) for both epochs - the added
launches per batch - and the rest, the end of the epoch on the host (two more reads, 2990 per-sentence records, the dicts).

Every batch reuses one set of 128 clips' features (validation_bench.py), and a model with synthetic weights decodes captions no
training caption equals: in (a) and (b) the first batch's captions take empty slots and are looked up without a hit, every
later batch's end at an equal row after the token-wise compare; (c) covers the hits in the bank.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import capmetrics_reference
import corpus_reference
from care_amd import CorpusBank, EpochCaptions, MetricBank, TestEpoch, ValidationEpoch, get_framework, get_translator
from care_amd.configs import feat_shapes, make_opt
from care_amd.synth import synth_state_dict
from scst_bench import synthetic_corpus
from validation_bench import V, timed


def insert_alone(corpus, train, rows, repeats, dev):
    rng = np.random.RandomState(rows)
    caps = []
    for r in range(rows):
        kind = r % 4
        if kind < 2:
            caps.append(list(train[int(rng.randint(len(train)))]))
        elif kind == 2 and caps:
            caps.append(list(caps[int(rng.randint(len(caps)))]))
        else:
            caps.append(rng.randint(6, V, size=int(rng.randint(5, 15))).tolist())
    fed = np.zeros((rows, 31), dtype=np.int32)
    fed[:, 0] = 2
    for r, c in enumerate(caps):
        fed[r, 1: 1 + len(c)] = c
        fed[r, 1 + len(c)] = 3
    fed = torch.from_numpy(fed).to(dev)
    length = torch.tensor([len(c) + 1 for c in caps], dtype=torch.int32, device=dev)
    epoch = EpochCaptions(1024, V, corpus)
    times = []
    for i in range(repeats + 3):
        epoch.reset()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        epoch.insert(fed[:, 1:], length)
        end.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(start.elapsed_time(end) * 1e3)
    got = epoch.totals()
    want = corpus_reference.totals(train, [corpus_reference.cut(c) for c in caps])
    assert all(got[k] == want[k] for k in want), (got, want)
    return dict(rows=rows, median_us=round(statistics.median(times), 1), min_us=round(min(times), 1), max_us=round(max(times), 1), n=len(times),
                n_distinct=got["n_distinct"], n_novel=got["n_novel"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--refs", type=int, default=20)
    ap.add_argument("--train-videos", type=int, default=6513)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--insert-repeats", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("test_epoch_bench.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    refs = synthetic_corpus(a.videos, a.refs)
    train = [r[:-1] for video in synthetic_corpus(a.train_videos, a.refs, seed=1) for r in video]
    bank = MetricBank(refs, V, device=dev)
    t0 = time.perf_counter()
    corpus = CorpusBank(train, V, device=dev)
    build_s = time.perf_counter() - t0
    yard = capmetrics_reference.Corpus(refs)
    opt = dict(make_opt("msrvtt_care"), seed=0)
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, a.batch)]
    batches = [{"feats": [f[: min(a.batch, a.videos - lo)] for f in feats], "video_ids": list(range(lo, min(lo + a.batch, a.videos)))}
               for lo in range(0, a.videos, a.batch)]
    res = dict(tool="test_epoch_bench", videos=a.videos, refs_per_video=a.refs, batch=a.batch, batches=len(batches),
               train_captions=len(train), train_distinct=corpus.n, corpus_bank_build_s=round(build_s, 2))
    for beam in (1, 5):
        test = TestEpoch(opt, model, bank, corpus, capacity=a.videos, beam_size=beam)
        valid = ValidationEpoch(opt, model, bank, beam_size=beam)
        translator = get_translator(dict(opt, beam_size=beam))

        def host_route():
            rows, preds = [], {}
            for b, (hyps, scores) in zip(batches, translator.translate_batches([model], ({"feats": b["feats"]} for b in batches))):
                rows += [(h[0], len(h[0]), v) for h, v in zip(hyps, b["video_ids"])]
                for h, s, v in zip(hyps, scores, b["video_ids"]):
                    preds[v] = [{"image_id": v, "caption": list(corpus_reference.cut(h[0])), "score": s[0]}]
            records = yard.records(*zip(*rows))
            scores = yard.corpus(records)
            detail = {v: corpus_reference.detail(*rec) for (_, _, v), rec in zip(rows, records)}
            scores.update(zip(corpus_reference.KEYS, corpus_reference.analyze(train, [r[0] for r in rows])))
            return scores, detail, preds

        (got, _, _), t_test = timed(lambda: test.run(batches), a.repeats)
        _, t_valid = timed(lambda: valid.run(batches), a.repeats)
        (want, _, _), t_host = timed(host_route, a.host_repeats)
        _, t_test_pass = timed(lambda: test.accumulate(batches), a.repeats)
        _, t_valid_pass = timed(lambda: valid.accumulate(batches), a.repeats)
        added_pass = t_test_pass["median_s"] - t_valid_pass["median_s"]
        added = t_test["median_s"] - t_valid["median_s"]
        res["greedy" if beam == 1 else "beam%d" % beam] = dict(
            test_epoch=t_test, validation_epoch=t_valid, host_route=t_host, added_s=round(added, 4),
            test_pass=t_test_pass, validation_pass=t_valid_pass, added_pass_per_batch_us=round(added_pass / len(batches) * 1e6, 1),
            added_end_of_epoch_s=round(added - added_pass, 4),
            added_per_batch_us=round(added / len(batches) * 1e6, 1), validation_per_batch_us=round(t_valid["median_s"] / len(batches) * 1e6, 1),
            host_over_test_epoch=round(t_host["median_s"] / t_test["median_s"], 1),
            analysis={k: got[k] for k in corpus_reference.KEYS}, analysis_equals_host_route=all(got[k] == want[k] for k in corpus_reference.KEYS),
            max_deviation_from_host_route=max(abs(got[k] - want[k]) for k in capmetrics_reference.KEYS))
    res["insert_alone"] = [insert_alone(corpus, train, rows, a.insert_repeats, dev) for rows in (128, 512)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""GPU: the test epoch (care_amd/testepoch.py) on the smallest golden model of the epoch tests (tests/test_gpu_validation.py's
model, references and split: 7 videos in batches of 3, 3 and 1), greedy and beam 5, against plain Python on the captions
`translate_batch` itself returns for the same batches:
  scores        == ValidationEpoch.run's on every key both have (the same launches in the same order);
  the analysis  == tests/corpus_reference.py's over those captions, the training corpus being the references, an empty
                   caption and two of the predictions themselves (so that known and novel captions both occur);
  detail_scores :  the per-sentence BLEU == the float64 restatement on the reference's record (the integers are exact), ROUGE_L
                   within 1e-12 and CIDEr within 2e-6 - the bars of tests/test_gpu_capmetrics_kernels.py for the same quantities;
  pred_captions :  to_sentence's words of translate_batch's captions and its scores, bit for bit.
The two JSON files round-trip, a second run starts from zero, a pass reads nothing on the host and a run reads three times.

Measured on one MI355X (greedy / beam 5): the analysis (29.0, 5 / 7, 1.0, 185 / 181) equal to the reference's; the three tests: 3.5 s."""
import gc
import json

import pytest
import torch

import capmetrics_reference as M
import corpus_reference as R
from test_gpu_validation import CIDER_BAR, DEV, N_VIDEOS, _batches, _model, _refs

pytestmark = pytest.mark.gpu

ROUGE_BAR = 1e-12   # tests/test_gpu_capmetrics_kernels.py
NAMES = ["video%d" % (7010 + i) for i in range(N_VIDEOS)]


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _train(refs):
    return [[t for t in r if t != M.EOS] for video in refs for r in video] + [[]]


@pytest.mark.parametrize("beam_size", [1, 5], ids=["greedy", "beam5"])
def test_the_test_epoch_against_translate_batch_in_plain_python(beam_size, tmp_path, monkeypatch):
    from care_amd import CorpusBank, MetricBank, TestEpoch, ValidationEpoch, get_translator

    opt, feats, model = _model()
    opt = dict(opt, seed=11, tags=["x", 2])
    refs, V = _refs(), opt["vocab_size"]

    # the yardstick: translate_batch's captions and scores; two of the captions join the training corpus (known, not novel)
    model.eval()
    translator = get_translator(dict(opt, beam_size=beam_size))
    hyps, model_scores, videos = [], [], []
    for batch in _batches(feats):
        h, s = translator.translate_batch([model], {"feats": batch["feats"]})
        hyps += [x[0] for x in h]
        model_scores += [x[0] for x in s]
        videos += batch["video_ids"]
    model.train()
    train = _train(refs) + [list(R.cut(hyps[0])), list(R.cut(hyps[4]))]
    bank = MetricBank(refs, V, device=DEV, video_ids=NAMES)
    corpus = CorpusBank(train, V, device=DEV)
    vocab = {i: "w%d" % i for i in range(V)}
    epoch = TestEpoch(opt, model, bank, corpus, capacity=N_VIDEOS, beam_size=beam_size)

    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)) if self.is_cuda else None, cpu(self, *a, **k))[1])
    scores, detail, preds = epoch.run(_batches(feats, NAMES), vocab=vocab, keys_added_to_scores=("seed", "tags"))
    monkeypatch.undo()
    assert len(reads) == 3, reads   # the state, the analysis' totals, the per-caption arrays
    assert model.training and epoch.count == N_VIDEOS and epoch.last == scores

    # ValidationEpoch on the same loader: the same numbers on every shared key
    plain = ValidationEpoch(opt, model, bank, beam_size=beam_size).run(_batches(feats, NAMES))
    assert set(plain) <= set(scores) and all(scores[k] == plain[k] for k in plain), (scores, plain)
    assert scores["seed"] == 11 and scores["tags"] == "x-2"
    assert set(scores) - set(plain) == {"seed", "tags", "ave_length", "novel", "unique", "usage"}

    want = R.analyze(train, hyps)
    print(beam_size, "analysis", want, [R.cut(h) for h in hyps][:3])
    assert (scores["ave_length"], scores["novel"], scores["unique"], scores["usage"]) == want
    assert isinstance(scores["usage"], int) and 0 < scores["novel"] < scores["unique"] <= 1, "known and novel captions both occur"

    yard = M.Corpus(refs)
    assert list(detail) == NAMES and list(preds) == NAMES
    for name, h, s, v in zip(NAMES, hyps, model_scores, videos):
        rec, rouge, cider = yard.record(h, len(h), v)
        d = detail[name]
        assert set(d) == {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"}
        bleu = R.sentence_bleu(rec)
        assert [d["Bleu_%d" % (k + 1)] for k in range(4)] == bleu, (name, d, bleu)   # floats by ==: the record's integers are exact
        assert abs(d["ROUGE_L"] - rouge) <= ROUGE_BAR and abs(d["CIDEr"] - cider) <= CIDER_BAR, (name, d, rouge, cider)
        assert preds[name] == [{"image_id": name, "caption": " ".join(vocab[t] for t in R.cut(h)), "score": s}], (name, preds[name], h, s)

    # the two files translate.py writes
    p1, p2 = str(tmp_path / "preds.json"), str(tmp_path / "detail.json")
    epoch.write_predictions(p1)
    epoch.write_detail_scores(p2)
    assert json.load(open(p1)) == preds and json.load(open(p2)) == detail

    # a second run on the same object starts from zero; without a vocabulary the captions are ids
    scores2, detail2, preds2 = epoch.run(_batches(feats, NAMES), keys_added_to_scores=("seed", "tags"))
    assert scores2 == scores and detail2 == detail and epoch.count == N_VIDEOS
    assert [preds2[n][0]["caption"] for n in NAMES] == [list(R.cut(h)) for h in hyps]
    assert [preds2[n][0]["score"] for n in NAMES] == model_scores


def test_a_pass_reads_nothing_and_an_epoch_beyond_its_capacity_is_refused():
    from care_amd import CorpusBank, MetricBank, TestEpoch

    opt, feats, model = _model()
    opt = dict(opt, seed=11)
    refs, V = _refs(), opt["vocab_size"]
    bank = MetricBank(refs, V, device=DEV)
    corpus = CorpusBank(_train(refs), V, device=DEV)
    epoch = TestEpoch(opt, model, bank, corpus, capacity=N_VIDEOS, beam_size=1)
    ids = torch.arange(N_VIDEOS, dtype=torch.int32, device=DEV)
    first = epoch.accumulate(_batches(feats, ids))   # (allocates the epoch's arrays)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = epoch.accumulate(_batches(feats, ids))
        totals = epoch.captions.totals_device()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second) and epoch.count == N_VIDEOS and int(totals[0]) == N_VIDEOS, "the pass starts from zero"
    small = TestEpoch(opt, model, bank, corpus, capacity=N_VIDEOS - 1, beam_size=1)
    with pytest.raises(ValueError, match="larger than its capacity 6"):
        small.run(_batches(feats, ids))
    assert small.captions is None and model.training, "refused before anything ran"
    with pytest.raises(ValueError, match="larger than its capacity 6"):
        small.accumulate(_batches(feats, ids))   # (batch by batch, for a loader whose sizes cannot be seen in advance)
    assert model.training
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        epoch.run([{"feats": [f.cpu() for f in _batches(feats)[0]["feats"]], "video_ids": [0, 1, 2]}])

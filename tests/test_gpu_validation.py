"""GPU: the validation epoch (care_amd/validation.py) on the smallest golden model of the training tests, a bank over 7 videos,
batches of 3, 3 and 1 clips, greedy and beam 5: the scores of `ValidationEpoch.run` against the Python reference
(tests/capmetrics_reference.py) on the captions `translate_batch` itself returns for the same batches - BLEU and ROUGE-L within
1e-12 (the integer totals are exact and a caption's ROUGE-L is a few ulps of a double off, see tests/test_gpu_capmetrics_kernels.py),
CIDEr within the 2e-6 of tests/test_gpu_reward_kernels.py (per-caption scores are fp32).  A second epoch - under
torch.cuda.set_sync_debug_mode("error") up to the one read - gives the same bits; the model's mode comes back.

Measured on one MI355X (greedy / beam 5): Bleu_4 0.078 / 0.019, ROUGE_L 0.143 / 0.064 - equal to the reference's to the last bit;
CIDEr 0.193 / 0.068, 1.5e-9 / 5.3e-10 off the float64 value (bar 2e-6).  The three tests: 0.9 s."""
import gc

import numpy as np
import pytest
import torch

import capmetrics_reference as M
from conftest import GoldenCase
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

NAME = "msrvtt_base_ami_b2"
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
SAMPLER = dict(temperature=0.5, top_k=2, top_p=1.0)   # references close to what the model decodes, so that n-grams match
CIDER_BAR = 2e-6
N_VIDEOS, SPLIT = 7, ((0, 3), (3, 6), (6, 7))
_state = {}


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _model():
    """The `_model()` recipe of tests/test_gpu_scst.py, with features for 7 clips from the same generator."""
    from care_amd import get_framework
    from care_amd.configs import feat_shapes
    from care_amd.synth import synth_feats

    case = GoldenCase(NAME)
    opt, P, _, _ = case.build()
    opt.update(NO_DROP)
    if "feats" not in _state:
        _state["feats"] = synth_feats(case.meta["seed"] + 1, feat_shapes(opt, N_VIDEOS))
    model = get_framework(opt)
    model.load_state_dict(P, strict=True)
    return opt, [f.to(DEV) for f in _state["feats"]], model.to(DEV).train()


def _refs():
    """Per video four captions the model itself samples, narrowly (two tokens a step at temperature 0.5).  Built once."""
    if "refs" not in _state:
        opt, feats, model = _model()
        model.eval()
        with torch.no_grad(), model.engine().lock:
            out = model.engine().translate_sample(feats, 4, seed=100, use_graph=False, **SAMPLER)
            fed, length = out[1].cpu().numpy(), out[2].cpu().numpy()
        _state["refs"] = [[fed[c * 4 + j, 1: length[c * 4 + j] + 1].tolist() for j in range(4)] for c in range(N_VIDEOS)]
    return _state["refs"]


def _batches(feats, ids=None):
    return [{"feats": [f[lo:hi] for f in feats], "video_ids": list(range(lo, hi)) if ids is None else ids[lo:hi]} for lo, hi in SPLIT]


@pytest.mark.parametrize("beam_size", [1, 5], ids=["greedy", "beam5"])
def test_the_epoch_scores_what_translate_batch_returns(beam_size):
    from care_amd import MetricBank, ValidationEpoch, get_translator

    opt, feats, model = _model()
    refs = _refs()
    bank = MetricBank(refs, opt["vocab_size"], device=DEV)
    epoch = ValidationEpoch(opt, model, bank, beam_size=beam_size)
    got = epoch.run(_batches(feats))
    assert model.training, "the caller's mode comes back"
    model.eval()

    # the yardstick: the captions translate_batch returns first, scored in plain Python
    translator = get_translator(dict(opt, beam_size=beam_size))
    corpus, rows = M.Corpus(refs), []
    for batch in _batches(feats):
        hyps, _ = translator.translate_batch([model], {"feats": batch["feats"]})
        rows += [(h[0], len(h[0]), v) for h, v in zip(hyps, batch["video_ids"])]
    records = corpus.records(*zip(*rows))
    want = corpus.corpus(records)
    print(beam_size, "captions", [r[0] for r in rows][:2], "\nwant", want, "\ngot", got)
    assert got["n_captions"] == 7.0 and got["n_invalid"] == 0.0 and want["n_captions"] == 7.0
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert abs(got["CIDEr"] - want["CIDEr"]) <= CIDER_BAR and abs(got["Sum"] - want["Sum"]) <= CIDER_BAR + 2e-12
    assert got["Bleu_1"] > 0 and got["ROUGE_L"] > 0, "the references must share tokens with the decoded captions"
    assert not model.training and epoch.last == got

    # once more, video_ids as a device tensor: nothing synchronises before the one read, and the bits are the first epoch's
    first = epoch.accumulate(_batches(feats))
    ids = torch.arange(N_VIDEOS, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = epoch.accumulate(_batches(feats, ids))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second) and not model.training
    scores, gave_up = epoch.scores(second)
    assert gave_up == 0 and scores == got, "a second run gives the same bits"


def test_refusals_by_name_and_the_mode_is_restored():
    from care_amd import MetricBank, ValidationEpoch

    opt, feats, model = _model()
    bank = MetricBank(_refs(), opt["vocab_size"], device=DEV)
    epoch = ValidationEpoch(opt, model, bank, beam_size=1)
    batches = _batches(feats)
    with pytest.raises(KeyError, match="video_ids"):
        epoch.run([{"feats": batches[0]["feats"]}])
    with pytest.raises(ValueError, match="video_ids"):
        epoch.run([{"feats": batches[0]["feats"], "video_ids": [0]}])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        epoch.run([{"feats": [f.cpu() for f in batches[0]["feats"]], "video_ids": [0, 1, 2]}])
    with pytest.raises(NotImplementedError, match="ensemble"):
        epoch.run([{"feats": [batches[0]["feats"], batches[0]["feats"]], "video_ids": [0, 1, 2]}])
    with pytest.raises(ValueError, match="no references"):
        epoch.run([{"feats": batches[2]["feats"], "video_ids": torch.tensor([N_VIDEOS], dtype=torch.int32, device=DEV)}])
    assert model.training, "a refusal leaves the caller's mode"
    one = epoch.run(iter(batches[2:]))   # a one-shot iterator
    assert one["n_captions"] == 1.0 and np.isfinite(one["Sum"]) and model.training

"""GPU: concept scoring in the validation epoch (care_amd/validation.py) and in NoisyOrMIL (care_amd/criterion.py).

A freshly initialised `msrvtt_care` model, a clip store of 6 videos, validate batches of 4 + 2 clips with `labels_attr`:
`ValidationEpoch.run`, greedy and beam 5, returns `mAP` / `F1-*` equal to tests/concept_reference.py evaluated on the
`preds_attr` the engine's own encode of the decode pass returns for the same batches (engine.encode, with the pass's kernel
forms), within the 1e-12 of tests/test_gpu_concept_kernels.py - the same double arithmetic on the same integers; `V-Attr Loss`
equals get_criterion(opt, skip_crit_list=['lang']) over the same batches (the same kernel on the same tensors: to fp32's 1e-6
relative at the most).  The caption scores are the bits of an epoch without `labels_attr`; the store's loader gives the numbers
of hand-made batches; a model without a concept head gains no key; a forced give-up retry starts the concept totals from
zero; nothing is read on the host inside the epoch.  NoisyOrMIL on device tensors matches the recorded reference over two
batches and keeps nothing between steps.

Measured on one MI355X (greedy and beam 5 alike: the encoder does not depend on the decode): mAP 0.0477 with the helper's to
1e-17, the six F1 equal to the last bit, `V-Attr Loss` 23.4176 equal to the criterion's; the first test 1.0 s (it builds the store and the model), every other below 0.2 s."""
import gc
import json

import numpy as np
import pytest
import torch

import concept_reference as R
from crit_reference import criterion_batches, load_case
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

N_VIDEOS, MAX_LEN, SPLIT = 6, 10, 4
BAR = 1e-12
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
CONCEPT_KEYS = ["F1-%02d" % k for k in R.TOPK_LIST] + ["mAP", "V-Attr Loss", "n_no_positive"]
_state = {}


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _opt(name="msrvtt_care"):
    from care_amd.configs import make_opt

    return make_opt(name, max_len=MAX_LEN, load_feats_type=0, **NO_DROP)


def _setup():
    """(opt, model, bank, batches): built once, never changed.  Captions over a small range of words, so that every video has
    concepts among the model's 500."""
    if "setup" not in _state:
        from care_amd import ClipStore, MetricBank, get_framework
        from care_amd.constants import BOS, EOS

        opt = _opt()
        rng = np.random.RandomState(66)
        names = ["video%d" % (7 * v + 1) for v in range(N_VIDEOS)]
        dbs = {"a": [{v: rng.randn(60, 128).astype(np.float32) for v in names}],
               "m": [{v: rng.randn(60, 2048).astype(np.float32) for v in names}],
               "i": [{v: rng.randn(60, 500).astype(np.float32) for v in names}, {v: rng.randn(12).astype(np.float32) for v in names}],
               "r": [{v: rng.randn(23, 512).astype(np.float32) for v in names}]}
        captions = {v: [[BOS] + rng.randint(6, 500, size=rng.randint(3, 9)).tolist() + [EOS] for _ in range(2 + k % 3)]
                    for k, v in enumerate(names)}
        store = ClipStore(opt, dbs, names, captions=captions, device=DEV)
        bank = MetricBank([[c[1:] for c in captions[v]] for v in names], opt["vocab_size"], with_eos=True, device=DEV)
        torch.manual_seed(11)
        model = get_framework(opt).to(DEV).train()
        batches = []
        for b in store.loader(mode="validate", batch_size=SPLIT, depth=2):   # copies: the loader's slots are its own
            batches.append({"feats": [f.clone() for f in b["feats"]], "video_ids": b["video_ids"].clone(),
                            "labels_attr": b["labels_attr"].clone()})
        assert [b["video_ids"].numel() for b in batches] == [4, 2]
        _state["setup"] = (opt, model, bank, batches, store)
    return _state["setup"]


def _pass_preds(epoch, model, feats):
    """`preds_attr` of the decode pass the epoch runs for these features (engine.encode's output of that pass)."""
    engine = model.engine()
    with torch.no_grad(), engine.lock:
        enc = epoch._decode(engine, list(feats))[2]
        plain = engine.encode(list(feats))["preds_attr"]
        assert torch.allclose(enc["preds_attr"], plain, atol=1e-5, rtol=0), "the pass's concept probabilities are the encoder's"
        return enc["preds_attr"].clone()


@pytest.mark.parametrize("beam_size", [1, 5], ids=["greedy", "beam5"])
def test_the_epoch_reports_the_concept_metrics_of_its_own_predictions(beam_size):
    from care_amd import ValidationEpoch, get_criterion

    opt, model, bank, batches, _ = _setup()
    epoch = ValidationEpoch(opt, model, bank, beam_size=beam_size)
    got = epoch.run(batches)
    assert model.training and set(CONCEPT_KEYS) <= set(got)
    assert epoch.concept[1].tolist() == [N_VIDEOS, got["n_no_positive"]]

    model.eval()
    try:
        preds = [_pass_preds(epoch, model, b["feats"]) for b in batches]
        crit = get_criterion(opt, skip_crit_list=["lang"])
        crit.reset_loss_recorder()
        for p, b in zip(preds, batches):
            crit.get_loss({"preds_attr": p, "avg_prob_attr": None, "labels_attr": b["labels_attr"]})
        info = crit.get_loss_info()
    finally:
        model.train()
    want = R.epoch([(p.cpu().numpy(), b["labels_attr"].cpu().numpy()) for p, b in zip(preds, batches)])
    print(beam_size, "want", want, "\ngot", {k: got[k] for k in CONCEPT_KEYS}, "\ncriterion", info)
    assert want["n_no_positive"] == got["n_no_positive"] == 0 and 0 < got["mAP"] <= 1
    for k in CONCEPT_KEYS[:7]:
        assert abs(got[k] - want[k]) <= BAR, (k, got[k], want[k])
        assert abs(info[k] - want[k]) <= BAR if k != "mAP" else "mAP" not in info, "the training-side criterion: F1 only"
    assert abs(got["V-Attr Loss"] - info["V-Attr"]) <= 1e-6 * abs(info["V-Attr"]), (got["V-Attr Loss"], info["V-Attr"])

    # the caption scores are the bits of an epoch that scores no concepts, and that epoch gains no key
    bare = ValidationEpoch(opt, model, bank, beam_size=beam_size).run([{k: v for k, v in b.items() if k != "labels_attr"} for b in batches])
    assert not set(CONCEPT_KEYS) & set(bare)
    assert bare == {k: v for k, v in got.items() if k not in CONCEPT_KEYS}


def test_nothing_is_read_inside_the_epoch_and_the_loader_gives_the_same_numbers():
    from care_amd import ValidationEpoch

    opt, model, bank, batches, store = _setup()
    epoch = ValidationEpoch(opt, model, bank, beam_size=1)
    want = epoch.run(batches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        state = epoch.accumulate(batches)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(state.shape) == (15,) and state.dtype == torch.int64, "the state keeps its shape and meaning"
    scores, gave_up = epoch.scores(state)
    assert gave_up == 0 and scores == want, "a second epoch gives the same bits"
    got = ValidationEpoch(opt, model, bank, beam_size=1).run(store.loader(mode="validate", batch_size=SPLIT, depth=2))
    assert got == want and "mAP" in got


def test_a_clip_without_a_positive_is_counted_and_makes_the_means_nan():
    from care_amd import ValidationEpoch

    opt, model, bank, batches, _ = _setup()
    holed = [dict(b) for b in batches]
    holed[1]["labels_attr"] = batches[1]["labels_attr"].clone()
    holed[1]["labels_attr"][0, : opt["attribute_prediction_k"]] = 0
    got = ValidationEpoch(opt, model, bank, beam_size=1).run(holed)
    assert got["n_no_positive"] == 1 and np.isnan(got["mAP"]) and all(np.isnan(got[k]) for k in CONCEPT_KEYS[:6])
    assert np.isfinite(got["V-Attr Loss"]) and np.isfinite(got["Sum"])


def test_a_give_up_retry_starts_the_concept_totals_from_zero():
    from care_amd import ValidationEpoch
    from care_amd.capmetrics import TOTALS

    opt, model, bank, batches, _ = _setup()
    plain = ValidationEpoch(opt, model, bank, beam_size=1).run(batches)
    epoch = ValidationEpoch(opt, model, bank, beam_size=1)
    inner, calls = epoch.accumulate, []

    def accumulate(batches, resident=True):
        state = inner(batches, resident=resident)
        calls.append(resident)
        if resident:
            state[TOTALS] += 1   # as if a resident launch had given up on one row
        return state

    epoch.accumulate = accumulate
    got = epoch.run(batches)
    assert calls == [True, False]
    assert epoch.concept[1].tolist() == [N_VIDEOS, 0], "six clips, not twelve"
    # (the multi-launch decodes may encode through other kernel forms: fp32 rounding of the probabilities, not a doubled sum)
    assert abs(got["V-Attr Loss"] - plain["V-Attr Loss"]) <= 1e-5 * plain["V-Attr Loss"]
    assert abs(got["mAP"] - plain["mAP"]) <= 1e-3 and abs(got["F1-50"] - plain["F1-50"]) <= 5e-2


def test_a_model_without_a_concept_head_gains_nothing():
    from care_amd import ValidationEpoch, get_framework

    _, _, bank, batches, _ = _setup()
    opt = _opt("msrvtt_base_ami")
    torch.manual_seed(12)
    model = get_framework(opt).to(DEV).train()
    calls = []
    from care_amd import _lib
    real = _lib.call

    def spy(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)

    fed = [dict(b, feats=b["feats"][:3]) for b in batches]   # modality "ami" of the same clips, `labels_attr` still there
    _lib.call = spy
    try:
        got = ValidationEpoch(opt, model, bank, beam_size=1).run(fed)
    finally:
        _lib.call = real
    assert not set(CONCEPT_KEYS) & set(got) and got["n_captions"] == float(N_VIDEOS)
    assert "care_concept_metrics" not in calls and "care_noisy_or_bce_fwd" not in calls and "care_caption_totals" in calls


def test_noisy_or_mil_on_device_tensors_matches_the_record_and_keeps_nothing():
    from care_amd import NoisyOrMIL

    z = load_case("criterion_two_batches")
    want = json.loads(str(z["info_json"]))
    batches = criterion_batches(z)
    crit = NoisyOrMIL({"calculate_mAP": True})
    crit.reset_recorder()
    P_max = 0
    for _, _, preds, labels_attr in batches:
        crit({"preds_attr": preds.to(DEV), "avg_prob_attr": None, "labels_attr": labels_attr.to(DEV)})
        P_max = max(P_max, int((labels_attr[:, : preds.shape[1]] != 0).sum(1).max()))
    held = [v for v in vars(crit).values() if torch.is_tensor(v)]
    assert not any(isinstance(v, (list, tuple, dict)) and len(v) and any(torch.is_tensor(x) or isinstance(x, tuple) for x in v)
                   for k, v in vars(crit).items() if k != "topk_list"), "no per-batch tensors"
    assert not hasattr(crit, "ap_pending") and sum(t.numel() for t in held) == 8 + 2, "the recorder's doubles and the two counts"
    names, info = crit.get_info()
    assert names == ["F1-%02d" % k for k in R.TOPK_LIST] + ["mAP"]
    bar = (P_max + 4) * 2.0 ** -24   # the reference's own fp32 evaluation (tests/test_concept_metrics_cpu.py)
    helper = R.epoch([(p.numpy(), y.numpy()) for _, _, p, y in batches])
    for k, v in zip(names, info):
        assert abs(v - want[k]) <= bar * abs(want[k]), (k, v, want[k])
        assert abs(v - helper[k]) <= BAR, (k, v, helper[k])
    off = NoisyOrMIL({})
    off.reset_recorder()
    off({"preds_attr": batches[0][2].to(DEV), "avg_prob_attr": None, "labels_attr": batches[0][3].to(DEV)})
    assert off.get_info()[0] == names[:-1] and len(off.get_info()[1]) == 6

"""CPU: the training criteria's yardstick and host interface (care_amd/criterion.py).

1. tests/crit_reference.py - the restatement of misc/Crit's two formulas the GPU tests measure the kernels against - evaluated
   in float64 reproduces every fixture of tests/golden/crit, which tools/gen_crit_golden.py recorded from the genuine
   reference (fp32): loss to 1e-6 relative, every gradient element to 1e-6 of the gradient's largest magnitude, the info
   values to 1e-6 relative (word accuracy: exactly).
2. get_criterion gives the reference's names and scales for the shipped configurations; what the HIP criteria do not cover is
   refused with the option named; CPU tensors raise (no fallback)."""
import json

import numpy as np
import pytest
import torch

from crit_reference import (bce_step, crit_cases, criterion_batches, criterion_opt, info_of_batches, lang_counts, lang_step,
                            load_case, total_loss)

REL = 1e-6


def _close(got, want, what):
    assert abs(got - want) <= REL * abs(want), (what, got, want)


def _grad_close(got, want, what):
    want = torch.as_tensor(want).double()
    assert got.shape == want.shape, what
    assert float((got - want).abs().max()) <= REL * float(want.abs().max()), (what, float((got - want).abs().max()))


def test_fixture_set_is_what_the_tests_expect():
    assert crit_cases("lang") == ["lang_v131", "lang_v131_drop_last", "lang_v2003"]
    assert crit_cases("attr") == ["attr_b3", "attr_b3_no_positive"]
    assert crit_cases("criterion") == ["criterion_two_batches"]
    z = load_case("lang_v131_drop_last")
    assert z["logits"].shape[1] == z["labels"].shape[1] + 1
    z = load_case("lang_v131")
    assert (z["labels"] == 0).mean() > 0.5                               # mostly PAD
    z = load_case("attr_b3_no_positive")
    K = z["preds_attr"].shape[1]
    assert z["labels_attr"].shape[1] > K and (z["labels_attr"][:, :K].sum(1) == 0).sum() == 1
    assert (z["preds_attr"] < 0.01).any() and (z["preds_attr"] > 0.99).any()


@pytest.mark.parametrize("name", ["lang_v131", "lang_v131_drop_last", "lang_v2003"])
def test_float64_restatement_reproduces_the_reference_language_loss(name):
    z = load_case(name)
    labels = torch.from_numpy(z["labels"])
    for i, eps in enumerate(z["eps"].tolist()):
        x = torch.from_numpy(z["logits"]).double().requires_grad_(True)
        den = float(x.shape[0])
        assert den == float(z["denominator"][i])
        loss = lang_step(x, labels, eps) / den
        loss.backward()
        _close(float(loss.detach()), float(z["loss"][i]), (name, eps, "loss"))
        _grad_close(x.grad, z["dlogits"][i], (name, eps, "dlogits"))
        hits, words, nlogp = lang_counts(x.detach(), labels)
        assert hits / words == z["info"][i][0]
        _close(np.exp(nlogp / words), z["info"][i][1], (name, eps, "Perplexity"))
        if x.shape[1] == labels.shape[1] + 1:
            assert float(x.grad[:, -1].abs().max()) == 0.0                # the dropped position gets no gradient
        assert float(x.grad[:, : labels.shape[1]][labels.eq(0)].abs().max()) == 0.0   # PAD positions neither


@pytest.mark.parametrize("name", ["attr_b3", "attr_b3_no_positive"])
def test_float64_restatement_reproduces_the_reference_concept_loss(name):
    from care_amd.metrics import concept_metrics

    z = load_case(name)
    labels = torch.from_numpy(z["labels_attr"])
    x = torch.from_numpy(z["preds_attr"]).double().requires_grad_(True)
    den = float(x.shape[0])
    assert den == float(z["denominator"])
    loss = bce_step(x, labels) / den
    loss.backward()
    _close(float(loss.detach()), float(z["loss"]), (name, "loss"))
    _grad_close(x.grad, z["dpreds"], (name, "dpreds"))
    p = torch.from_numpy(z["preds_attr"])
    outside = (p < 0.01) | (p > 0.99)
    assert outside.any() and float(x.grad[outside].abs().max()) == 0.0    # torch.clamp passes no gradient outside [0.01, 0.99]
    names = json.loads(str(z["info_names"]))
    assert names == ["F1-05", "F1-10", "F1-20", "F1-30", "F1-40", "F1-50", "mAP"]
    c = concept_metrics(p, labels, calculate_mAP=True)
    np.testing.assert_allclose([c[n] for n in names], z["info"], rtol=1e-6, atol=0, equal_nan=True)
    if name == "attr_b3_no_positive":
        assert np.isnan(z["info"]).all()   # the reference divides by the clip's zero positives: F1 and mAP are NaN there


def test_float64_restatement_reproduces_the_reference_criterion_over_two_batches():
    z = load_case("criterion_two_batches")
    opt = criterion_opt(z)
    batches = criterion_batches(z)
    assert batches[0][0].shape[0] != batches[1][0].shape[0]               # different sizes: the recorder weighting matters
    assert json.loads(str(z["names"])) == ["Lang Loss", "V-Attr"]
    scales = z["scales"].tolist()
    assert scales == [opt["language_generation_scale"], opt["attribute_prediction_scales"][0]]
    for b, (logits, labels, preds, labels_attr) in enumerate(batches):
        x, p = logits.double().requires_grad_(True), preds.double().requires_grad_(True)
        loss = total_loss({"logits": x, "preds_attr": p}, labels, labels_attr, opt["label_smoothing"], scales)
        loss.backward()
        _close(float(loss.detach()), float(z["loss"][b]), ("batch", b))
        _grad_close(x.grad, z["b%d_dlogits" % b], ("dlogits", b))
        _grad_close(p.grad, z["b%d_dpreds" % b], ("dpreds", b))
    want = json.loads(str(z["info_json"]))
    got = info_of_batches(batches, opt["label_smoothing"])
    assert list(got) == list(want)
    for k in want:
        _close(got[k], want[k], k)


def test_get_criterion_names_and_scales_of_the_shipped_configurations():
    from care_amd import get_criterion
    from care_amd.configs import CONFIG_NAMES, make_opt
    from care_amd.criterion import Criterion, LanguageGeneration, NoisyOrMIL

    for name in CONFIG_NAMES:
        opt = make_opt(name)
        crit = get_criterion(opt)
        assert isinstance(crit, Criterion)
        if "attribute" in opt["crits"]:
            assert crit.names == ["Lang Loss", "V-Attr"] and crit.scales == [1.0, 1.0], name
            assert isinstance(crit.crit_objects[0], LanguageGeneration) and isinstance(crit.crit_objects[1], NoisyOrMIL)
            assert crit.crit_objects[1].get_fieldsnames() == ["F1-05", "F1-10", "F1-20", "F1-30", "F1-40", "F1-50"]
            # Wrapper.py:421: the eval criterion - no language loss, mAP on
            ev = get_criterion(opt, skip_crit_list=["lang"], override_opt={"calculate_mAP": True})
            assert ev.names == ["V-Attr"] and ev.crit_objects[0].get_fieldsnames()[-1] == "mAP"
            assert "calculate_mAP" not in opt                             # override_opt works on a copy
        else:
            assert crit.names == ["Lang Loss"] and crit.scales == [1.0], name
        assert crit.crit_objects[0].get_fieldsnames() == ["Word Acc0", "Perplexity"]
        assert crit.crit_objects[0].label_smoothing == 0.0 and crit.crit_objects[0].keys == ["logits", "labels", "probs"]
    opt = make_opt("msrvtt_care", label_smoothing=0.1, language_generation_scale=0.8, attribute_prediction_scales=[0.3])
    crit = get_criterion(opt)
    assert crit.scales == [0.8, 0.3] and crit.crit_objects[0].label_smoothing == 0.1
    crit.set_scales([1.0, 0.5])
    assert crit.scales == [1.0, 0.5]
    assert get_criterion(opt, skip_crit_list=["lang", "attribute"]) is None
    assert get_criterion(opt).get_loss_info()["Perplexity"] == 1.0        # nothing recorded: AverageMeter's zeros


@pytest.mark.parametrize("over,named", [
    (dict(visual_word_generation=True), "visual_word_generation"),
    (dict(attribute_prediction_flags="VH"), "attribute_prediction_flags"),
    (dict(attribute_prediction_flags="H"), "attribute_prediction_flags"),
    (dict(attribute_prediction_sparse_sampling=True), "attribute_prediction_sparse_sampling"),
    (dict(crits=["lang", "length"]), "length"),
    (dict(crits=["lang", "attribute", "attn"]), "attn"),
    (dict(use_attr_type="prefix"), "prefix"),
    (dict(use_attr_type="pp"), "pp"),
])
def test_what_the_hip_criteria_do_not_cover_is_refused_by_name(over, named):
    from care_amd import get_criterion
    from care_amd.configs import make_opt

    with pytest.raises(NotImplementedError, match=named):
        get_criterion(make_opt("msrvtt_care", **over))


def test_a_probs_entry_is_refused_and_cpu_tensors_raise():
    from care_amd import LanguageGeneration, NoisyOrMIL, get_criterion
    from care_amd.configs import make_opt

    z = load_case("lang_v131")
    logits, labels = torch.from_numpy(z["logits"]), torch.from_numpy(z["labels"])
    lang = LanguageGeneration({"label_smoothing": 0.1})
    with pytest.raises(NotImplementedError, match="probs"):
        lang({"logits": logits, "labels": labels, "probs": torch.softmax(logits, -1)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lang({"logits": logits, "labels": labels})
    a = load_case("attr_b3")
    attr = NoisyOrMIL({})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attr({"preds_attr": torch.from_numpy(a["preds_attr"]), "avg_prob_attr": None, "labels_attr": torch.from_numpy(a["labels_attr"])})
    crit = get_criterion(make_opt("msrvtt_care"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit.get_loss({"logits": logits, "labels": labels, "preds_attr": torch.from_numpy(a["preds_attr"]),
                       "labels_attr": torch.from_numpy(a["labels_attr"])})

"""CPU: the oracle against the GENUINE reference on the options the other fixtures do not cover - the shapes
tests/test_gpu_parity.py::test_options_outside_the_shipped_configurations_... and test_other_caption_lengths_... then hold the
HIP path to.  The reference's captions, scores and parameter names / shapes are recorded in tests/golden/option_variants.json
(`python -m oracle.gen_golden option_variants`); the inputs are regenerated from the seed and checked against stored hashes."""
import json
import os

import pytest

from care_amd.configs import feat_shapes, make_opt
from care_amd.synth import synth_feats, synth_state_dict, tensor_sha256
from oracle import care_cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_variants.json")
with open(GOLDEN) as _fh:
    CASES = json.load(_fh)["cases"]
VARIANTS = [(name, c["config"], c["overrides"]) for name, c in CASES.items() if name != "prefix_guidance"]


def _case(name):
    """(opt, state dict, feats, parameter shapes) of a recorded case, regenerated from its seed and checked against the
    hashes of what the reference saw."""
    c = CASES[name]
    opt = make_opt(c["config"], beam_size=c["beam_size"], topk=c["topk"], **c["overrides"])
    shapes = [(k, tuple(s)) for k, s in c["state_dict"]]
    row_scale = {k: {int(r): f for r, f in v.items()} for k, v in c["row_scale"].items()}
    sd = synth_state_dict(c["seed"], shapes, row_scale=row_scale)
    feats = synth_feats(c["seed"], feat_shapes(opt, c["batch"]))
    assert tensor_sha256(feats[0]) == c["sha256"]["feats0"]
    assert tensor_sha256(sd["cls_head.tgt_word_prj.weight"]) == c["sha256"]["cls_head.tgt_word_prj.weight"]
    return opt, sd, feats, shapes


@pytest.mark.parametrize("name,config,over", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_oracle_equals_the_reference_on_option_variants(name, config, over):
    opt, sd, feats, shapes = _case(name)
    r_hyps, r_scores = CASES[name]["hyps"], CASES[name]["scores"]
    hyps, scores = care_cpu.translate_batch(sd, opt, feats)
    assert hyps == r_hyps
    assert max(abs(a - b) for x, y in zip(scores, r_scores) for a, b in zip(x, y)) < 1e-5
    # and the module this repository builds for the same options has the reference's parameters, name by name
    from care_amd import get_framework as build
    assert [(k, tuple(v.shape)) for k, v in build(opt).state_dict().items()] == shapes


def test_prefix_guidance_is_a_layout_the_oracle_does_not_restate():
    """`use_attr_flags` Gp.. prepends the guidance vector to the decoder's input sequence (Embeddings.py:155-157); the oracle
    restates the additive form only and care_amd refuses the option (tests/test_host_cpu.py) - recorded here so that the gap is
    a known one: the reference and the oracle DO differ on it."""
    opt, sd, feats, _ = _case("prefix_guidance")
    assert care_cpu.translate_batch(sd, opt, feats)[0] != CASES["prefix_guidance"]["hyps"]

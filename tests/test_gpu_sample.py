"""GPU: sampled decoding end to end (care_amd/engine_sample.py, Translator_ARFormer.sample_batch) on golden fixtures of
2 - 4 clips; fp32 mode unless said.  What the sampler computes per row is held by tests/test_gpu_sample_kernel.py; here:
the token that was drawn is the token that was fed back, the samples of a clip read THAT clip's memory, the two scores are
what they claim to be, ended rows are frozen, and a captured graph replays with new settings."""
import numpy as np
import pytest
import torch

import sample_reference as R
from conftest import GoldenCase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETTINGS = [dict(temperature=1.0, top_k=0, top_p=1.0), dict(temperature=0.7, top_k=20, top_p=0.9)]
_models = {}


def _case(name, mode="fp32"):
    """(opt, P, device feats, model, translator) of a fixture; one model per (fixture, mode) for the whole module."""
    from care_amd import get_framework, get_translator

    opt, P, feats, _ = GoldenCase(name).build()
    if (name, mode) not in _models:
        model = get_framework(opt).eval()
        model.load_state_dict(P, strict=True)
        model.set_compute_dtype(mode)
        _models[name, mode] = model.to(DEV)
    return opt, P, feats, [f.to(DEV) for f in feats], _models[name, mode], get_translator(opt)


def _raw(model, feats, n, seed, steps=None, use_graph=False, **kw):
    """engine.translate_sample -> numpy copies of (fed, length, score, score_q)."""
    with torch.no_grad(), model.engine().lock:
        out = model.engine().translate_sample(feats, n, seed=seed, use_graph=use_graph, steps=steps, **kw)[1:]
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in out]


@pytest.mark.parametrize("name", ["msrvtt_care_b2", "msrvtt_base_ami_eos_b4", "msrvtt_cabase_b3"])
def test_top_k_1_is_the_greedy_decode(name):
    opt, P, _, feats, model, tr = _case(name)
    ref_hyps, ref_scores = GoldenCase(name).hyps()
    hyps, scores, logq = tr.sample_batch([model], {"feats": feats}, n_samples=1, top_k=1, temperature=2.0, seed=5, with_logq=True)
    assert hyps == ref_hyps
    for a, b, q in zip(scores, ref_scores, logq):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-4)
        assert q == [0.0] and all(isinstance(s, float) for s in a)   # one kept entry: drawn with probability 1
    assert all(isinstance(t, int) for hs in hyps for h in hs for t in h)


def _teacher_forced_sums(model, feats, fed, length):
    """Sum over each caption's own length of the label log-probabilities of the teacher-forced pass over the captions."""
    eng = model.engine()
    T = eng.T
    with torch.no_grad(), eng.lock:
        enc = model.encoding_phase(feats)
        ids = torch.from_numpy(fed[:, :T].copy()).to(DEV)
        labels = torch.from_numpy(fed[:, 1: T + 1].copy()).to(DEV)
        logp, _ = eng.score_teacher_forced(ids, labels, enc["encoder_hidden_states"], enc.get("semantic_hidden_states"),
                                           sem_embs=enc.get("semantic_embs"))
        logp = logp.cpu().numpy().astype(np.float64)
    return np.array([logp[r, : length[r]].sum() for r in range(fed.shape[0])])


@pytest.mark.parametrize("setting", SETTINGS, ids=["plain", "filtered"])
@pytest.mark.parametrize("name", ["msrvtt_care_b2", "msrvtt_cabase_b3"])
def test_scores_are_the_models_log_probabilities_of_the_tokens_fed_back(name, setting):
    """The sampled captions fed back through score_teacher_forced: the label log-probabilities over each caption's length
    sum to `score` within 1e-4 per token - not so if another token than the drawn one went into the next step, or if a
    sample attended to another clip's memory."""
    from care_amd.constants import EOS

    opt, P, _, feats, model, _ = _case(name)
    n = 3
    fed, length, score, score_q = _raw(model, feats, n, seed=11, **setting)
    assert fed.shape == (len(feats[0]) * n, opt["max_len"]) and (fed[:, 0] == 2).all() and (length >= 1).all()
    sums = _teacher_forced_sums(model, feats, fed, length)
    err = np.abs(sums - score) / length
    print(name, setting, "per-token error", err.max(), "lengths", length.tolist())
    assert err.max() <= 1e-4
    # a caption ends at its first EOS or runs to max_len - 1; the samples of a clip differ from one another somewhere
    for r in range(fed.shape[0]):
        toks = fed[r, 1: length[r] + 1].tolist()
        assert EOS not in toks[:-1] and (toks[-1] == EOS or length[r] == opt["max_len"] - 1)
    assert len({tuple(row) for row in fed.tolist()}) > len(feats[0])
    # the sampling distribution's own log-probability: never above 0, and the model's when nothing is filtered or scaled
    assert (score_q <= 0).all()
    if setting["temperature"] == 1.0 and setting["top_k"] == 0 and setting["top_p"] == 1.0:
        np.testing.assert_allclose(score_q, score, rtol=0, atol=1e-4 * length.max())


@pytest.mark.parametrize("setting", SETTINGS, ids=["plain", "filtered"])
def test_tokens_against_the_oracle(setting):
    """oracle/care_cpu.py logits, teacher-forced on the device's captions, through the reference sampler with the same seed,
    key and step: it names the device's token at every position - but those it decides by less than the logits' own
    agreement (1e-4): a Gumbel margin under 2e-4 / temperature + 1e-4 or a nucleus margin under 5e-4; at most 2 %."""
    from oracle import care_cpu

    name, n, seed = "msrvtt_care_b2", 3, 21
    opt, P, cpu_feats, feats, model, _ = _case(name)
    fed, length, score, _ = _raw(model, feats, n, seed=seed, **setting)
    enc = care_cpu.encoding_phase(P, opt, cpu_feats)
    inputs = care_cpu.inputs_for_decoder(opt, enc)
    total = left_out = 0
    for r in range(fed.shape[0]):
        clip = r // n
        one = {k: v[clip: clip + 1] for k, v in inputs.items()}
        L = int(length[r])
        logits = care_cpu.decoding_phase(P, opt, torch.from_numpy(fed[r: r + 1, :L].astype(np.int64)), one)["logits"][0].numpy()
        logp = 0.0
        for t in range(1, L + 1):
            ref = R.sample_row(logits[t - 1], seed, clip * n + (r % n), t, **setting)
            total += 1
            if ref["gumbel_margin"] < 2e-4 / setting["temperature"] + 1e-4 or ref["nucleus_margin"] < 5e-4:
                left_out += 1
            else:
                assert ref["tok"] == int(fed[r, t]), (r, t, ref["tok"], int(fed[r, t]), ref["gumbel_margin"], ref["nucleus_margin"])
            x = logits[t - 1].astype(np.float64)
            logp += x[fed[r, t]] - (x.max() + np.log(np.exp(x - x.max()).sum()))
        assert abs(logp - score[r]) <= 1e-4 * L
    print(setting, "positions", total, "left out", left_out)
    assert left_out * 50 <= total


def test_same_seed_same_captions_and_graph_replay_with_new_settings():
    opt, P, _, feats, model, tr = _case("msrvtt_care_b2")
    batch = {"feats": feats}
    a = tr.sample_batch([model], batch, n_samples=3, seed=7, with_logq=True)
    b = tr.sample_batch([model], batch, n_samples=3, seed=7, with_logq=True)
    c = tr.sample_batch([model], batch, n_samples=3, seed=8, with_logq=True)
    assert a == b and a[0] != c[0]
    assert [len(h) for h in a[0]] == [3, 3] and [len(s) for s in a[1]] == [3, 3] and [len(q) for q in a[2]] == [3, 3]
    # seed None: from torch's generator
    torch.manual_seed(99)
    d = tr.sample_batch([model], batch, n_samples=2)
    torch.manual_seed(99)
    assert tr.sample_batch([model], batch, n_samples=2) == d
    # recycled input buffers: first call eager, second captured, third replayed - with a seed, then with settings, that the
    # graph has never seen - against the eager pass
    eng = model.engine()
    eng._graphs.clear()
    n = 4
    key_count = lambda: sum(1 for k in eng._graphs if k[0] == "sample")
    _raw(model, feats, n, seed=1, use_graph=True)
    _raw(model, feats, n, seed=2, use_graph=True)
    assert key_count() == 1 and not isinstance(next(v for k, v in eng._graphs.items() if k[0] == "sample"), str)
    for seed, kw in ((3, {}), (4, dict(temperature=0.6, top_k=30, top_p=0.85)), (5, dict(temperature=1.5)),
                     (6, dict(sample_ids=torch.tensor([9, 4])))):
        replayed = _raw(model, feats, n, seed=seed, use_graph=True, **kw)
        eager = _raw(model, feats, n, seed=seed, use_graph=False, **kw)
        for x, y in zip(replayed, eager):
            assert x.tobytes() == y.tobytes(), (seed, kw)
    assert key_count() == 1


def test_ended_rows_are_frozen_and_draws_come_back_in_order():
    """msrvtt_care_eos_b4: greedy ends three of its four clips within 3 tokens; its logits are nearly flat, so the draws are
    taken from the two best tokens (top_k 2), which ends most rows within a few steps (13 of 20 within 6 on the CPU oracle
    with this seed).  Columns behind a row's end hold what the frozen row went on drawing: `length` is what cuts them."""
    from care_amd.constants import EOS

    opt, P, _, feats, model, tr = _case("msrvtt_care_eos_b4")
    n, seed, kw = 5, 31, dict(temperature=1.0, top_k=2)
    hyps, scores, logq = tr.sample_batch([model], {"feats": feats}, n_samples=n, seed=seed, with_logq=True, **kw)
    fed, length, score, score_q = _raw(model, feats, n, seed=seed, **kw)
    T = opt["max_len"] - 1
    assert [len(h) for h in hyps] == [n] * 4
    for i in range(4):
        for j in range(n):   # draw order: list j of clip i is row i n + j
            r = i * n + j
            assert hyps[i][j] == fed[r, 1: length[r] + 1].tolist()
            assert EOS not in hyps[i][j][:-1] and (hyps[i][j][-1] == EOS or len(hyps[i][j]) == T)
            assert abs(scores[i][j] - float(score[r]) / float(length[r]) ** tr.beam_alpha) < 1e-12 and logq[i][j] == float(score_q[r])
    # a pass cut after S steps: the rows that had ended by then have their final tokens, length, score and logq
    S = 6
    fed_s, length_s, score_s, score_q_s = _raw(model, feats, n, seed=seed, steps=S, **kw)
    ended = np.array([EOS in fed_s[r, 1: S + 1].tolist() for r in range(4 * n)])
    print("ended within", S, "steps:", int(ended.sum()), "of", 4 * n, "lengths", length.tolist())
    assert 3 <= ended.sum() < 4 * n
    assert (fed_s[:, : S + 1] == fed[:, : S + 1]).all()
    for x, y in ((length_s, length), (score_s, score), (score_q_s, score_q)):
        assert x[ended].tobytes() == y[ended].tobytes()
    assert (length[ended] <= S).all()
    assert (length[~ended] > S).all() and (score[~ended] <= score_s[~ended]).all()


def test_fp16_mode_scores_are_consistent():
    name = "msrvtt_care_b2"
    opt, P, _, feats, model, _ = _case(name, "fp16")
    fed, length, score, _ = _raw(model, feats, 3, seed=11, temperature=0.7, top_k=20, top_p=0.9)
    sums = _teacher_forced_sums(model, feats, fed, length)
    err = np.abs(sums - score) / length
    print("fp16 per-token score error", err.max())
    assert err.max() <= 2e-2

"""GPU: Translator_ARFormer.consensus_batch end to end on the golden model msrvtt_care_peaked_b3 (3 clips) and a CiderBank of
random references: the caption it returns for a clip is one of the captions sample_batch draws with the same seed, with that
caption's score, and by the float64 reference (tests/consensus_reference.py) no other draw of the clip agrees more with the
rest by more than 1e-9; one draw comes back as it is; top_k = 1 makes every draw the greedy caption; a graph replay with another
seed and other settings agrees with the eager pass; `last_consensus` holds device tensors of the stated shapes."""
import functools

import numpy as np
import pytest
import torch

import cider_reference as C
import consensus_reference as R
from conftest import GoldenCase
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

NAME = "msrvtt_care_peaked_b3"
_state = {}


def _case():
    from care_amd import get_framework, get_translator

    opt, P, feats, _ = GoldenCase(NAME).build()
    if "model" not in _state:
        model = get_framework(opt).eval()
        model.load_state_dict(P, strict=True)
        model.set_compute_dtype("fp32")
        _state["model"] = model.to(DEV)
        _state["feats"] = [f.to(DEV) for f in feats]
    return opt, _state["feats"], _state["model"], get_translator(opt)


@functools.lru_cache(maxsize=None)
def _refs(vocab_size):
    rng = np.random.RandomState(11)
    return [[rng.randint(6, vocab_size, size=int(rng.randint(3, 12))).tolist() + [C.EOS] for _ in range(3)] for _ in range(12)]


def _bank(opt):
    from care_amd import CiderBank

    if "bank" not in _state:
        _state["bank"] = CiderBank(_refs(opt["vocab_size"]), opt["vocab_size"], device=DEV)
    return _state["bank"]


@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.7, top_k=20, top_p=0.9)], ids=["plain", "filtered"])
def test_the_winner_is_one_of_the_draws_and_none_agrees_more(kw):
    opt, feats, model, tr = _case()
    bank, batch, n, seed = _bank(opt), {"feats": feats}, 5, 17
    hyps, scores = tr.consensus_batch([model], batch, bank, n_samples=n, seed=seed, **kw)
    last = tr.last_consensus
    draws, draw_scores = tr.sample_batch([model], batch, n_samples=n, seed=seed, **kw)
    corpus = C.Corpus(_refs(opt["vocab_size"]))
    winner = last["winner"].cpu().tolist()
    assert [len(h) for h in hyps] == [1, 1, 1] and [len(s) for s in scores] == [1, 1, 1]
    for b in range(3):
        j = winner[b]
        assert 0 <= j < n and hyps[b][0] == draws[b][j] and scores[b][0] == draw_scores[b][j], (b, j)
        assert isinstance(scores[b][0], float) and all(isinstance(t, int) for t in hyps[b][0])
        ref, _, _ = R.clip(corpus, draws[b])
        got = last["consensus"][b].cpu().double().numpy()
        print(kw, "clip", b, "winner", j, "reference", ref, "device", got.tolist())
        assert np.abs(got - np.array(ref)).max() <= 2e-6
        assert ref[j] >= max(ref) - 1e-9
    # the device tensors
    T = opt["max_len"] - 1
    assert all(t.is_cuda for t in last.values()) and set(last) == {"tokens", "length", "score", "consensus", "winner"}
    assert tuple(last["tokens"].shape) == (3, T) and last["tokens"].dtype == torch.int32
    assert tuple(last["length"].shape) == (3,) and last["length"].dtype == torch.int32
    assert tuple(last["score"].shape) == (3,) and last["score"].dtype == torch.float32
    assert tuple(last["consensus"].shape) == (3, n) and last["consensus"].dtype == torch.float32
    assert tuple(last["winner"].shape) == (3,) and last["winner"].dtype == torch.int32
    for b in range(3):
        L = int(last["length"][b])
        assert last["tokens"][b, :L].tolist() == hyps[b][0]
        assert abs(float(last["score"][b]) / L ** tr.beam_alpha - scores[b][0]) < 1e-12


def test_one_draw_comes_back_and_top_k_1_is_the_greedy_caption():
    from care_amd import get_translator

    opt, feats, model, tr = _case()
    bank, batch = _bank(opt), {"feats": feats}
    hyps, scores = tr.consensus_batch([model], batch, bank, n_samples=1, seed=5)
    draws, draw_scores = tr.sample_batch([model], batch, n_samples=1, seed=5)
    assert hyps == draws and scores == draw_scores
    assert tr.last_consensus["winner"].tolist() == [0, 0, 0] and bool((tr.last_consensus["consensus"] == 0).all())
    # every draw the arg-max token: five copies of the greedy caption, the first wins
    hyps, scores = tr.consensus_batch([model], batch, bank, n_samples=5, top_k=1, temperature=2.0, seed=5)
    greedy, greedy_scores = get_translator(dict(opt, beam_size=1)).translate_batch([model], batch)
    assert [h[0] for h in hyps] == [g[0] for g in greedy]
    np.testing.assert_allclose([s[0] for s in scores], [g[0] for g in greedy_scores], rtol=0, atol=1e-4)
    assert tr.last_consensus["winner"].tolist() == [0, 0, 0]
    c = tr.last_consensus["consensus"].cpu()
    assert bool((c == c[:, :1]).all()), "copies of one caption agree alike"


def test_a_graph_replay_with_new_settings_agrees_with_the_eager_pass():
    opt, feats, model, tr = _case()
    bank, batch = _bank(opt), {"feats": feats}
    model.engine()._graphs.clear()
    tr.consensus_batch([model], batch, bank, n_samples=4, seed=1)   # eager, then captured: the same feature buffers
    tr.consensus_batch([model], batch, bank, n_samples=4, seed=2)
    assert sum(1 for k in model.engine()._graphs if k[0] == "sample") == 1
    for seed, kw in ((3, {}), (4, dict(temperature=0.6, top_k=30, top_p=0.85))):
        replayed = tr.consensus_batch([model], batch, bank, n_samples=4, seed=seed, **kw)
        state = {k: v.cpu().numpy().tobytes() for k, v in tr.last_consensus.items()}
        eager = tr.consensus_batch([model], batch, bank, n_samples=4, seed=seed, use_graph=False, **kw)
        assert replayed == eager, (seed, kw)
        assert state == {k: v.cpu().numpy().tobytes() for k, v in tr.last_consensus.items()}, (seed, kw)


def test_refusals():
    from care_amd import CiderBank

    opt, feats, model, tr = _case()
    bank, batch = _bank(opt), {"feats": feats}
    with pytest.raises(TypeError, match="CiderBank"):
        tr.consensus_batch([model], batch, object())
    with pytest.raises(RuntimeError, match="device=None"):
        tr.consensus_batch([model], batch, CiderBank(_refs(opt["vocab_size"]), opt["vocab_size"], device=None))
    with pytest.raises(ValueError, match="ONE model"):
        tr.consensus_batch([model, model], batch, bank)
    with pytest.raises(ValueError, match="n_samples"):
        tr.consensus_batch([model], batch, bank, n_samples=0)
    with pytest.raises(ValueError, match="n_samples"):
        tr.consensus_batch([model], batch, bank, n_samples=33)
    with pytest.raises(ValueError, match="temperature"):
        tr.consensus_batch([model], batch, bank, temperature=0.0)
    with pytest.raises(ValueError, match="top_p"):
        tr.consensus_batch([model], batch, bank, top_p=0.0)
    with pytest.raises(ValueError, match="no fallback path"):
        tr.consensus_batch([model], {"feats": [f.cpu() for f in feats]}, bank)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            tr.consensus_batch([model], batch, bank)
    finally:
        model.eval()

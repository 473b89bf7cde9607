"""No GPU: the float64 definition of the consensus among a clip's candidates (tests/consensus_reference.py) on hand-worked
anchors, the header / binding / libraries of care_consensus_score, and the refusals that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cider_reference as C
import consensus_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ESHAPE = -1, -2, -3


def _corpus(n_videos=40, with_eos=False):
    """n_videos x 5 references of 4 .. 15 tokens in [4, 60), most with a trailing EOS (EOS = 3 never inside)."""
    rng = np.random.RandomState(40)
    refs = []
    for _ in range(n_videos):
        video = []
        for _ in range(5):
            toks = rng.randint(4, 60, size=int(rng.randint(4, 16))).tolist()
            video.append(toks + [C.EOS] if rng.rand() < 0.8 else toks)
        refs.append(video)
    return refs, C.Corpus(refs, with_eos=with_eos)


def test_the_reference_on_hand_worked_anchors():
    refs, corpus = _corpus()
    a = next(r for video in refs for r in video if len(r) >= 9)[:7]   # seven tokens of the corpus
    assert any(corpus.df[(t,)] < 40 for t in a), "a unigram every video holds has weight 0"
    # identical candidates: every order's cosine is 1, the length penalty 1
    score, pair, winner = R.clip(corpus, [a, list(a)])
    assert abs(score[0] - 10.0) <= 1e-12 and abs(score[1] - 10.0) <= 1e-12 and winner == 0
    assert abs(pair[0][1] - 10.0) <= 1e-12 and pair[0][0] == 0.0 and pair[1][1] == 0.0
    # ... of three tokens: order 4 has no n-gram and adds 0
    score, _, _ = R.clip(corpus, [a[:3], a[:3]])
    assert abs(score[0] - 7.5) <= 1e-12 and abs(score[1] - 7.5) <= 1e-12
    # disjoint tokens
    score, pair, winner = R.clip(corpus, [[4, 5, 6, 7, 8], [20, 21, 22, 23, 24]])
    assert score == [0.0, 0.0] and pair[0][1] == 0.0 and winner == 0
    # tokens the corpus does not hold: df = 0, every weight tf ln N
    unseen = [3000, 3001, 3002, 3003, 3004]
    score, _, _ = R.clip(corpus, [unseen, list(unseen)])
    assert abs(score[0] - 10.0) <= 1e-12 and abs(score[1] - 10.0) <= 1e-12
    # the trailing EOS is dropped; a length cuts; the first m candidates are valid
    score, pair, winner = R.clip(corpus, [a + [C.EOS], a + [9, 9], a[::-1], a], lengths=[8, 7, 7, 7], m=2)
    assert abs(score[0] - 10.0) <= 1e-12 and abs(score[1] - 10.0) <= 1e-12 and score[2:] == [0.0, 0.0]
    assert pair[0][2] == 0.0 and pair[2][0] == 0.0 and pair[3] == [0.0] * 4 and winner == 0
    # three candidates, one unlike the two others: each of the two has ONE full and one partial agreement
    score, pair, winner = R.clip(corpus, [a[::-1], a, list(a)])
    assert winner == 1 and score[1] == score[2] > score[0]
    assert abs(score[1] - (pair[1][0] + pair[1][2]) / 2) <= 1e-12 and abs(pair[1][2] - 10.0) <= 1e-12
    # an empty candidate scores 0 and, as a reference, still counts in m - 1
    score, _, winner = R.clip(corpus, [a, [], list(a)])
    assert abs(score[0] - 5.0) <= 1e-12 and score[1] == 0.0 and winner == 0
    # m <= 1
    assert R.clip(corpus, [a])[0] == [0.0] and R.clip(corpus, [a])[2] == 0
    assert R.clip(corpus, [a, a], m=1) == ([0.0, 0.0], [[0.0, 0.0], [0.0, 0.0]], 0)
    assert R.clip(corpus, [a, a], m=0)[2] == -1
    # a bank of one video: ln N = 0, all weights 0
    one = C.Corpus(refs[:1])
    score, _, winner = R.clip(one, [a, list(a), a[:3]])
    assert score == [0.0, 0.0, 0.0] and winner == 0
    # rows of a batch
    toks = [a + [0], a + [0], a[:3] + [0] * 5, a[:3] + [0] * 5]
    s, p, w = R.clips(corpus, toks, [7, 7, 3, 3], 2)
    assert abs(s[0][0] - 10.0) <= 1e-12 and abs(s[1][1] - 7.5) <= 1e-12 and w == [0, 0] and len(p) == 2


def test_header_binding_and_libraries_agree_on_the_consensus_entry_point():
    from care_amd import _lib, build

    name = "care_consensus_score"
    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "consensus.hip" in build.SOURCES and build.SOURCES[-1] == "consensus.hip"
    build.build_all()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
    assert m, name
    params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert params[-1] == "void* stream"
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(params) == 16
    for ctype, decl in zip(sig, params):
        assert ctype is (ctypes.c_void_p if "*" in decl else ctypes.c_int), (decl, ctype)
    for variant in build.VARIANTS:
        assert hasattr(ctypes.CDLL(build.lib_path(variant)), name), variant
        assert _lib.load(variant=variant).care_version() == 25, "the ABI is additive"
    assert name in _lib.exported_symbols() and _lib.ABI_VERSION == 25
    assert int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1)) == 25
    assert int(re.search(r"#define CARE_CONSENSUS_MAX_N (\d+)", header).group(1)) == 32


def test_the_entry_point_refuses_before_any_launch():
    """Pointers that are never dereferenced (no GPU here: a launch would fail)."""
    from care_amd import _lib

    lib = _lib.load()
    P = 0x10000
    desc = _lib.CiderBankDesc()
    for k in ("corpus_keys", "corpus_lndf", "ref_keys", "ref_w", "ref_start", "ref_norm", "ref_len", "vid_start"):
        setattr(desc, k, P)
    desc.n_corpus, desc.n_videos, desc.n_refs, desc.ln_n = 3, 2, 2, 0.6931471805599453
    bank = ctypes.addressof(desc)

    def run(tokens=P, ld=30, col0=1, width=29, length=P, count=None, clips=0, n=5, bank_=bank, score=P, pairs=None, winner=P, row=None):
        return lib.care_consensus_score(tokens, ld, col0, width, length, count, clips, n, 0, 3, bank_, score, pairs, winner, row, None)

    assert run() == 0 and run(n=32, width=64, ld=65) == 0, "clips == 0 is a no-op"
    assert run(tokens=None) == EINVAL and run(length=None) == EINVAL and run(bank_=None) == EINVAL
    assert run(score=None) == EINVAL and run(winner=None) == EINVAL and run(clips=-1) == EINVAL and run(n=0) == EINVAL
    assert run(ld=29) == EINVAL and run(width=0) == EINVAL and run(col0=-1) == EINVAL
    assert run(n=33) == ESHAPE and run(clips=4, n=33) == ESHAPE, "at most 32 candidates a clip"
    assert run(width=65, ld=70) == ESHAPE, "at most 64 tokens a candidate"
    assert run(clips=2 ** 30, n=2) == ESHAPE
    for k in ("corpus_keys", "corpus_lndf"):
        setattr(desc, k, None)
        assert run() == EINVAL, k
        setattr(desc, k, P + 4)
        assert run() == EALIGN, k
        setattr(desc, k, P)
    desc.n_videos = 0
    assert run() == EINVAL


def test_python_refusals_need_no_gpu():
    from care_amd import CiderBank, _lib, consensus_select, get_translator

    refs, _ = _corpus(3)
    host = CiderBank(refs, 100, device=None)
    tokens, length = torch.zeros(10, 8, dtype=torch.int32), torch.ones(10, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device=None"):
        consensus_select(tokens, length, 5, host)
    with pytest.raises(TypeError, match="CiderBank"):
        consensus_select(tokens, length, 5, object())
    for n in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match="1 .. 32"):
            consensus_select(tokens, length, n, host)
    host.desc = _lib.CiderBankDesc()   # (stands in for device tables: what follows is refused before they are read)
    with pytest.raises(ValueError, match="not a multiple of n = 3"):
        consensus_select(tokens, length, 3, host)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consensus_select(tokens, length, 5, host)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consensus_select(tokens, length, 1, host)
    # the translator's entry
    tr = get_translator({"decoding_type": "ARFormer"})
    with pytest.raises(TypeError, match="CiderBank"):
        tr.consensus_batch([object()], {"feats": [torch.zeros(1, 2, 3)]}, object())
    with pytest.raises(ValueError, match="n_samples"):
        tr.consensus_batch([object()], {"feats": [torch.zeros(1, 2, 3)]}, host, n_samples=0)
    with pytest.raises(ValueError, match="ONE model"):
        tr.consensus_batch([object(), object()], {"feats": [torch.zeros(1, 2, 3)]}, host)
    with pytest.raises(ValueError, match="no fallback path"):
        tr.consensus_batch([object()], {"feats": [torch.zeros(1, 2, 3)]}, host)
    with pytest.raises(ValueError, match="temperature"):
        tr.consensus_batch([object()], {"feats": [torch.zeros(1, 2, 3)]}, host, temperature=0)

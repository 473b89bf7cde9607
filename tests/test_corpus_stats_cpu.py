"""CPU: the caption analysis of the test epoch without a GPU - the plain-Python yardstick (tests/corpus_reference.py) against the
fixtures recorded from the genuine reference (tests/golden/corpus, tools/gen_corpus_golden.py) with floats compared by `==`;
the key function and the host tables of care_amd.corpusstats.CorpusBank; every refusal of the banks and of TestEpoch that comes
before a launch; the descriptor layouts and the agreement of include/care_hip.h, care_amd/_lib.py and both libraries on the three
entry points; the per-sentence BLEU of care_amd.testepoch against the restatement."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import corpus_reference as R
from c_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("care_corpus_insert", "care_corpus_totals", "care_caption_model_score")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
REQUIRED = ("toy", "all_distinct_novel", "all_identical", "prefixes", "eos_pad", "random200")


def fixtures():
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*.json"))):
        case = json.load(open(path))
        out[case["name"]] = case
    return out


# ------------------------------------------------------------------------------------------------ the yardstick
def test_the_restatement_equals_every_fixture_exactly():
    cases = fixtures()
    assert set(REQUIRED) <= set(cases)
    for name, case in cases.items():
        got = R.analyze(case["train"], case["rows"])
        assert got == tuple(case["expected"]), (name, got, case["expected"])   # floats by ==
        assert isinstance(got[3], int)
        # the cut rows are to_sentence's words
        words = case["vocab"]
        assert [" ".join(words[t] for t in R.cut(r)) for r in case["rows"]] == case["captions"], name
        assert len({tuple(c) for c in case["train"]}) == case["n_train_distinct"], name
    assert tuple(cases["toy"]["expected"]) == (1.75, 0.25, 0.75, 4)
    t = R.totals(cases["random200"]["train"], [R.cut(r) for r in cases["random200"]["rows"]])
    assert 0 < t["n_novel"] < t["n_distinct"] < t["n_captions"] and t["n_empty"] == 2, "duplicates, novel and known captions all occur"


def test_the_empty_caption_is_one_empty_word_and_novel_unless_trained():
    assert R.analyze([[6]], [[3, 0]]) == (1.0, 1.0, 1.0, 1)
    assert R.analyze([[6], []], [[3, 0], [0, 6]]) == (1.0, 0.0, 0.5, 1)
    assert R.analyze([[6], []], [[6, 3], [3, 3]]) == (1.0, 0.0, 1.0, 2)
    assert R.cut([6, 7, 3, 8]) == (6, 7) and R.cut([6, 0, 7]) == (6,) and R.cut([6, 7, 8], 2) == (6, 7) and R.cut([6, 7], -1) == ()


# ------------------------------------------------------------------------------------------------ the key and the bank
def _key(caption, mask=(1 << 64) - 1):
    """The key in Python integers: (h(n, 64) + sum_j h(token_j, j)) & mask."""
    M = (1 << 64) - 1

    def fin(z):
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & M
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & M
        return z ^ (z >> 31)

    def h(a, i):
        return fin((a + 0x9E3779B97F4A7C15 * (i + 1)) & M)

    return (h(len(caption), 64) + sum(h(t, j) for j, t in enumerate(caption))) & M & mask


def test_the_key_function_in_numpy_is_the_integer_one():
    from care_amd.corpusstats import caption_key, caption_keys

    rng = np.random.RandomState(3)
    caps = [[], [0], [65535], [6, 7], [7, 6], [6, 7, 0]] + [rng.randint(0, 65536, size=int(rng.randint(1, 80))).tolist() for _ in range(50)]
    keys = caption_keys(caps)
    assert keys.dtype == np.uint64 and [int(k) for k in keys] == [_key(c) for c in caps]
    assert caption_key([6, 7]) != caption_key([7, 6]), "position-weighted"
    assert caption_key([6]) != caption_key([6, 0]) and caption_key([]) != 0
    assert [int(k) for k in caption_keys(caps, 0x7)] == [_key(c, 7) for c in caps]
    assert caption_keys([]).size == 0


def test_bank_tables_sorted_distinct_and_runs_of_equal_keys():
    from care_amd import CorpusBank
    from care_amd.corpusstats import caption_keys

    case = fixtures()["random200"]
    for mask in ((1 << 64) - 1, 0x7):
        bank = CorpusBank(case["train"], 46, device=None, key_mask=mask)
        h = bank.host
        assert bank.desc is None and bank.dev is None and bank.n_train == 500 and bank.n == case["n_train_distinct"]
        assert h["keys"].dtype == np.uint64 and h["start"].dtype == np.int64 and h["tokens"].dtype == np.int32
        assert np.all(h["keys"][1:] >= h["keys"][:-1]), "ascending keys"
        caps = [tuple(h["tokens"][h["start"][i]: h["start"][i + 1]].tolist()) for i in range(bank.n)]
        assert caps == bank.captions and len(set(caps)) == len(caps) and set(caps) == {tuple(c) for c in case["train"]}
        assert np.array_equal(caption_keys(caps, mask), h["keys"])
        if mask == 0x7:
            assert set(h["keys"].tolist()) <= set(range(8)) and np.bincount(h["keys"].astype(np.int64)).max() > 20, "long runs of equal keys"
        else:
            assert len(set(h["keys"].tolist())) == bank.n
        for c in case["train"][:40]:
            assert c in bank
        assert [6] * 9 not in bank and () in bank   # (train[17] is empty)
    empty = CorpusBank([], 10, device=None)
    assert empty.n == 0 and empty.host["start"].tolist() == [0] and [6] not in empty


def test_from_words_numbers_unknown_words_above_the_vocabulary():
    from care_amd import CorpusBank, MetricBank

    w2i = {"a": 6, "man": 7}
    bank = CorpusBank.from_words([["a", "man"], ["a", "dog"], ["cat", "dog"], []], w2i, vocab_size=10, device=None)
    assert bank.extra_words == {"dog": 10, "cat": 11} and bank.vocab_size == 12
    assert (6, 7) in bank and (6, 10) in bank and (11, 10) in bank and () in bank and (6, 1) not in bank
    metric = MetricBank.from_words([[["a", "dog"]], [["cat", "man"]]], w2i, vocab_size=10, device=None)
    assert metric.extra_words == bank.extra_words and metric.vocab_size == bank.vocab_size, "the numbering of MetricBank.from_words"
    with pytest.raises(ValueError, match="65536"):
        CorpusBank.from_words([["w%d" % i for i in range(20)]], {}, vocab_size=65530, device=None)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_the_banks():
    from care_amd import CorpusBank, EpochCaptions

    with pytest.raises(ValueError, match="vocab_size"):
        CorpusBank([[6]], 65537, device=None)
    with pytest.raises(ValueError, match="vocab_size"):
        CorpusBank([[6]], 0, device=None)
    with pytest.raises(ValueError, match="outside"):
        CorpusBank([[6, 50]], 50, device=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CorpusBank([[6]], 50, device="cpu")
    with pytest.raises(ValueError, match="key_mask"):
        CorpusBank([[6]], 50, device=None, key_mask=1 << 64)
    host = CorpusBank([[6]], 50, device=None)
    with pytest.raises(ValueError, match="power of two"):
        EpochCaptions(12, 50, host)
    with pytest.raises(ValueError, match="vocab_size"):
        EpochCaptions(16, 51, host)
    with pytest.raises(TypeError, match="CorpusBank"):
        EpochCaptions(16, 50, object())
    with pytest.raises(RuntimeError, match="device=None"):
        EpochCaptions(16, 50, host)


def test_the_test_epoch_refuses_by_name_before_anything_runs():
    from care_amd import CorpusBank, MetricBank, TestEpoch, get_framework
    from conftest import GoldenCase

    opt = GoldenCase("msrvtt_base_ami_b2").build()[0]
    V = opt["vocab_size"]
    model = get_framework(opt)
    bank = MetricBank([[[10, 11]], [[10, 12]]], V, device=None)
    corpus = CorpusBank([[10, 11]], V, device=None)
    with pytest.raises(NotImplementedError, match="ensemble"):
        TestEpoch(opt, [model, model], bank, corpus)
    with pytest.raises(NotImplementedError, match="topk"):
        TestEpoch(dict(opt, topk=2), model, bank, corpus)
    with pytest.raises(NotImplementedError, match="METEOR"):
        TestEpoch(opt, model, bank, corpus, metric_sum=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="vocab_size"):
        TestEpoch(opt, model, bank, CorpusBank([[10, 11]], V + 1, device=None))
    with pytest.raises(TypeError, match="CorpusBank"):
        TestEpoch(opt, model, bank, bank)
    with pytest.raises(ValueError, match="capacity"):
        TestEpoch(opt, model, bank, corpus, capacity=0)
    epoch = TestEpoch(dict(opt, seed=7), model, bank, corpus, capacity=3, beam_size=1)
    cpu = [torch.zeros(2, 4)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        epoch.run([{"feats": cpu, "video_ids": [0, 1]}])
    with pytest.raises(NotImplementedError, match="ensemble"):
        epoch.run([{"feats": [cpu, cpu], "video_ids": [0, 1]}])
    with pytest.raises(KeyError, match="seed"):
        TestEpoch({k: v for k, v in opt.items() if k != "seed"}, model, bank, corpus).run([])
    with pytest.raises(RuntimeError, match="device=None"):
        epoch.run([])   # (host-only banks: nothing to run on)

    class Sized(object):   # a stand-in for a device tensor: on "cuda", two clips
        device, shape = torch.device("cuda"), (2, 4)
    with pytest.raises(ValueError, match="larger than its capacity 3"):
        epoch._refuse([{"feats": [Sized()]}, {"feats": [Sized()]}])
    epoch._refuse([{"feats": [Sized()]}])


def test_per_sentence_bleu_is_the_restatement():
    from care_amd.testepoch import sentence_scores

    recs = [[1, 6, 6, 6, 5, 4, 3, 6, 5, 4, 3, 0], [1, 3, 6, 3, 2, 1, 0, 3, 2, 1, 0, 0], [1, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [1, 9, 7, 9, 8, 7, 6, 4, 1, 0, 0, 0], [1, 1, 2, 1, 0, 0, 0, 1, 0, 0, 0, 0]]
    rouge, cider = [1.0, 0.5, 0.0, 0.25, 0.75], np.asarray([5.0, 0.1, 0.0, 1.5, 0.3], dtype=np.float32)
    got = sentence_scores(np.asarray(recs, dtype=np.int32), np.asarray(rouge), cider)
    for g, rec, r, c in zip(got, recs, rouge, cider.tolist()):
        assert g == R.detail(rec, r, c)   # floats by ==
    assert abs(got[0]["Bleu_4"] - 1.0) < 1e-9 and got[2]["Bleu_1"] < 1e-5


# ------------------------------------------------------------------------------------------------ header, binding, libraries
def test_descriptor_layouts_are_the_headers():
    from care_amd import _lib

    for c_name, cls in (("care_corpus_bank", _lib.CorpusBankDesc), ("care_epoch_set", _lib.EpochSetDesc)):
        names = [f[0] for f in cls._fields_]
        got = c_layout(["sizeof({})".format(c_name)] + ["offsetof({}, {})".format(c_name, n) for n in names])
        assert got[0] == ctypes.sizeof(cls), c_name
        assert got[1:] == [getattr(cls, n).offset for n in names], c_name
    consts = c_layout(["CARE_CORPUS_MAX_CAPTION", "CARE_CORPUS_BITMAP_WORDS", "CARE_CORPUS_TOTALS", "CARE_CORPUS_N_CAPTIONS",
                       "CARE_CORPUS_LENGTH_SUM", "CARE_CORPUS_N_DISTINCT", "CARE_CORPUS_N_NOVEL", "CARE_CORPUS_N_EMPTY",
                       "CARE_CORPUS_USAGE", "CARE_CORPUS_N_OVERFLOW"])
    from care_amd.corpusstats import TOTAL_NAMES
    assert consts[:3] == [_lib.CORPUS_MAX_CAPTION, _lib.CORPUS_BITMAP_WORDS, _lib.CORPUS_TOTALS] == [64, 2048, 8]
    assert consts[3:] == list(range(7)) and TOTAL_NAMES == ("n_captions", "length_sum", "n_distinct", "n_novel", "n_empty", "usage", "n_overflow")
    assert _lib.CORPUS_BITMAP_WORDS * 32 == 65536


def test_header_binding_and_libraries_agree_on_the_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "corpus_stats.hip" in build.SOURCES
    build.build_all()
    for name in ENTRY_POINTS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "void* stream"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), name
        for ctype, decl in zip(sig, params):
            want = ctypes.c_void_p if "*" in decl else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            lib = ctypes.CDLL(build.lib_path(variant))
            assert hasattr(lib, name), (variant, name)
            assert lib.care_version() == _lib.ABI_VERSION == int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1))
    assert set(ENTRY_POINTS) <= set(_lib.exported_symbols())
    import care_amd
    assert {"CorpusBank", "EpochCaptions", "TestEpoch"} <= set(care_amd.__all__)
    assert issubclass(care_amd.TestEpoch, care_amd.ValidationEpoch)


@pytest.mark.parametrize("variant", ["", "f16"])
def test_refusals_come_before_any_launch(variant):
    """The argument checks of the three entry points with pointers that are never dereferenced (no GPU here: a launch would fail)."""
    from care_amd import _lib

    lib = _lib.load(variant=variant)
    P = 0x10000   # an aligned non-NULL address
    bank, st = _lib.CorpusBankDesc(), _lib.EpochSetDesc()
    bank.keys = bank.start = bank.tokens = P
    bank.n, bank.key_mask = 3, (1 << 64) - 1
    for k in ("slots", "tokens", "length", "keys", "bitmap", "totals"):
        setattr(st, k, P)
    st.capacity, st.key_mask = 8, (1 << 64) - 1
    pb, ps = ctypes.addressof(bank), ctypes.addressof(st)

    def insert(tokens=P, ld=30, col0=1, width=29, length=P, rows=4, cursor=0, bank_=pb, set_=ps, keys_out=None):
        return lib.care_corpus_insert(tokens, ld, col0, width, length, rows, cursor, 3, 0, bank_, set_, keys_out, None)

    assert insert(rows=0) == 0 and insert(rows=0, cursor=8) == 0, "rows == 0 is a no-op"
    assert insert(tokens=None) == EINVAL and insert(length=None) == EINVAL and insert(bank_=None) == EINVAL and insert(set_=None) == EINVAL
    assert insert(rows=-1) == EINVAL and insert(cursor=-1) == EINVAL and insert(width=0) == EINVAL and insert(col0=-1) == EINVAL
    assert insert(ld=29) == EINVAL, "ld below col0 + width"
    assert insert(width=65, ld=70) == ESHAPE and insert(width=64, ld=65, rows=0) == 0
    assert insert(rows=9) == ESHAPE and insert(rows=4, cursor=5) == ESHAPE and insert(rows=0, cursor=9) == ESHAPE, "beyond the remaining capacity"
    assert insert(keys_out=P + 4) == EALIGN and insert(keys_out=P, rows=0) == 0
    for cap in (0, 3, 12, -8):
        st.capacity = cap
        assert insert(rows=0) == ESHAPE and lib.care_corpus_totals(ps, None) == ESHAPE, cap
    st.capacity = 8
    for k in ("slots", "tokens", "length", "keys", "bitmap", "totals"):
        setattr(st, k, None)
        assert insert() == EINVAL and lib.care_corpus_totals(ps, None) == EINVAL, k
        setattr(st, k, P)
    for k in ("keys", "totals"):
        setattr(st, k, P + 4)
        assert insert() == EALIGN and lib.care_corpus_totals(ps, None) == EALIGN, k
        setattr(st, k, P)
    for k in ("keys", "start", "tokens"):
        setattr(bank, k, None)
        assert insert() == EINVAL, k
        setattr(bank, k, P)
    for k in ("keys", "start"):
        setattr(bank, k, P + 4)
        assert insert() == EALIGN, k
        setattr(bank, k, P)
    bank.n = -1
    assert insert() == EINVAL
    bank.n, bank.key_mask = 3, 7
    assert insert() == EINVAL, "one key mask for the bank and the set"
    bank.key_mask = (1 << 64) - 1
    assert lib.care_corpus_totals(None, None) == EINVAL

    def score(nfin=P, fscore=P, flen=P, B=4, cap=10, pw=P, n_pow=32, out=P):
        return lib.care_caption_model_score(nfin, fscore, flen, B, cap, pw, n_pow, out, None)

    assert score(B=0) == 0 and score(B=0, nfin=None) == 0 and score(B=0, cap=64) == 0
    for k in ("fscore", "flen", "pw", "out"):
        assert score(**{k: None}) == EINVAL, k
    assert score(B=-1) == EINVAL and score(cap=0) == EINVAL and score(cap=65) == EINVAL and score(n_pow=0) == EINVAL
    assert score(pw=P + 4) == EALIGN and score(out=P + 4) == EALIGN

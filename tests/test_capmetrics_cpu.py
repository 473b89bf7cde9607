"""CPU: the validation metrics without a GPU - the float64 yardstick (tests/capmetrics_reference.py) on hand-worked anchors, the
bit-parallel LCS recurrence of csrc/capmetrics.hip against the plain DP, the host tables of care_amd.capmetrics.MetricBank against
a brute-force count, `from_words`, the corpus formulas of `MetricBank.scores`, the refusals that come before any launch, and the
agreement of include/care_hip.h, care_amd/_lib.py and both libraries on the three entry points."""
import ctypes
import math
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

import capmetrics_reference as M
import cider_reference as C
from c_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("care_caption_stats", "care_caption_totals", "care_beam_winner")
EINVAL, EALIGN = -1, -2
EOS = C.EOS


# ------------------------------------------------------------------------------------------------ the yardstick itself
def test_hand_worked_anchors():
    a, b, c, d, e, f = 10, 11, 12, 13, 14, 15
    ref = [a, b, c, d, e, f]
    corpus = M.Corpus([[ref + [EOS]], [[a, b]]])
    # a candidate equal to a reference: every n-gram matches, no brevity penalty
    rec, rouge, _ = corpus.record(ref + [EOS], 7, 0)
    assert rec == [1, 6, 6, 6, 5, 4, 3, 6, 5, 4, 3, 0] and rouge == 1.0
    assert abs(M.bleu(rec[1], rec[2], rec[3:7], rec[7:11])[3] - 1.0) < 1e-9
    # no shared token: all zeros
    rec, rouge, cider = corpus.record([20, 21, 22], 3, 0)
    assert rec[7:11] == [0, 0, 0, 0] and rouge == 0.0 and cider == 0.0
    assert max(M.bleu(rec[1], rec[2], rec[3:7], rec[7:11])) < 1e-5
    # 3 candidate tokens against a 6-token reference: Bleu_1 = precision 1 times exp(1 - 6 / 3)
    rec, rouge, _ = corpus.record([a, b, c], 3, 0)
    assert rec[:3] == [1, 3, 6] and rec[7:11] == [3, 2, 1, 0]
    assert abs(M.bleu(rec[1], rec[2], rec[3:7], rec[7:11])[0] - math.exp(1 - 2)) < 1e-9
    p, r = 1.0, 0.5
    assert abs(rouge - (1 + 1.44) * p * r / (r + 1.44 * p)) < 1e-12
    # the closest length: 4 lies between 3 and 5 - the shorter one
    assert M.closest([5, 3, 9], 4) == 3 and M.closest([5, 3, 9], 8) == 9 and M.closest([5, 3], 0) == 3
    # clipping: "a a a a" against "a b"
    rec, _, _ = corpus.record([a, a, a, a], 4, 1)
    assert rec[3:7] == [4, 3, 2, 1] and rec[7:11] == [1, 0, 0, 0] and rec[2] == 2
    # the LCS of a sequence and its reverse (distinct tokens): one token
    assert M.lcs(ref, ref[::-1]) == 1 and M.lcs([a, b, a], [a, b, a][::-1]) == 3 and M.lcs([], ref) == 0
    assert M.lcs([a, b, c, b, d, a, b], [b, d, c, a, b, a]) == 4
    rec, rouge, _ = corpus.record(ref[::-1], 6, 0)
    assert abs(rouge - (1 / 6)) < 1e-12 and rec[7:11] == [6, 0, 0, 0]
    # an empty caption is a legitimate row; a length of 0, a video outside the corpus and a video without references are not
    rec, rouge, cider = corpus.record([EOS], 1, 0)
    assert rec == [1, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0] and rouge == 0.0 and cider == 0.0
    for length, video in ((0, 0), (-1, 0), (3, 2), (3, -1)):
        assert corpus.record([a, b, c], length, video) == ([0] * 12, 0.0, 0.0)
    assert M.Corpus([[], [[a]]]).record([a], 1, 0) == ([0] * 12, 0.0, 0.0)


def _lcs_bits(cand, ref):
    """The recurrence of caption_stats_kernel on one 64-bit word: bit j = candidate token j, per reference token
    M = the positions that hold it, U = V & M, V = (V + U) | (V & ~M) (the carry out of bit 63 dropped)."""
    L, mask = len(cand), (1 << 64) - 1
    V = mask
    for t in ref:
        m = sum(1 << j for j in range(L) if cand[j] == t)
        u = V & m
        V = ((V + u) & mask) | (V & ~m & mask)
    return bin(~V & ((1 << L) - 1)).count("1")


def test_the_bit_parallel_lcs_is_the_dp():
    rng = np.random.RandomState(11)
    for i in range(400):
        L = (1, 2, 63, 64)[i % 4] if i < 40 else int(rng.randint(1, 65))
        n = 100 if i % 50 == 0 else int(rng.randint(1, 70))
        vocab = (2, 4, 30)[i % 3]
        cand, ref = rng.randint(0, vocab, size=L).tolist(), rng.randint(0, vocab, size=n).tolist()
        assert _lcs_bits(cand, ref) == M.lcs(cand, ref), (cand, ref)
    same = list(range(64))
    assert _lcs_bits(same, same) == 64 and _lcs_bits(same, same[::-1]) == 1 and _lcs_bits([7] * 64, [7] * 100) == 64


# ------------------------------------------------------------------------------------------------ the bank
def _refs(rng):
    refs = []
    for v in range(7):
        video = []
        for _ in range(1 + v % 4):
            n = int(rng.randint(1, 12))
            toks = rng.randint(6, 14, size=n).tolist()
            if rng.rand() < 0.3:
                toks[rng.randint(n)] = 65535
            video.append(toks + [EOS])
        refs.append(video)
    refs[3].append(list(refs[3][0]))
    refs[5] = []                                  # a video without references
    refs[6].append([EOS])                         # a reference that is empty without its EOS
    return refs


def _pack(gram):
    return sum(int(t) << (16 * j) for j, t in enumerate(gram))


@pytest.mark.parametrize("with_eos", [False, True])
def test_bank_tables_against_a_brute_force_count(with_eos):
    from care_amd import CiderBank, MetricBank, _lib

    refs = _refs(np.random.RandomState(5))
    bank = MetricBank(refs, 65536, with_eos=with_eos, device=None)
    assert isinstance(bank.cider, CiderBank) and bank.cider.with_eos == with_eos and bank.desc is None and bank.dev is None
    assert bank.n_videos == 7 and bank.n_refs == sum(len(v) for v in refs) == bank.cider.n_refs
    h = bank.host
    assert h["clip_keys"].dtype == np.uint64 and h["clip_max"].dtype == np.int32 and h["ref_tok"].dtype == np.int32
    assert h["clip_start"].dtype == np.int64 and h["ref_tok_start"].dtype == np.int64
    assert len(h["clip_start"]) == 8 and len(h["ref_tok_start"]) == bank.n_refs + 1
    i = 0
    for v, video in enumerate(refs):
        most = Counter()
        for ref in video:
            toks = C.caption(ref, None, with_eos)
            assert h["ref_tok"][h["ref_tok_start"][i]: h["ref_tok_start"][i + 1]].tolist() == toks
            assert bank.cider.host["ref_len"][i] == len(toks)
            i += 1
            for n in range(1, 5):
                for g, c in C.ngrams(toks, n).items():
                    most[g] = max(most[g], c)
        want = sorted((_pack(g), c) for g, c in most.items())
        lo, hi = h["clip_start"][v], h["clip_start"][v + 1]
        assert h["clip_keys"][lo:hi].tolist() == [k for k, _ in want] and h["clip_max"][lo:hi].tolist() == [c for _, c in want]
    assert i == bank.n_refs and h["clip_start"][5] == h["clip_start"][6], "a video without references owns no keys"
    assert max(h["clip_max"]) >= 2, "some n-gram must repeat inside a reference"
    # the struct the kernel takes: ctypes mirror against the C compiler's layout of the header
    D = _lib.MetricBankDesc
    sizes = c_layout(["sizeof(care_metric_bank)", "offsetof(care_metric_bank, cider)", "offsetof(care_metric_bank, clip_keys)",
                      "offsetof(care_metric_bank, clip_max)", "offsetof(care_metric_bank, clip_start)",
                      "offsetof(care_metric_bank, ref_tok)", "offsetof(care_metric_bank, ref_tok_start)", "sizeof(care_cider_bank)"])
    assert sizes == [ctypes.sizeof(D), D.cider.offset, D.clip_keys.offset, D.clip_max.offset, D.clip_start.offset, D.ref_tok.offset,
                     D.ref_tok_start.offset, ctypes.sizeof(_lib.CiderBankDesc)]


def test_from_words_gives_unknown_words_ids_of_their_own():
    from care_amd import MetricBank

    w2i = {"<pad>": 0, "<unk>": 1, "<bos>": 2, "<eos>": 3, "a": 6, "man": 7, "is": 8}
    words = [[["a", "man", "is", "cooking"], ["a", "chef", "is", "cooking"]], [["a", "man", "is", "singing"]]]
    bank = MetricBank.from_words(words, w2i, vocab_size=20, device=None)
    assert bank.extra_words == {"cooking": 20, "chef": 21, "singing": 22} and bank.vocab_size == 23
    assert bank.host["ref_tok"].tolist() == [6, 7, 8, 20, 6, 21, 8, 20, 6, 7, 8, 22]
    assert MetricBank.from_words(words, w2i, device=None).extra_words["cooking"] == 9, "default: above the largest id"
    # over ids alone the three unknown words would all be <unk> and match each other; here they do not
    ids = MetricBank([[[6, 7, 8, 1], [6, 1, 8, 1]], [[6, 7, 8, 1]]], 20, device=None)
    assert ids.host["clip_keys"].size < bank.host["clip_keys"].size
    many = [[["w%d" % i for i in range(100)]] for _ in range(2)]
    assert MetricBank.from_words(many, {}, vocab_size=65436, device=None).vocab_size == 65536
    with pytest.raises(ValueError, match="65536"):
        MetricBank.from_words(many, {}, vocab_size=65437, device=None)


def test_scores_of_summed_components_are_the_reference_corpus_scores():
    from care_amd import MetricBank
    from care_amd.capmetrics import corpus_scores

    rng = np.random.RandomState(9)
    refs = [[rng.randint(6, 14, size=rng.randint(2, 12)).tolist() + [EOS] for _ in range(1 + v % 3)] for v in range(9)]
    corpus = M.Corpus(refs)
    bank = MetricBank(refs, 100, device=None)
    for short in (False, True):   # with and without a brevity penalty
        rows = []
        for r in range(40):
            n = int(rng.randint(1, 4)) if short else int(rng.randint(12, 17))   # shorter / longer than every reference
            toks = rng.randint(6, 14, size=n).tolist() if r % 3 else list(refs[r % 9][0][:n])
            rows.append((toks, len(toks), r % 9))
        rows.append(([6, 7], 0, 0))   # an invalid row
        records = corpus.records(*zip(*rows))
        ints, rouge, cider = M.Corpus.totals(records)
        assert ints[0] == 40 and ints[1] == 1 and (ints[2] < ints[3]) == short
        totals = bank.new_totals()
        assert totals.device.type == "cpu" and totals.dtype == torch.int64 and totals.tolist() == [0] * 14
        totals[:12] = torch.tensor(ints)
        totals[12:] = torch.tensor([rouge, cider], dtype=torch.float64).view(torch.int64)
        for flags in ((1, 0, 1, 1), (0, 0, 0, 1), (1, 0, 0, 0)):
            got, want = bank.scores(totals, flags), corpus.corpus(records, flags)
            assert set(got) == set(want) == set(M.KEYS) | {"Sum", "n_captions", "n_invalid"}
            for k in want:
                assert isinstance(got[k], float) and abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
        assert got["Bleu_1"] > 0.01 and got["ROUGE_L"] > 0.1 and got["n_captions"] == 40.0 and got["n_invalid"] == 1.0
    empty = corpus_scores([0] * 12, 0.0, 0.0)
    assert empty["ROUGE_L"] == 0.0 and empty["CIDEr"] == 0.0 and empty["n_captions"] == 0.0


def test_refusals_by_name():
    from care_amd import MetricBank, ValidationEpoch

    two = [[[10, 11]], [[10, 12]]]
    with pytest.raises(ValueError, match="vocab_size"):
        MetricBank(two, 65537, device=None)
    with pytest.raises(ValueError, match="outside"):
        MetricBank([[[10, 0, 11]]], 100, device=None)
    with pytest.raises(ValueError, match="empty"):
        MetricBank([], 100, device=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MetricBank(two, 100, device="cpu")
    with pytest.raises(ValueError, match="video_ids"):
        MetricBank(two, 100, device=None, video_ids=["a"])
    host = MetricBank(two, 100, device=None, video_ids=["a", "b"])
    assert host.rows(["b", "a"]).tolist() == [1, 0]
    with pytest.raises(KeyError, match="not in the bank"):
        host.rows(["c"])
    z = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device=None"):
        host.score(torch.zeros(1, 4, dtype=torch.int32), z, z)
    with pytest.raises(RuntimeError, match="device=None"):
        host.accumulate({"stats": torch.zeros(1, 12, dtype=torch.int32), "rouge": torch.zeros(1, dtype=torch.float64)}, host.new_totals())
    with pytest.raises(NotImplementedError, match="METEOR"):
        host.scores(host.new_totals(), (1, 1, 1, 1))
    with pytest.raises(ValueError, match="4 flags"):
        host.scores(host.new_totals(), (1, 0, 1))
    # the epoch
    with pytest.raises(NotImplementedError, match="ensemble"):
        ValidationEpoch({}, [object(), object()], host)
    with pytest.raises(TypeError, match="MetricBank"):
        ValidationEpoch({}, object(), host.cider)
    with pytest.raises(TypeError, match="training mode"):
        ValidationEpoch({}, torch.nn.Linear(2, 2), host)


def test_the_epoch_refuses_meteor_and_wide_beams_before_it_decodes():
    from care_amd import MetricBank, ValidationEpoch, get_framework
    from conftest import GoldenCase

    opt = GoldenCase("msrvtt_base_ami_b2").build()[0]
    model = get_framework(opt)
    host = MetricBank([[[10, 11]], [[10, 12]]], opt["vocab_size"], device=None)
    with pytest.raises(NotImplementedError, match="METEOR"):
        ValidationEpoch(opt, model, host, metric_sum=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="beam_size 9"):
        ValidationEpoch(opt, model, host, beam_size=9)
    epoch = ValidationEpoch(opt, model, host, beam_size=3, beam_alpha=0.5)
    assert epoch.beam_size == 3 and epoch.beam_alpha == 0.5 and epoch.translator._len_pow[4] == 2.0
    assert ValidationEpoch(opt, model, host).beam_size == opt.get("beam_size", 5)
    with pytest.raises(RuntimeError, match="device=None"):
        epoch.run([])


def test_the_epoch_retries_once_without_the_resident_decodes_then_raises():
    """`run` on states that a stand-in for `accumulate` hands back (no GPU, nothing decoded): rows without a caption send the
    epoch once more through the multi-launch decodes; still without, the Translator's error; rows invalid for another reason
    are named as such."""
    from care_amd import MetricBank, ValidationEpoch, _lib, get_framework
    from conftest import GoldenCase

    opt = GoldenCase("msrvtt_base_ami_b2").build()[0]
    host = MetricBank([[[10, 11]], [[10, 12]]], opt["vocab_size"], device=None)
    epoch = ValidationEpoch(opt, get_framework(opt), host)

    def state(n_valid, n_invalid, gave_up):
        s = torch.zeros(15, dtype=torch.int64)
        s[0], s[1], s[14] = n_valid, n_invalid, gave_up
        s[2:12] = torch.tensor([6, 6, 6, 5, 4, 3, 6, 5, 4, 3]) * n_valid
        s[12:14] = torch.tensor([1.0 * n_valid, 5.0 * n_valid], dtype=torch.float64).view(torch.int64)
        return s

    def play(states):
        calls = []

        def accumulate(batches, resident=True):
            calls.append(resident)
            return states[len(calls) - 1]
        epoch.accumulate = accumulate
        return calls

    calls = play([state(3, 0, 0)])
    got = epoch.run([{}])
    assert calls == [True] and got["n_captions"] == 3.0 and got["ROUGE_L"] == 1.0 and got["CIDEr"] == 5.0
    assert abs(got["Bleu_4"] - 1.0) < 1e-9 and abs(got["Sum"] - (got["Bleu_4"] + 6.0)) < 1e-12 and epoch.last == got
    calls = play([state(2, 1, 1), state(3, 0, 0)])
    assert epoch.run(iter([{}]))["n_captions"] == 3.0 and calls == [True, False], "once more, the resident decodes switched off"
    calls = play([state(2, 1, 1), state(2, 1, 1)])
    with pytest.raises(_lib.CareHipError, match="resident decode timed out"):
        epoch.run([{}])
    assert calls == [True, False]
    calls = play([state(2, 1, 0)])
    with pytest.raises(ValueError, match="no references"):
        epoch.run([{}])
    assert calls == [True]


# ------------------------------------------------------------------------------------------------ header, binding, libraries
def test_header_binding_and_libraries_agree_on_the_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "capmetrics.hip" in build.SOURCES
    build.build_all()
    for name in ENTRY_POINTS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "void* stream"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), name
        for ctype, decl in zip(sig, params):
            want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else \
                ctypes.c_double if decl.startswith("double") else ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            assert hasattr(ctypes.CDLL(build.lib_path(variant)), name), (variant, name)
    assert set(ENTRY_POINTS) <= set(_lib.exported_symbols())
    import care_amd
    assert {"MetricBank", "ValidationEpoch"} <= set(care_amd.__all__)


def _desc(P):
    from care_amd import _lib

    desc = _lib.MetricBankDesc()
    for k in ("corpus_keys", "corpus_lndf", "ref_keys", "ref_w", "ref_start", "ref_norm", "ref_len", "vid_start"):
        setattr(desc.cider, k, P)
    desc.cider.n_corpus, desc.cider.n_videos, desc.cider.n_refs, desc.cider.ln_n = 3, 2, 2, math.log(2)
    for k in ("clip_keys", "clip_max", "clip_start", "ref_tok", "ref_tok_start"):
        setattr(desc, k, P)
    return desc


def test_refusals_come_before_any_launch():
    """The argument checks of the three entry points with pointers that are never dereferenced (no GPU here: a launch would fail)."""
    from care_amd import _lib

    lib = _lib.load()
    P = 0x10000   # an aligned non-NULL address
    desc = _desc(P)
    bank = ctypes.addressof(desc)

    def stats(tokens=P, ld=30, col0=1, width=29, length=P, video=P, rows=4, bank_=bank, rec=P, rouge=P):
        return lib.care_caption_stats(tokens, ld, col0, width, length, video, rows, 0, 3, bank_, rec, rouge, None)

    assert stats(rows=0) == 0, "rows == 0 is a no-op"
    assert stats(tokens=None) == EINVAL and stats(length=None) == EINVAL and stats(video=None) == EINVAL
    assert stats(rec=None) == EINVAL and stats(rouge=None) == EINVAL and stats(bank_=None) == EINVAL and stats(rows=-1) == EINVAL
    assert stats(ld=29) == EINVAL, "ld below col0 + width"
    assert stats(width=65, ld=70) == EINVAL and stats(width=0) == EINVAL and stats(col0=-1) == EINVAL
    assert stats(width=64, ld=65, rows=0) == 0
    assert stats(rouge=P + 4) == EALIGN
    for k in ("clip_keys", "clip_max", "clip_start", "ref_tok", "ref_tok_start"):
        setattr(desc, k, None)
        assert stats() == EINVAL, k
        setattr(desc, k, P)
    desc.cider.vid_start = None
    assert stats() == EINVAL
    desc.cider.vid_start = P
    for k in ("clip_keys", "clip_start", "ref_tok_start"):
        setattr(desc, k, P + 4)
        assert stats() == EALIGN, k
        setattr(desc, k, P)
    desc.cider.n_videos = 0
    assert stats() == EINVAL
    desc.cider.n_videos = 2

    def totals(rec=P, rouge=P, cider=P, rows=4, ti=P, td=P):
        return lib.care_caption_totals(rec, rouge, cider, rows, ti, td, None)

    assert totals(rows=0) == 0 and totals(rows=0, cider=None) == 0
    assert totals(rec=None) == EINVAL and totals(rouge=None) == EINVAL and totals(ti=None) == EINVAL and totals(td=None) == EINVAL
    assert totals(rows=-1) == EINVAL
    assert totals(rouge=P + 4) == EALIGN and totals(ti=P + 4) == EALIGN and totals(td=P + 4) == EALIGN

    def winner(nfin=P, fscore=P, flen=P, fhyp=P, B=4, cap=10, w=30, pw=P, n_pow=32, tokens=P, length=P):
        return lib.care_beam_winner(nfin, fscore, flen, fhyp, B, cap, w, pw, n_pow, tokens, length, None)

    assert winner(B=0) == 0
    for k in ("nfin", "fscore", "flen", "fhyp", "pw", "tokens", "length"):
        assert winner(**{k: None}) == EINVAL, k
    assert winner(B=-1) == EINVAL and winner(cap=0) == EINVAL and winner(cap=65) == EINVAL and winner(w=0) == EINVAL
    assert winner(n_pow=0) == EINVAL and winner(pw=P + 4) == EALIGN
    assert winner(cap=64, B=0) == 0

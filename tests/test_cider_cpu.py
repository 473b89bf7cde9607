"""CPU: the CIDEr-D reward without a GPU - the float64 yardstick (tests/cider_reference.py) on hand-worked anchors, the host
tables of care_amd.reward.CiderBank against a brute-force count, the refusals that come before any launch, and the agreement of
include/care_hip.h, care_amd/_lib.py and both libraries on the entry points of csrc/reward.hip."""
import ctypes
import math
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

import cider_reference as C
from c_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("care_cider_score", "care_reward_advantage", "care_reward_loss_fwd", "care_reward_loss_bwd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
TWO = [[[10, 11]], [[10, 12]]]


def test_hand_worked_anchors():
    corpus = C.Corpus(TWO)
    assert corpus.score([10, 11], 2, 0) == 5.0
    assert corpus.score([10, 12], 2, 0) == 0.0
    want = 10 * math.exp(-1 / 72) * (0.5 + 1 / math.sqrt(2)) / 4
    assert abs(want - 2.9761432456900) < 1e-12
    assert abs(corpus.score([10, 11, 11], 3, 0) - want) < 1e-14
    assert corpus.score([], 0, 0) == 0.0 and corpus.score([10, 11], 0, 0) == 0.0
    assert corpus.score([10, 11, 99, 99], 2, 0) == 5.0, "`length` cuts the caption"
    assert corpus.score([10, 11], 2, 2) == 0.0 and corpus.score([10, 11], 2, -1) == 0.0, "a video outside the corpus"


def test_a_corpus_of_one_video_scores_zero_everywhere():
    corpus = C.Corpus([[[10, 11, 12], [10, 13]]])
    for cand in ([10, 11, 12], [10, 13], [10], [7, 8, 9, 10, 11], []):
        assert corpus.score(cand, len(cand), 0) == 0.0


def test_with_eos_changes_lengths_and_ngrams_as_defined():
    eos = C.EOS
    assert C.caption([10, 11, eos], 3) == [10, 11] and C.caption([10, 11, eos], 3, with_eos=True) == [10, 11, eos]
    assert C.caption([10, eos, 11], 3) == [10, eos, 11], "only a TRAILING EOS is dropped"
    assert C.caption([10, 11, eos, 5], 3) == [10, 11] and C.caption([eos], 1) == []
    refs = [[[10, 11, eos]], [[10, 12, eos]]]
    off, on = C.Corpus(refs), C.Corpus(refs, with_eos=True)
    assert off.score([10, 11, eos], 3, 0) == 5.0, "without EOS this is the two-video anchor"
    assert off.score([10, 11], 2, 0) == 5.0
    # with EOS the unigram EOS and the bigrams (11, EOS) / (12, EOS) exist; EOS is in both videos, so its weight is 0
    assert (eos,) in on.df and on.df[(eos,)] == 2 and (11, eos) in on.df and (eos,) not in off.df
    full = on.score([10, 11, eos], 3, 0)
    assert abs(full - 7.5) < 1e-12, "orders 1..3 match fully (the 4-gram does not exist)"
    short = on.score([10, 11], 2, 0)   # no EOS: shorter by one token, and the (11, EOS) bigram and the trigram are missing
    uni = 1.0                                          # 11 is the only weighted unigram on both sides
    bi = (math.log(2) ** 2) / (math.log(2) * math.sqrt(2) * math.log(2))
    assert abs(short - 10 * math.exp(-1 / 72) * (uni + bi) / 4) < 1e-12


def _brute_force(refs, with_eos):
    """Per reference {tuple n-gram: tf}; df per n-gram, once per video."""
    per_ref, df = [], Counter()
    for video in refs:
        seen = set()
        for ref in video:
            toks = C.caption(ref, None, with_eos)
            grams = Counter()
            for n in range(1, 5):
                for i in range(len(toks) - n + 1):
                    grams[tuple(toks[i:i + n])] += 1
            per_ref.append((toks, grams))
            seen |= set(grams)
        for g in seen:
            df[g] += 1
    return per_ref, df


def _pack(gram):
    return sum(int(t) << (16 * j) for j, t in enumerate(gram))


@pytest.mark.parametrize("with_eos", [False, True])
def test_bank_tables_against_a_brute_force_count(with_eos):
    from care_amd.reward import CiderBank, key_order, pack_ngrams

    rng = np.random.RandomState(5)
    V = 65536
    refs = []
    for v in range(7):
        video = []
        for _ in range(1 + v % 4):
            n = int(rng.randint(1, 12))
            toks = rng.randint(6, 40, size=n).tolist()
            if rng.rand() < 0.3:
                toks[rng.randint(n)] = 65535      # the largest id: the top bit of a key when it is an n-gram's 4th token
            video.append(toks + [C.EOS])
        refs.append(video)
    refs[3].append(list(refs[3][0]))              # a repeated reference: df still counts the video once
    refs[5] = []                                  # a video without references
    bank = CiderBank(refs, V, with_eos=with_eos, device=None)
    h = bank.host
    per_ref, df = _brute_force(refs, with_eos)
    # the packing: token j in bits [16 j, 16 j + 16), in caption order
    assert pack_ngrams([5, 65535, 7, 9], 4).tolist() == [5 | 65535 << 16 | 7 << 32 | 9 << 48]
    assert pack_ngrams([5, 6, 7], 2).tolist() == [5 | 6 << 16, 6 | 7 << 16] and pack_ngrams([5], 2).size == 0
    assert key_order(np.array([5, 5 | 6 << 16, 5 | 6 << 16 | 7 << 32, 1 << 48 | 1], dtype=np.uint64)).tolist() == [1, 2, 3, 4]
    # the corpus: sorted unique keys (as uint64) with ln max(1, df), df once per video
    want = sorted((_pack(g), c) for g, c in df.items())
    assert h["corpus_keys"].dtype == np.uint64 and h["corpus_keys"].tolist() == [k for k, _ in want]
    assert h["df"].tolist() == [c for _, c in want] and max(h["df"]) <= 6
    assert np.array_equal(h["corpus_lndf"], np.log(np.maximum(1, h["df"]).astype(np.float64)))
    assert bank.ln_n == math.log(7) and bank.n_videos == 7
    # per video its range of references, per reference its sorted unique keys, weights, norms and length
    assert h["vid_start"].tolist() == np.cumsum([0] + [len(v) for v in refs]).tolist()
    assert len(per_ref) == bank.n_refs == len(h["ref_len"])
    for i, (toks, grams) in enumerate(per_ref):
        lo, hi = h["ref_start"][i], h["ref_start"][i + 1]
        keys = h["ref_keys"][lo:hi].tolist()
        assert keys == sorted(_pack(g) for g in grams) and len(set(keys)) == len(keys)
        w = {_pack(g): tf * (math.log(7) - math.log(max(1, df[g]))) for g, tf in grams.items()}
        assert np.allclose(h["ref_w"][lo:hi], [w[k] for k in keys], rtol=1e-15, atol=0)
        for n in range(1, 5):
            norm = math.sqrt(sum(w[_pack(g)] ** 2 for g in grams if len(g) == n))
            assert abs(h["ref_norm"][i, n - 1] - norm) <= 1e-14 * max(1.0, norm)
        assert h["ref_len"][i] == len(toks)
    # the struct the kernel takes: ctypes mirror against the C compiler's layout of the header
    from care_amd import _lib
    sizes = c_layout(["sizeof(care_cider_bank)", "offsetof(care_cider_bank, n_corpus)", "offsetof(care_cider_bank, vid_start)",
                      "offsetof(care_cider_bank, n_videos)", "offsetof(care_cider_bank, n_refs)", "offsetof(care_cider_bank, ln_n)"])
    D = _lib.CiderBankDesc
    assert sizes == [ctypes.sizeof(D), D.n_corpus.offset, D.vid_start.offset, D.n_videos.offset, D.n_refs.offset, D.ln_n.offset]


def test_bank_and_step_refusals_by_name():
    from care_amd import CiderBank, SelfCriticalStep, self_critical_loss
    from care_amd.criterion import DeferredLogits
    from care_amd.reward import reward_advantage

    with pytest.raises(ValueError, match="vocab_size"):
        CiderBank(TWO, 65537, device=None)
    with pytest.raises(ValueError, match="vocab_size"):
        CiderBank(TWO, 0, device=None)
    with pytest.raises(ValueError, match="outside"):
        CiderBank([[[10, 0, 11]]], 100, device=None)          # PAD inside a caption
    with pytest.raises(ValueError, match="outside"):
        CiderBank([[[10, 100]]], 100, device=None)
    with pytest.raises(ValueError, match="empty"):
        CiderBank([], 100, device=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CiderBank(TWO, 100, device="cpu")
    with pytest.raises(ValueError, match="video_ids"):
        CiderBank(TWO, 100, device=None, video_ids=["a"])
    host = CiderBank(TWO, 100, device=None, video_ids=["a", "b"])
    assert host.rows(["b", "a", "b"]).tolist() == [1, 0, 1]
    with pytest.raises(KeyError, match="not in the bank"):
        host.rows(["c"])
    with pytest.raises(RuntimeError, match="device=None"):
        host.score(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    # the loss: everything is checked before anything runs
    logits, labels, adv = torch.zeros(2, 3, 7), torch.ones(2, 3, dtype=torch.long), torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        self_critical_loss(logits, labels, adv)
    with pytest.raises(NotImplementedError, match="DeferredLogits"):
        self_critical_loss(DeferredLogits(torch.zeros(2, 3, 4), torch.zeros(7, 4)), labels, adv)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reward_advantage(torch.zeros(2, 3))
    # the step
    with pytest.raises(NotImplementedError, match="ensemble"):
        SelfCriticalStep({}, [object(), object()], host)
    with pytest.raises(TypeError, match="CiderBank"):
        SelfCriticalStep({}, object(), object())
    with pytest.raises(ValueError, match="n_samples"):
        SelfCriticalStep({}, object(), host, n_samples=0)
    with pytest.raises(ValueError, match="n_samples"):
        SelfCriticalStep({}, object(), host, n_samples=1, baseline="mean")
    with pytest.raises(ValueError, match="baseline"):
        SelfCriticalStep({}, object(), host, baseline="median")
    with pytest.raises(ValueError, match="with_eos"):
        SelfCriticalStep({}, object(), host, with_eos=True)

    class Fused(object):
        fused_head = True

    with pytest.raises(NotImplementedError, match="fused head"):
        SelfCriticalStep({}, Fused(), host)


def test_header_binding_and_libraries_agree_on_the_reward_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "reward.hip" in build.SOURCES
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
    for variant in build.VARIANTS:
        assert _lib.load(variant=variant).care_version() == int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1))
        assert _lib.source_hash(variant) == build.source_hash(variant)


def test_refusals_come_before_any_launch():
    """The argument checks of the four entry points with pointers that are never dereferenced (no GPU here: a launch would fail)."""
    from care_amd import _lib

    lib = _lib.load()
    P = 0x10000   # an aligned non-NULL address
    desc = _lib.CiderBankDesc()
    for k in ("corpus_keys", "corpus_lndf", "ref_keys", "ref_w", "ref_start", "ref_norm", "ref_len", "vid_start"):
        setattr(desc, k, P)
    desc.n_corpus, desc.n_videos, desc.n_refs, desc.ln_n = 3, 2, 2, math.log(2)
    bank = ctypes.addressof(desc)

    def score(tokens=P, ld=30, col0=1, width=29, length=P, video=P, rows=4, bank_=bank, out=P):
        return lib.care_cider_score(tokens, ld, col0, width, length, video, rows, 0, 3, bank_, out, None, None)

    assert score(rows=0) == 0, "rows == 0 is a no-op"
    assert score(tokens=None) == EINVAL and score(length=None) == EINVAL and score(video=None) == EINVAL
    assert score(out=None) == EINVAL and score(bank_=None) == EINVAL and score(rows=-1) == EINVAL
    assert score(ld=29) == EINVAL, "ld below col0 + width"
    assert score(width=65, ld=70) == EINVAL and score(width=0) == EINVAL and score(col0=-1) == EINVAL
    assert score(width=64, ld=65, rows=0) == 0
    for k in ("corpus_keys", "ref_w", "vid_start"):
        setattr(desc, k, None)
        assert score() == EINVAL, k
        setattr(desc, k, P)
    for k in ("corpus_keys", "corpus_lndf", "ref_keys", "ref_w", "ref_start", "ref_norm"):
        setattr(desc, k, P + 4)
        assert score() == EALIGN, k
        setattr(desc, k, P)
    desc.n_videos = 0
    assert score() == EINVAL
    desc.n_videos = 2

    adv = lib.care_reward_advantage
    assert adv(P, None, 3, 1, P, P, None) == EINVAL, "the leave-one-out baseline needs n >= 2"
    assert adv(None, P, 3, 2, P, P, None) == EINVAL and adv(P, P, 3, 2, None, P, None) == EINVAL
    assert adv(P, P, 3, 2, P, None, None) == EINVAL and adv(P, P, 0, 2, P, P, None) == EINVAL and adv(P, P, 3, 0, P, P, None) == EINVAL
    assert adv(P, P, 3, 2, P, P + 4, None) == EALIGN

    V = 10547

    def fwd(logits=P, ld=V, ss=29 * V, rps=29, v=V, labels=P, a=P, totals=P, loss=P, acc=None, rows=58):
        return lib.care_reward_loss_fwd(logits, ld, ss, rps, v, labels, a, P, P, P, totals, loss, None, acc, rows, None)

    assert fwd(logits=None) == EINVAL and fwd(labels=None) == EINVAL and fwd(a=None) == EINVAL and fwd(totals=None) == EINVAL
    assert fwd(loss=None) == EINVAL and fwd(rows=0) == EINVAL and fwd(v=0) == EINVAL
    assert fwd(ld=V - 1) == ESHAPE and fwd(ss=28 * V) == ESHAPE and fwd(rows=57) == ESHAPE
    assert fwd(logits=P + 2) == EALIGN and fwd(totals=P + 4) == EALIGN and fwd(acc=P + 4) == EALIGN

    def bwd(logits=P, ld=V, ss=29 * V, rps=29, labels=P, a=P, totals=P, g=P, d=P, ldd=V, dss=29 * V, seq_rows=29, rows=58):
        return lib.care_reward_loss_bwd(logits, ld, ss, rps, V, labels, a, P, P, totals, g, d, ldd, dss, seq_rows, rows, None)

    assert bwd(logits=None) == EINVAL and bwd(a=None) == EINVAL and bwd(totals=None) == EINVAL and bwd(g=None) == EINVAL
    assert bwd(d=None) == EINVAL and bwd(rows=0) == EINVAL
    assert bwd(ldd=V - 1) == ESHAPE and bwd(seq_rows=28) == ESHAPE and bwd(dss=28 * V) == ESHAPE and bwd(rows=57) == ESHAPE
    assert bwd(d=P + 2) == EALIGN and bwd(totals=P + 4) == EALIGN

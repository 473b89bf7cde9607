"""GPU: the kernels of the caption analysis (csrc/corpus_stats.hip) in both libraries.

care_corpus_insert / care_corpus_totals against tests/corpus_reference.py (dicts and sets): every total is an integer and must
EQUAL the reference's - for each fixture of tests/golden/corpus as one batch, as batches of 1 and as batches of 7 (duplicates
inside one launch and across launches), and the four floats must be the genuine reference's by `==`; a table of 8 slots whose
probe chains wrap around, held slot by slot against linear probing on the host; key_mask 0x7 on the 200-caption case (8 keys
for 147 distinct captions and 438 distinct training captions: every probe and every lookup is decided by the token-wise compare);
captions of 0, 1, 63 and 64 tokens; a strided view with an offset; the bitmap's word edges; keys_out against the host's key
function.  care_caption_model_score against the Translator's own host division, bit for bit.

Measured on one MI355X: every integer, key and score equal to the host's; the 22 tests of this file: 2.6 s."""
import ctypes
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

import corpus_reference as R
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["", "f16"]
INTS = ("n_captions", "length_sum", "n_distinct", "n_novel", "n_empty", "usage")
GAP = 8


@functools.lru_cache(maxsize=None)
def _fixtures():
    return {c["name"]: c for c in (json.load(open(p)) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*.json"))))}


@functools.lru_cache(maxsize=None)
def _want(name):
    case = _fixtures()[name]
    return R.totals(case["train"], [R.cut(r) for r in case["rows"]])


def _insert_all(epoch, rows, batch, lengths=None):
    """The token rows through EpochCaptions.insert in batches of `batch` (0: all at once); returns the keys the kernel wrote."""
    from care_amd.corpusstats import caption_keys

    tokens = torch.tensor(rows, dtype=torch.int32, device=DEV)
    length = torch.tensor([len(r) for r in rows] if lengths is None else lengths, dtype=torch.int32, device=DEV)
    n = len(rows)
    whole = torch.full((n + 2 * GAP,), -77, dtype=torch.int64, device=DEV)
    step = batch or n
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        assert epoch.insert(tokens[lo:hi], length[lo:hi], keys_out=whole[GAP + lo: GAP + hi]) == lo
    keys = whole.cpu().numpy()
    assert (keys[:GAP] == -77).all() and (keys[GAP + n:] == -77).all(), "keys_out was written outside its rows"
    caps = [R.cut(r, None if lengths is None else lengths[i]) for i, r in enumerate(rows)]
    assert np.array_equal(keys[GAP: GAP + n].view(np.uint64), caption_keys(caps, epoch.bank.key_mask)), "keys_out is the host's key function"
    return caps


@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["toy", "all_distinct_novel", "all_identical", "prefixes", "eos_pad", "random200"])
def test_every_fixture_in_one_batch_in_batches_of_1_and_of_7(name, variant):
    from care_amd import CorpusBank, EpochCaptions

    case, want = _fixtures()[name], _want(name)
    bank = CorpusBank(case["train"], len(case["vocab"]), device=DEV)
    epoch = EpochCaptions(256, bank.vocab_size, bank, variant=variant)
    for batch in (0, 1, 7):
        epoch.reset()
        _insert_all(epoch, case["rows"], batch)
        got = epoch.totals()
        assert {k: got[k] for k in INTS} == want and got["n_overflow"] == 0, (name, batch, got, want)
        assert (got["ave_length"], got["novel"], got["unique"], got["usage"]) == tuple(case["expected"]), (name, batch)   # floats by ==
        store = epoch.tokens[:len(case["rows"])].cpu().tolist()
        lens = epoch.length[:len(case["rows"])].cpu().tolist()
        assert [tuple(s[:n]) for s, n in zip(store, lens)] == [R.cut(r) for r in case["rows"]] and all(not any(s[n:]) for s, n in zip(store, lens))


@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
def test_eight_slots_probe_chains_and_wrap_around(variant):
    """5 distinct captions, 3 of them repeated, in a table of 8 slots; the captions are chosen so that every key starts at slot
    6 or 7: the chains run over the table's end.  In batches of 1 the table's contents are those of linear probing on the host."""
    from care_amd import CorpusBank, EpochCaptions
    from care_amd.corpusstats import caption_key

    distinct = []
    for t in range(6, 400):
        for cap in ((t,), (t, t + 1)):
            if caption_key(cap) & 7 >= 6 and len(distinct) < 5:
                distinct.append(cap)
    assert len(distinct) == 5
    order = [0, 1, 0, 2, 3, 1, 4, 0]
    rows = [list(distinct[i]) + [3] * (3 - len(distinct[i])) for i in order]
    train = [list(distinct[1]), list(distinct[4]), [6, 6, 6]]
    bank = CorpusBank(train, 512, device=DEV)
    epoch = EpochCaptions(8, 512, bank, variant=variant)
    want = R.totals(train, [R.cut(r) for r in rows])
    assert want["n_distinct"] == 5 and want["n_novel"] == 3 and want["n_captions"] == 8

    slots = [-1] * 8   # linear probing, one caption after the other
    for g, i in enumerate(order):
        s = caption_key(distinct[i]) & 7
        while slots[s] != -1 and order[slots[s]] != i:
            s = (s + 1) & 7
        if slots[s] == -1:
            slots[s] = g
    assert slots[7] != -1 and slots[0] != -1, "the chains wrap around"

    for batch in (1, 0, 7):
        epoch.reset()
        _insert_all(epoch, rows, batch)
        got = epoch.totals()
        assert {k: got[k] for k in INTS} == want, (batch, got, want)
        table = epoch.slots.cpu().tolist()
        if batch == 1:
            assert table == slots
        assert [s != -1 for s in table] == [s != -1 for s in slots], "which slots are taken does not depend on who wins one"
        assert sorted(order[g] for g in table if g != -1) == [0, 1, 2, 3, 4], "one slot per distinct caption"
    with pytest.raises(ValueError, match="larger than its capacity"):
        epoch.insert(torch.zeros(1, 3, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
def test_key_mask_7_every_probe_and_lookup_is_decided_by_the_tokens(variant):
    from care_amd import CorpusBank, EpochCaptions

    case, want = _fixtures()["random200"], _want("random200")
    bank = CorpusBank(case["train"], len(case["vocab"]), device=DEV, key_mask=0x7)
    assert len(set(bank.host["keys"].tolist())) <= 8 < bank.n
    epoch = EpochCaptions(256, bank.vocab_size, bank, variant=variant)
    from care_amd.corpusstats import caption_key
    probing = [False] * 256   # linear probing on the host: WHICH slots end up taken does not depend on the order
    for cap in sorted({R.cut(r) for r in case["rows"]}):
        s = caption_key(cap, 0x7)
        while probing[s]:
            s = (s + 1) & 255
        probing[s] = True
    assert sum(probing) == want["n_distinct"] > 100 and max(i for i, t in enumerate(probing) if t) < 8 + want["n_distinct"], "long chains"
    for batch in (0, 7):
        epoch.reset()
        _insert_all(epoch, case["rows"], batch)
        got = epoch.totals()
        assert {k: got[k] for k in INTS} == want, (batch, got, want)
        assert [g != -1 for g in epoch.slots.cpu().tolist()] == probing


@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
def test_lengths_0_1_63_64_an_offset_and_a_strided_view(variant):
    """Captions of 0, 1, 63 and 64 tokens without an EOS (the length ends them), pairs that differ in their last token only,
    and a row whose length reaches beyond the width; read through fed[:, 1:] with offset 1 (a row stride of 70)."""
    from care_amd import CorpusBank, EpochCaptions

    rng = np.random.RandomState(9)
    base = rng.randint(6, 500, size=64).tolist()
    other63, other64 = list(base), list(base)
    other63[62], other64[63] = 501, 501
    caps = [(base, 0), (base, 1), (base, 63), (base, 64), (other63, 63), (other64, 64), (base, 64), (base, 63), (base, 0), (base, 99),
            (base, -5), (other64, 63)]
    fed = torch.full((len(caps), 70), 777, dtype=torch.int32, device=DEV)
    for r, (toks, _) in enumerate(caps):
        fed[r, 2:66] = torch.tensor(toks, dtype=torch.int32)
    lengths = [n for _, n in caps]
    rows = [toks for toks, _ in caps]
    train = [base, base[:63], other64[:63] + [502], []]
    want = R.totals(train, [R.cut(t, min(n, 64)) for t, n in caps])
    assert want["n_empty"] == 3 and want["n_distinct"] == 6 and want["n_novel"] == 3
    bank = CorpusBank(train, 512, device=DEV)
    epoch = EpochCaptions(16, 512, bank, variant=variant)
    view = fed[:, 1:66]
    assert view.stride(0) == 70 and not view.is_contiguous()
    keys = torch.zeros(len(caps), dtype=torch.int64, device=DEV)
    epoch.insert(view, torch.tensor(lengths, dtype=torch.int32, device=DEV), offset=1, keys_out=keys)
    got = epoch.totals()
    assert {k: got[k] for k in INTS} == want, (got, want)
    from care_amd.corpusstats import caption_keys
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), caption_keys([R.cut(t, min(n, 64)) for t, n in zip(rows, lengths)]))
    assert epoch.length[:len(caps)].cpu().tolist() == [0, 1, 63, 64, 63, 64, 64, 63, 0, 64, 0, 63]
    with pytest.raises(ValueError, match="64"):
        epoch.insert(fed[:, 1:67], torch.tensor(lengths, dtype=torch.int32, device=DEV), offset=1)


@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
def test_bitmap_word_edges_in_a_vocabulary_of_65536(variant):
    """Tokens 0, 31, 32 and 65535 through the raw entry point with eos = 1 and pad = 2, so that 0 is an ordinary token."""
    from care_amd import CorpusBank, EpochCaptions, _lib

    bank = CorpusBank([[31, 32], [5]], 65536, device=DEV)
    epoch = EpochCaptions(8, 65536, bank, variant=variant)
    tokens = torch.tensor([[0, 31, 1], [32, 65535, 2], [31, 32, 1], [65535, 1, 0]], dtype=torch.int32, device=DEV)
    length = torch.full((4,), 3, dtype=torch.int32, device=DEV)
    _lib.call("care_corpus_insert", tokens.data_ptr(), 3, 0, 3, length.data_ptr(), 4, 0, 1, 2, ctypes.addressof(bank.desc),
              ctypes.addressof(epoch.desc), None, variant=variant)
    epoch.cursor = 4
    got = epoch.totals()
    assert (got["n_captions"], got["length_sum"], got["n_distinct"], got["n_novel"], got["n_empty"], got["usage"]) == (4, 7, 4, 3, 0, 4)
    words = epoch.bitmap.cpu().numpy().view(np.uint32)
    want = np.zeros(2048, dtype=np.uint32)
    want[0], want[1], want[2047] = (1 << 0) | (1 << 31), 1, 1 << 31
    assert np.array_equal(words, want)
    assert epoch.totals()["usage"] == 4, "care_corpus_totals writes: a second call gives the same"


# ------------------------------------------------------------------------------------------------ care_caption_model_score
@pytest.mark.parametrize("variant", VARIANTS, ids=["bf16", "fp16"])
def test_model_score_is_the_host_division_bit_for_bit(variant):
    from care_amd import _lib
    from care_amd.translator import Translator_ARFormer

    tr = Translator_ARFormer({"beam_size": 5, "beam_alpha": 0.7, "max_len": 30})
    pw = torch.from_numpy(tr._len_pow).to(DEV)
    rng = np.random.RandomState(4)

    def run(nfin, fscore, flen, cap):
        B = fscore.shape[0]
        whole = torch.full((B + 2 * GAP,), -7.25, dtype=torch.float64, device=DEV)
        d = [None if nfin is None else torch.from_numpy(nfin).to(DEV), torch.from_numpy(fscore).to(DEV), torch.from_numpy(flen).to(DEV)]
        _lib.call("care_caption_model_score", _lib.ptr(d[0]), d[1].data_ptr(), d[2].data_ptr(), B, cap, pw.data_ptr(), pw.numel(),
                  whole[GAP: GAP + B].data_ptr(), variant=variant)
        out = whole.cpu().numpy()
        assert (out[:GAP] == -7.25).all() and (out[GAP + B:] == -7.25).all()
        return out[GAP: GAP + B]

    # greedy: one hypothesis a clip
    B = 130
    score = (-rng.rand(B) * 30).astype(np.float32)
    length = rng.randint(1, 30, size=B).astype(np.int32)
    length[:3] = (29, 1, 31)   # (31: the table's last entry; longer lengths are clamped like the host's np.clip)
    got = run(None, score, length, 1)
    assert np.array_equal(got.view(np.int64), tr._norm(score, length).view(np.int64))

    # beam: the stable arg-sort's first, as _assemble_beam_gen takes it
    cap = 10
    nfin = rng.randint(1, cap + 3, size=B).astype(np.int32)
    fscore = (-rng.rand(B, cap) * 30).astype(np.float32)
    flen = rng.randint(1, 30, size=(B, cap)).astype(np.int32)
    # clip 0: two finished hypotheses with the SAME normalised score, the best of the clip; clip 1: one finished
    fscore[0, :] = -20.0
    flen[0, :] = 10
    fscore[0, 2], flen[0, 2], fscore[0, 6], flen[0, 6], nfin[0] = -3.0, 6, -3.0, 6, 8
    nfin[1] = 1
    norm = tr._norm(fscore, flen)
    n = np.minimum(nfin.astype(np.int64), cap)
    key = np.where(np.arange(cap)[None, :] < n[:, None], -norm, np.inf)
    first = np.argsort(key, axis=1, kind="stable")[:, 0]
    want = norm[np.arange(B), first]
    assert first[0] == 2 and norm[0, 2] == norm[0, 6]
    got = run(nfin, fscore, flen, cap)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    nfin[5] = 0
    assert run(nfin, fscore, flen, cap)[5] == 0.0, "a clip without a finished hypothesis"

"""GPU: the kernels of the validation metrics (csrc/capmetrics.hip) through the raw ABI.

care_caption_stats against tests/capmetrics_reference.py (plain Python): the twelve integers of a row must EQUAL the reference's,
its ROUGE-L must lie within 1e-12 - two integer-to-double quotients, three products, a sum and a quotient of values <= 2.44: a
few ulps of 1.1e-16, with three orders of margin.  care_caption_totals: the integer totals equal numpy's int64 sums, for one
batch and for two; the two double sums within 1e-12 relative (<= 1030 additions of non-negative doubles: n ulps at the worst,
2.3e-13).  care_beam_winner against numpy's stable arg-sort of the Translator's own normalised scores.  Every output lies in a
guarded buffer between canaries; invalid rows are inputs (a length of 0, a negative length, a video outside the bank).

Measured on one MI355X: ROUGE-L deviates by exactly 0 from the reference on all 6 x 130 rows (the same double operations in the
same order); this file and tests/test_gpu_validation.py together: 4.9 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import capmetrics_reference as M
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

GAP = 8
EINVAL, EALIGN = -1, -2
ROUGE_BAR = 1e-12
CIDER_BAR = 2e-6                 # tests/test_gpu_reward_kernels.py: BAR
W, COL0, LD = 64, 1, 70          # caption width, the column offset of fed[:, 1:], a padded row stride
EOS = M.EOS
UNSEEN = 3000                    # tokens from here on occur in no reference
CANARY = {torch.int32: -77, torch.int64: -77, torch.float64: -7.25, torch.float32: -7.25}


def _guarded(n, dtype):
    """(whole, view): n elements between GAP canaries on either side, on the device."""
    whole = torch.full((n + 2 * GAP,), CANARY[dtype], dtype=dtype, device=DEV)
    return whole, whole[GAP:GAP + n]


def _intact(whole, n):
    w, fill = whole.cpu(), CANARY[whole.dtype]
    return bool((w[:GAP] == fill).all()) and bool((w[GAP + n:] == fill).all())


# ------------------------------------------------------------------------------------------------ care_caption_stats
CORPORA = {"v2": (2, (1, 5)), "v3": (3, (20, 41, 1)), "v40": (40, (1, 5, 20, 41))}


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """refs of a corpus: captions of 1 .. 30 tokens over a small vocabulary (so that n-grams repeat within and between videos),
    most with a trailing EOS; one reference of 64 tokens and one of 100."""
    n_videos, counts = CORPORA[name]
    rng = np.random.RandomState(200 + n_videos)
    refs = []
    for v in range(n_videos):
        video = []
        for _ in range(counts[v % len(counts)]):
            n = int(rng.randint(1, 31))
            toks = rng.randint(6, 30, size=n).tolist()
            video.append(toks + [EOS] if rng.rand() < 0.8 else toks)
        refs.append(video)
    refs[0][0] = rng.randint(6, 30, size=W).tolist()
    refs[1][-1] = rng.randint(6, 30, size=100).tolist()
    return refs


KINDS = 15


@functools.lru_cache(maxsize=None)
def _candidates(name):
    """130 rows (tokens [130, W] int32, length, video) that cycle through the candidate kinds, over all videos of the corpus."""
    refs = _corpus(name)
    rng = np.random.RandomState(7)
    tokens = rng.randint(6, 30, size=(130, W)).astype(np.int32)       # what lies behind a caption's end is never read
    length, video = np.zeros(130, dtype=np.int32), np.zeros(130, dtype=np.int32)
    plain = (0, 1, 2, 3, 4, 5, 30, 64)
    for r in range(130):
        v = video[r] = (r // 2) % len(refs)
        kind = r % KINDS
        short = [x for x in refs[v] if len(x) <= W]
        ref = short[r % len(short)] if short else refs[v][0][:W]
        if kind < 8:                                   # random captions of the lengths at which an order appears
            length[r] = plain[kind]
        elif kind == 8:                                # one token repeated
            tokens[r, :9] = 11
            length[r] = 9
        elif kind == 9:                                # a copy of a reference
            tokens[r, :len(ref)] = ref
            length[r] = len(ref)
        elif kind == 10:                               # a reference with one token changed
            tokens[r, :len(ref)] = ref
            tokens[r, (len(ref) - 1) // 2] = 29 if ref[(len(ref) - 1) // 2] != 29 else 28
            length[r] = len(ref)
        elif kind == 11:                               # a reference reversed
            tokens[r, :len(ref)] = ref[::-1]
            length[r] = len(ref)
        elif kind == 12:                               # tokens no reference holds
            tokens[r, :12] = np.arange(UNSEEN, UNSEEN + 12)
            tokens[r, 5] = tokens[r, 4]
            length[r] = 12
        elif kind == 13:                               # only EOS
            tokens[r, 0] = EOS
            length[r] = 1
        else:                                          # EOS in the last column
            tokens[r, W - 1] = EOS
            length[r] = W
    length[[15, 60]] = (-3, -2 ** 31)                  # the invalid rows: lengths of 0 (kind 0), negative lengths ...
    video[[46, 91]] = (len(refs), -1)                  # ... and videos outside the bank
    return tokens, length, video


@functools.lru_cache(maxsize=None)
def _want(name, with_eos):
    """The reference's records of the 130 rows, computed once: (ints [130, 12], rouge [130], cider [130])."""
    tokens, length, video = _candidates(name)
    recs = M.Corpus(_corpus(name), with_eos=with_eos).records(tokens.tolist(), length.tolist(), video.tolist())
    return (np.array([r[0] for r in recs], dtype=np.int32), np.array([r[1] for r in recs]), np.array([r[2] for r in recs]))


@functools.lru_cache(maxsize=None)
def _bank(name, with_eos):
    from care_amd import MetricBank

    return MetricBank(_corpus(name), 4096, with_eos=with_eos, device=DEV)


def _stats_raw(bank, tokens, length, video, col0=COL0, ld=LD):
    """care_caption_stats on rows placed at column `col0` of a [rows, ld] buffer full of another token; outputs between canaries."""
    from care_amd import _lib

    rows = tokens.shape[0]
    buf = torch.full((rows, ld), 17, dtype=torch.int32, device=DEV)
    buf[:, col0:col0 + W] = torch.from_numpy(tokens).to(DEV)
    w_rec, rec = _guarded(rows * 12, torch.int32)
    w_rouge, rouge = _guarded(rows, torch.float64)
    len_d, vid_d = torch.from_numpy(length).to(DEV), torch.from_numpy(video).to(DEV)
    _lib.call("care_caption_stats", buf.data_ptr(), ld, col0, W, len_d.data_ptr(), vid_d.data_ptr(), rows, int(bank.with_eos), EOS,
              ctypes.addressof(bank.desc), rec.data_ptr(), rouge.data_ptr())
    torch.cuda.synchronize()
    assert _intact(w_rec, rows * 12) and _intact(w_rouge, rows)
    return rec.cpu().view(rows, 12).numpy(), rouge.cpu().numpy()


def _tie_rows(name, with_eos):
    """Rows at which two reference lengths are equally close to the caption's and the shorter one must win."""
    ints = _want(name, with_eos)[0]
    corpus = M.Corpus(_corpus(name), with_eos=with_eos)
    video = _candidates(name)[2]
    out = []
    for r in range(130):
        if ints[r, 0]:
            L, rl = int(ints[r, 1]), int(ints[r, 2])
            lens = {len(x) for x in corpus.refs[video[r]]}
            if rl < L and (2 * L - rl) in lens:
                out.append(r)
    return out


@pytest.mark.parametrize("with_eos", [False, True], ids=["no_eos", "with_eos"])
@pytest.mark.parametrize("name", sorted(CORPORA))
def test_caption_stats_against_the_reference(name, with_eos):
    tokens, length, video = _candidates(name)
    (ints, rouge, _), bank = _want(name, with_eos), _bank(name, with_eos)
    valid = ints[:, 0] == 1
    print(name, "with_eos", with_eos, "valid", int(valid.sum()), "rouge 0 / 1 / between", int((rouge == 0).sum()), int((rouge == 1).sum()),
          int(((rouge > 0) & (rouge < 1)).sum()), "ties", len(_tie_rows(name, with_eos)), "empty captions",
          int((valid & (ints[:, 1] == 0)).sum()))
    if name == "v40":   # the yardstick itself covers misses, copies, everything between and the closest-length tie
        assert (rouge == 0).sum() >= 9 and (rouge == 1).sum() >= 9 and ((rouge > 0) & (rouge < 1)).sum() >= 40
        assert len(_tie_rows(name, with_eos)) >= 1
        assert (~valid).sum() >= 11 and (valid & (ints[:, 1] == 0)).sum() >= (0 if with_eos else 8)
    got_i, got_r = _stats_raw(bank, tokens, length, video)
    bad = np.nonzero((got_i != ints).any(axis=1))[0]
    assert bad.size == 0, (name, with_eos, int(bad[0]), got_i[bad[0]].tolist(), ints[bad[0]].tolist())
    err = np.abs(got_r - rouge)
    print("worst ROUGE-L deviation", err.max(), "bar", ROUGE_BAR)
    assert err.max() <= ROUGE_BAR, (name, with_eos, int(err.argmax()), err.max())
    # any row count, any place in the batch, any layout: the same bits
    for rows in (1, 3):
        pi, pr = _stats_raw(bank, tokens[:rows], length[:rows], video[:rows])
        assert pi.tobytes() == got_i[:rows].tobytes() and pr.tobytes() == got_r[:rows].tobytes(), rows
    pick = np.array([14, 9, 127, 11])                                  # EOS in the last column, a copy, a plain one, a reversed one
    di, dr = _stats_raw(bank, tokens[pick], length[pick], video[pick], col0=0, ld=W)
    assert di.tobytes() == got_i[pick].tobytes() and dr.tobytes() == got_r[pick].tobytes()
    perm = np.random.RandomState(3).permutation(130)
    ai, ar = _stats_raw(bank, tokens[perm], length[perm], video[perm])
    assert ai.tobytes() == got_i[perm].tobytes() and ar.tobytes() == got_r[perm].tobytes(), "permuting the rows permutes the results"
    ri, rr = _stats_raw(bank, tokens, length, video)
    assert ri.tobytes() == got_i.tobytes() and rr.tobytes() == got_r.tobytes(), "a repeat run gives the same bits"


def test_score_accumulate_scores_on_the_view_of_fed_without_a_synchronisation():
    """MetricBank.score / accumulate / scores on the 130 rows as a `fed[:, 1:]` view, in one batch and in two: the integer totals
    equal the reference's, the scores are the reference's corpus scores; nothing synchronises before `scores`."""
    name = "v40"
    tokens, length, video = _candidates(name)
    bank, corpus = _bank(name, False), M.Corpus(_corpus(name))
    recs = corpus.records(tokens.tolist(), length.tolist(), video.tolist())
    ints, rouge_sum, cider_sum = M.Corpus.totals(recs)
    want = corpus.corpus(recs)
    fed = torch.full((130, W + 1), 2, dtype=torch.int32, device=DEV)
    fed[:, 1:] = torch.from_numpy(tokens).to(DEV)
    len_d, vid_d = torch.from_numpy(length).to(DEV), torch.from_numpy(video).to(DEV)
    one, two = bank.new_totals(), bank.new_totals()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rec = bank.score(fed[:, 1:], len_d, vid_d)
        bank.accumulate(rec, one)
        for lo, hi in ((0, 47), (47, 130)):
            bank.accumulate(bank.score(fed[lo:hi, 1:], len_d[lo:hi], vid_d[lo:hi]), two)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rec["stats"].shape == (130, 12) and rec["rouge"].dtype == torch.float64 and rec["cider"].dtype == torch.float32
    assert one[:12].tolist() == ints == two[:12].tolist(), "the integer totals are exact for any split into batches"
    assert ints[0] >= 110 and ints[1] >= 11
    for t in (one, two):
        sums = t[12:].view(torch.float64).tolist()
        assert abs(sums[0] - rouge_sum) <= 130 * ROUGE_BAR and abs(sums[1] - cider_sum) <= 130 * CIDER_BAR
        got = bank.scores(t)
        for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L"):
            assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
        assert abs(got["CIDEr"] - want["CIDEr"]) <= CIDER_BAR and abs(got["Sum"] - want["Sum"]) <= 2 * CIDER_BAR
        assert got["n_captions"] == float(ints[0]) and got["n_invalid"] == float(ints[1])
    assert bank.score(fed, len_d, vid_d, offset=1, with_cider=False)["cider"] is None
    assert bank.score(fed, len_d, vid_d, offset=1)["stats"].cpu().numpy().tobytes() == rec["stats"].cpu().numpy().tobytes()
    with pytest.raises(TypeError, match="int32"):
        bank.score(fed.long()[:, 1:], len_d, vid_d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.score(fed.cpu()[:, 1:], len_d, vid_d)
    with pytest.raises(ValueError, match="64"):
        bank.score(torch.zeros(2, 66, dtype=torch.int32, device=DEV), len_d[:2], vid_d[:2])


def test_caption_stats_refusals_and_the_empty_batch_write_nothing():
    from care_amd import _lib

    bank = _bank("v3", False)
    lib, stream = _lib.load(), _lib.stream_ptr()
    buf = torch.full((4, LD), 17, dtype=torch.int32, device=DEV)
    ln = torch.full((4,), 5, dtype=torch.int32, device=DEV)
    vd = torch.zeros(4, dtype=torch.int32, device=DEV)
    w_rec, rec = _guarded(48, torch.int32)
    w_rouge, rouge = _guarded(4, torch.float64)
    T, L, V_, R, Q, B = buf.data_ptr(), ln.data_ptr(), vd.data_ptr(), rec.data_ptr(), rouge.data_ptr(), ctypes.addressof(bank.desc)
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, 0, 0, EOS, B, R, Q, stream) == 0
    assert lib.care_caption_stats(None, LD, COL0, W, L, V_, 4, 0, EOS, B, R, Q, stream) == EINVAL
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, 4, 0, EOS, None, R, Q, stream) == EINVAL
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, 4, 0, EOS, B, None, Q, stream) == EINVAL
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, -1, 0, EOS, B, R, Q, stream) == EINVAL
    assert lib.care_caption_stats(T, W, COL0, W, L, V_, 4, 0, EOS, B, R, Q, stream) == EINVAL, "ld below the caption width"
    assert lib.care_caption_stats(T, LD, COL0, W + 1, L, V_, 4, 0, EOS, B, R, Q, stream) == EINVAL, "more than 64 tokens"
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, 4, 0, EOS, B, R, Q + 4, stream) == EALIGN
    keep = bank.desc.clip_keys
    bank.desc.clip_keys = keep + 4
    assert lib.care_caption_stats(T, LD, COL0, W, L, V_, 4, 0, EOS, B, R, Q, stream) == EALIGN
    bank.desc.clip_keys = keep
    torch.cuda.synchronize()
    assert bool((w_rec == CANARY[torch.int32]).all()) and bool((w_rouge == CANARY[torch.float64]).all())


# ------------------------------------------------------------------------------------------------ care_caption_totals
def _totals_raw(batches, with_cider=True):
    """care_caption_totals over `batches` of (rec int32 [n, 12], rouge float64 [n], cider fp32 [n]) into zeroed guarded totals."""
    from care_amd import _lib

    w_i, ti = _guarded(12, torch.int64)
    w_d, td = _guarded(2, torch.float64)
    ti.zero_()
    td.zero_()
    for rec, rouge, cider in batches:
        r_d, q_d, c_d = torch.from_numpy(rec).to(DEV), torch.from_numpy(rouge).to(DEV), torch.from_numpy(cider).to(DEV)
        _lib.call("care_caption_totals", r_d.data_ptr(), q_d.data_ptr(), c_d.data_ptr() if with_cider else None, rec.shape[0],
                  ti.data_ptr(), td.data_ptr())
    torch.cuda.synchronize()
    assert _intact(w_i, 12) and _intact(w_d, 2)
    return ti.cpu().numpy(), td.cpu().numpy()


@pytest.mark.parametrize("rows", [1, 3, 130, 1030])
def test_caption_totals_are_exact_in_the_integers_for_any_split(rows):
    rng = np.random.RandomState(rows)
    rec = rng.randint(0, 2 ** 20, size=(rows, 12)).astype(np.int32)
    rec[:, 0] = rng.rand(rows) < 0.8
    rec[0, 0] = 1
    rec[0, 1:11] = 2 ** 31 - 1            # the sums are 64-bit
    rec[:, 11] = 0
    if rows >= 3:
        rec[1, 0] = 0                     # an invalid row is counted and adds nothing, whatever it holds
    rouge, cider = rng.rand(rows), (rng.rand(rows) * 10).astype(np.float32)
    valid = rec[:, 0] == 1
    want_i = np.concatenate([[valid.sum(), (~valid).sum()], rec[valid, 1:11].astype(np.int64).sum(axis=0)])
    want_d = np.array([rouge[valid].sum(), cider[valid].astype(np.float64).sum()])
    got_i, got_d = _totals_raw([(rec, rouge, cider)])
    assert got_i.tolist() == want_i.tolist()
    assert np.abs(got_d - want_d).max() <= 1e-12 * max(1.0, want_d.max())
    again_i, again_d = _totals_raw([(rec, rouge, cider)])
    assert again_i.tobytes() == got_i.tobytes() and again_d.tobytes() == got_d.tobytes(), "a repeat run gives the same bits"
    none_i, none_d = _totals_raw([(rec, rouge, cider)], with_cider=False)
    assert none_i.tolist() == want_i.tolist() and none_d[0] == got_d[0] and none_d[1] == 0.0
    if rows >= 3:
        cut = rows // 3
        two_i, two_d = _totals_raw([(rec[:cut], rouge[:cut], cider[:cut]), (rec[cut:], rouge[cut:], cider[cut:])])
        assert two_i.tolist() == want_i.tolist(), "two batches accumulated equal one, the integers exactly"
        assert np.abs(two_d - want_d).max() <= 1e-12 * max(1.0, want_d.max())


def test_caption_totals_refusals_write_nothing():
    from care_amd import _lib

    lib, stream = _lib.load(), _lib.stream_ptr()
    rec = torch.ones(4, 12, dtype=torch.int32, device=DEV)
    rouge = torch.ones(4, dtype=torch.float64, device=DEV)
    w_i, ti = _guarded(12, torch.int64)
    w_d, td = _guarded(2, torch.float64)
    R, Q, I, D = rec.data_ptr(), rouge.data_ptr(), ti.data_ptr(), td.data_ptr()
    assert lib.care_caption_totals(R, Q, None, 0, I, D, stream) == 0
    assert lib.care_caption_totals(None, Q, None, 4, I, D, stream) == EINVAL
    assert lib.care_caption_totals(R, Q, None, 4, None, D, stream) == EINVAL
    assert lib.care_caption_totals(R, Q, None, -1, I, D, stream) == EINVAL
    assert lib.care_caption_totals(R, Q, None, 4, I + 4, D, stream) == EALIGN
    assert lib.care_caption_totals(R, Q, None, 4, I, D + 4, stream) == EALIGN
    torch.cuda.synchronize()
    assert bool((w_i == CANARY[torch.int64]).all()) and bool((w_d == CANARY[torch.float64]).all())


# ------------------------------------------------------------------------------------------------ care_beam_winner
@pytest.mark.parametrize("alpha", [1.0, 0.7])
@pytest.mark.parametrize("cap", [5, 8])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_beam_winner_is_the_first_of_the_stable_sort(B, cap, alpha):
    from care_amd import _lib
    from care_amd.translator import Translator_ARFormer

    T1 = 30
    tr = Translator_ARFormer({"beam_alpha": alpha, "max_len": T1, "beam_size": 5})
    rng = np.random.RandomState(B * 100 + cap)
    nfin = (np.arange(B) % (cap + 3)).astype(np.int32)          # 0 .. cap + 2: none, some, all, more than the block holds
    if B == 1:
        nfin[0] = cap
    flen = rng.randint(1, T1 + 1, size=(B, cap)).astype(np.int32)
    fscore = (-rng.rand(B, cap) * 20).astype(np.float32)
    fhyp = rng.randint(4, 500, size=(B, cap, T1)).astype(np.int32)
    for b in range(B):
        if b % 3 == 1:                                          # the same score and length twice: the earlier one wins
            fscore[b, -1], flen[b, -1] = fscore[b, 0], flen[b, 0]
            fscore[b, 1:-1] -= 25.0
        elif b % 3 == 2 and alpha == 1.0:                       # equal quotients of different pairs: -2 / 2 == -4 / 4, exactly
            fscore[b], flen[b] = -30.0, 3
            fscore[b, cap - 2], flen[b, cap - 2] = -4.0, 4
            fscore[b, 1], flen[b, 1] = -2.0, 2
    norm = tr._norm(fscore, flen)
    key = np.where(np.arange(cap)[None, :] < np.minimum(nfin, cap)[:, None], -norm, np.inf)
    win = np.argsort(key, axis=1, kind="stable")[:, 0]
    want_len = np.where(nfin > 0, flen[np.arange(B), win], 0).astype(np.int32)
    want_tok = np.where(np.arange(T1)[None, :] < want_len[:, None], fhyp[np.arange(B), win], 0).astype(np.int32)
    if B == 130:
        ties = [b for b in range(B) if (key[b] == key[b].min()).sum() >= 2 and np.isfinite(key[b].min())]
        assert len(ties) >= 10, "the inputs must hold exact ties for the first place"
    w_t, tokens = _guarded(B * T1, torch.int32)
    w_l, length = _guarded(B, torch.int32)
    dev = [torch.from_numpy(a).to(DEV) for a in (nfin, fscore, flen, fhyp, tr._len_pow)]
    _lib.call("care_beam_winner", *[t.data_ptr() for t in dev[:4]], B, cap, T1, dev[4].data_ptr(), dev[4].numel(), tokens.data_ptr(),
              length.data_ptr())
    torch.cuda.synchronize()
    assert _intact(w_t, B * T1) and _intact(w_l, B)
    assert length.cpu().numpy().tolist() == want_len.tolist()
    assert np.array_equal(tokens.cpu().numpy().reshape(B, T1), want_tok)

"""GPU: care_consensus_score (csrc/consensus.hip) through the raw ABI against tests/consensus_reference.py (float64, plain Python).

A corpus of 40 videos x 5 references over tokens in [4, 60); 130 clips in five groups, one per n in {2, 3, 5, 16, 32} (n is an
argument of the launch), a clip's candidates one reference with 0 - 3 tokens substituted, a fifth of them truncated, most with
a trailing EOS - and by hand: candidates of 0, 1, 3 and 64 tokens, an EOS in the last column, a clip of exact duplicates, clips
with count 0, 1 and n - 2, and a clip with n = 1.  `score` and `pairs` within 2e-6 absolute of float64 - the bar
tests/test_gpu_reward_kernels.py holds care_cider_score to: the kernel computes in double and rounds once to fp32, a score is
at most 10, half an fp32 ulp at 10 is 4.8e-7 and the bar is four times that.  The winner is judged by the REFERENCE's scores:
never worse than its best by more than 1e-9 (exact duplicates make near-ties that the reference itself resolves in its last
bits), exactly its winner where its gap exceeds 1e-6, and the lowest index where the device's best scores are bit-equal.
Every output lies between canaries.  Same bits for a subset of the clips, a permutation, a repeat, another column offset and
row stride, and the fp16 library.

Measured on one MI355X: worst deviation from float64 4.8e-7 (pairs, n = 16) and 4.6e-7 (score, n = 3 with EOS) over the ten
cases, bar 2e-6, scores up to 10; the reference has 47 clips with a top-2 gap above 1e-3, 66 exact ties and 3 gaps below 1e-9;
between 5 (n = 5) and 24 (n = 32) of a group's 26 clips have several best device scores that are bit-equal.  The whole file: 3.4 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cider_reference as C
import consensus_reference as R
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

GAP = 8
BAR = 2e-6
W, COL0, LD = 64, 1, 70
EOS = C.EOS
EINVAL, ESHAPE = -1, -3
GROUPS = (2, 3, 5, 16, 32)
PER_GROUP = 26                    # 5 x 26 = 130 clips


@functools.lru_cache(maxsize=None)
def _corpus():
    rng = np.random.RandomState(4005)
    refs = []
    for _ in range(40):
        video = []
        for _ in range(5):
            toks = rng.randint(4, 60, size=int(rng.randint(4, 21))).tolist()
            video.append(toks + [EOS] if rng.rand() < 0.8 else toks)
        refs.append(video)
    return refs


@functools.lru_cache(maxsize=None)
def _group(n):
    """(tokens [26 n, W] int32, length [26 n], count [26]) of the group of n candidates a clip."""
    refs = _corpus()
    rng = np.random.RandomState(900 + n)
    rows = PER_GROUP * n
    tokens = rng.randint(4, 60, size=(rows, W)).astype(np.int32)   # what lies behind a caption's end is never read
    length = np.zeros(rows, dtype=np.int32)
    for b in range(PER_GROUP):
        video = refs[int(rng.randint(40))]
        base = [t for t in video[int(rng.randint(5))] if t != EOS]
        for j in range(n):
            cand = list(base)
            for _ in range(int(rng.randint(0, 4))):
                cand[int(rng.randint(len(cand)))] = int(rng.randint(4, 60))
            if rng.rand() < 0.2:
                cand = cand[:int(rng.randint(1, len(cand) + 1))]
            if rng.rand() < 0.7:
                cand = cand + [EOS]
            r = b * n + j
            tokens[r, :len(cand)] = cand
            length[r] = len(cand)
    count = np.full(PER_GROUP, n, dtype=np.int32)
    # by hand (the clips 20 .. 25 of every group)
    r = 20 * n
    length[r] = 0                                         # an empty candidate ...
    length[r + 1] = 1                                     # ... one token (orders 2 - 4 have no n-gram)
    tokens[r + 1, 0] = 7
    if n >= 3:
        length[r + 2] = 3
    r = 21 * n
    length[r] = W                                         # 64 tokens: 250 keys, four rounds of the lanes
    tokens[r + 1] = tokens[r]                             # ... next to a copy that ends with an EOS in the last column
    tokens[r + 1, W - 1] = EOS
    length[r + 1] = W
    if n >= 3:
        tokens[r + 2] = tokens[r]
        tokens[r + 2, 30] = 61
        length[r + 2] = W + 9                             # (a length beyond the width is cut to it)
    r = 22 * n
    for j in range(1, n):                                 # exact duplicates
        tokens[r + j] = tokens[r]
        length[r + j] = length[r]
    count[23], count[24], count[25] = 0, 1, max(0, n - 2)
    if n == 32:
        count[19] = 40                                    # (clamped to n)
    if n == 16:
        count[19] = -3                                    # (clamped to 0)
    return tokens, length, count


@functools.lru_cache(maxsize=None)
def _want(n, with_eos):
    """The float64 reference of a group: (score [26, n], pairs [26, n, n], winner [26]).  Computed once, left unchanged."""
    tokens, length, count = _group(n)
    corpus = C.Corpus(_corpus(), with_eos=with_eos)
    s, p, w = R.clips(corpus, tokens.tolist(), np.minimum(length, W).tolist(), n, count.tolist())
    out = np.array(s), np.array(p), np.array(w)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _bank(with_eos):
    from care_amd import CiderBank

    return CiderBank(_corpus(), 4096, with_eos=with_eos, device=DEV)


def _guarded(n, dtype, fill):
    whole = torch.full((n + 2 * GAP,), fill, dtype=dtype, device=DEV)
    return whole, whole[GAP:GAP + n]


def _intact(whole, n, fill):
    w = whole.cpu()
    return bool((w[:GAP] == fill).all()) and bool((w[GAP + n:] == fill).all())


def _run(bank, tokens, length, n, count=None, col0=COL0, ld=LD, variant="", with_pairs=True, with_row=True):
    """care_consensus_score on rows placed at column `col0` of a [rows, ld] buffer full of another token; every output
    between canaries.  Returns CPU tensors (score [B, n], pairs [B, n, n] or None, winner [B], winner_row [B] or None)."""
    from care_amd import _lib

    rows = tokens.shape[0]
    B = rows // n
    buf = torch.full((rows, ld), 17, dtype=torch.int32, device=DEV)
    buf[:, col0:col0 + W] = torch.from_numpy(tokens).to(DEV)
    len_d = torch.from_numpy(length).to(DEV)
    cnt_d = None if count is None else torch.from_numpy(count).to(DEV)
    w_s, score = _guarded(B * n, torch.float32, -7.25)
    w_p, pairs = _guarded(B * n * n, torch.float32, -7.25)
    w_w, winner = _guarded(B, torch.int32, -77)
    w_r, row = _guarded(B, torch.int32, -77)
    _lib.call("care_consensus_score", buf.data_ptr(), ld, col0, W, len_d.data_ptr(), None if cnt_d is None else cnt_d.data_ptr(),
              B, n, int(bank.with_eos), EOS, ctypes.addressof(bank.desc), score.data_ptr(), pairs.data_ptr() if with_pairs else None,
              winner.data_ptr(), row.data_ptr() if with_row else None, variant=variant)
    torch.cuda.synchronize()
    assert _intact(w_s, B * n, -7.25) and _intact(w_p, B * n * n, -7.25) and _intact(w_w, B, -77) and _intact(w_r, B, -77)
    if not with_pairs:
        assert bool((w_p == -7.25).all())
    if not with_row:
        assert bool((w_r == -77).all())
    return (score.cpu().view(B, n), pairs.cpu().view(B, n, n) if with_pairs else None, winner.cpu(),
            row.cpu() if with_row else None)


def _bits(out):
    return [None if t is None else t.numpy().tobytes() for t in out]


def test_the_generator_gives_clear_winners_and_exact_ties():
    """So that the winner checks below mean something: of the 130 clips at least 40 have a top-2 gap above 1e-3 in the reference
    and at least one an exact tie."""
    clear = ties = close = 0
    for n in GROUPS:
        score, _, _ = _want(n, False)
        _, _, count = _group(n)
        for b in range(PER_GROUP):
            m = min(max(int(count[b]), 0), n)
            if m < 2:
                continue
            top = np.sort(score[b, :m])[::-1]
            gap = top[0] - top[1]
            clear += gap > 1e-3
            ties += gap == 0.0
            close += 0.0 < gap < 1e-9
    print("clips with a top-2 gap above 1e-3:", clear, "exact ties:", ties, "gaps in (0, 1e-9):", close)
    assert clear >= 40 and ties >= 1


@pytest.mark.parametrize("with_eos", [False, True], ids=["no_eos", "with_eos"])
@pytest.mark.parametrize("n", GROUPS)
def test_consensus_against_the_float64_reference(n, with_eos):
    tokens, length, count = _group(n)
    want_s, want_p, want_w = _want(n, with_eos)
    bank = _bank(with_eos)
    score, pairs, winner, row = got = _run(bank, tokens, length, n, count)
    err_s = np.abs(score.double().numpy() - want_s)
    err_p = np.abs(pairs.double().numpy() - want_p)
    print("n", n, "with_eos", with_eos, "worst deviation: score", err_s.max(), "pairs", err_p.max(), "bar", BAR,
          "largest score", want_s.max())
    assert want_s.max() > 5 and (want_s > 0).sum() >= 20
    assert err_s.max() <= BAR, (int(err_s.argmax()), err_s.max())
    assert err_p.max() <= BAR, (int(err_p.argmax()), err_p.max())
    # the diagonal, and everything beyond `count`
    s, p = score.numpy(), pairs.numpy()
    for b in range(PER_GROUP):
        m = min(max(int(count[b]), 0), n)
        assert (p[b][np.arange(n), np.arange(n)] == 0).all()
        assert (p[b, m:] == 0).all() and (p[b, :, m:] == 0).all() and (s[b, m:] == 0).all()
        if m <= 1:
            assert (s[b] == 0).all()
    # the winner: judged by the reference's scores, for EVERY clip
    w = winner.numpy()
    exact = equal = 0
    for b in range(PER_GROUP):
        m = min(max(int(count[b]), 0), n)
        if m == 0:
            assert w[b] == -1 and row[b] == -1
            continue
        assert 0 <= w[b] < m and row[b] == b * n + w[b]
        ref = want_s[b, :m]
        assert ref[w[b]] >= ref.max() - 1e-9, (b, int(w[b]), ref.tolist())
        top = np.sort(ref)[::-1]
        if m == 1 or top[0] - top[1] > 1e-6:
            assert w[b] == want_w[b], (b, int(w[b]), int(want_w[b]))
            exact += 1
        best = np.nonzero(s[b, :m] == s[b, :m].max())[0]
        if len(best) > 1:
            equal += 1
        assert w[b] == best[0], (b, int(w[b]), best.tolist(), s[b, :m].tolist())
    print("winners held to the reference's exactly:", exact, "clips whose best device scores are bit-equal:", equal)
    # the same bits whatever else is in the launch, wherever the candidates lie, in both libraries
    for clips in (1, 3):
        part = _run(bank, tokens[:clips * n], length[:clips * n], n, count[:clips])
        assert _bits(part)[:3] == _bits((score[:clips], pairs[:clips], winner[:clips])), clips
    perm = np.random.RandomState(3).permutation(PER_GROUP)
    rows = (perm[:, None] * n + np.arange(n)[None, :]).reshape(-1)
    again = _run(bank, tokens[rows], length[rows], n, count[perm])
    assert _bits(again)[:3] == _bits((score[perm], pairs[perm], winner[perm])), "permuting the clips permutes the results"
    assert _bits(_run(bank, tokens, length, n, count)) == _bits(got), "a repeat run gives the same bits"
    assert _bits(_run(bank, tokens, length, n, count, col0=0, ld=W)) == _bits(got), "dense rows"
    assert _bits(_run(bank, tokens, length, n, count, col0=9, ld=83)) == _bits(got), "another offset in a wider buffer"
    assert _bits(_run(bank, tokens, length, n, count, variant="f16")) == _bits(got), "the fp16 library"
    # the optional outputs left out: the others keep their bits
    lean = _run(bank, tokens, length, n, count, with_pairs=False, with_row=False)
    assert lean[1] is None and lean[3] is None and _bits(lean)[0] == _bits(got)[0] and _bits(lean)[2] == _bits(got)[2]
    # without `count` every candidate is valid
    full = _run(bank, tokens[:19 * n], length[:19 * n], n, None)
    assert _bits(full)[:3] == _bits((score[:19], pairs[:19], winner[:19]))


def test_one_candidate_a_clip():
    """n = 1: nothing to agree with - the score is 0 and the candidate wins; count 0 leaves no winner."""
    tokens, length, _ = _group(2)
    bank = _bank(False)
    score, pairs, winner, row = _run(bank, tokens[:4], length[:4], 1, np.array([1, 1, 0, 1], dtype=np.int32))
    assert score.view(-1).tolist() == [0.0] * 4 and pairs.view(-1).tolist() == [0.0] * 4
    assert winner.tolist() == [0, 0, -1, 0] and row.tolist() == [0, 1, -1, 3]
    want = R.clips(C.Corpus(_corpus()), tokens[:4].tolist(), length[:4].tolist(), 1, [1, 1, 0, 1])
    assert want[0] == [[0.0]] * 4 and want[2] == [0, 0, -1, 0]


def test_anchors_and_the_view_of_fed_without_a_synchronisation():
    """consensus_select on the `fed[:, 1:]` view of a [rows, T + 1] buffer: identical candidates score 10 (7.5 with three
    tokens), disjoint ones 0, a bank of one video gives 0 everywhere and winner 0."""
    from care_amd import CiderBank, consensus_select

    bank = _bank(False)
    a = [t for t in next(r for video in _corpus() for r in video if len(r) >= 9) if t != EOS][:7]
    rows = [a + [EOS], a + [EOS], a[:3] + [EOS], a[:3], [4, 5, 6, 7, 8], [20, 21, 22, 23, 24], [3000, 3001, 3002, 3003], [3000, 3001, 3002, 3003]]
    fed = torch.zeros(8, 12, dtype=torch.int32)
    fed[:, 0] = 2
    for r, toks in enumerate(rows):
        fed[r, 1:1 + len(toks)] = torch.tensor(toks, dtype=torch.int32)
    fed = fed.to(DEV)
    length = torch.tensor([len(t) for t in rows], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score, winner, winner_row, pairs = consensus_select(fed[:, 1:], length, 2, bank, pairs=True)
        again = consensus_select(fed, length, 2, bank, offset=1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert score.dtype == torch.float32 and tuple(score.shape) == (4, 2) and tuple(pairs.shape) == (4, 2, 2)
    assert winner.dtype == torch.int32 and winner_row.dtype == torch.int32 and again[3] is None
    want = np.array([[10.0, 10.0], [7.5, 7.5], [0.0, 0.0], [10.0, 10.0]])
    assert np.abs(score.cpu().double().numpy() - want).max() <= BAR
    assert winner.tolist() == [0, 0, 0, 0] and winner_row.tolist() == [0, 2, 4, 6]
    assert again[0].cpu().numpy().tobytes() == score.cpu().numpy().tobytes()
    one = CiderBank(_corpus()[:1], 4096, device=DEV)
    s1, w1, _, _ = consensus_select(fed[:, 1:], length, 4, one)
    assert bool((s1 == 0).all()) and w1.tolist() == [0, 0], "a corpus of one video has ln N = 0"
    # count through the Python entry, and its refusals on the device
    cnt = torch.tensor([2, 1, 0, 2], dtype=torch.int32, device=DEV)
    s2, w2, r2, _ = consensus_select(fed[:, 1:], length, 2, bank, count=cnt)
    assert w2.tolist() == [0, 0, -1, 0] and r2.tolist() == [0, 2, -1, 6] and s2[1].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match="count"):
        consensus_select(fed[:, 1:], length, 2, bank, count=cnt.long())
    with pytest.raises(ValueError, match="count"):
        consensus_select(fed[:, 1:], length, 2, bank, count=cnt[:3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consensus_select(fed[:, 1:], length, 2, bank, count=cnt.cpu())
    with pytest.raises(ValueError, match="multiple"):
        consensus_select(fed[:, 1:], length, 3, bank)
    with pytest.raises(ValueError, match="1 .. 32"):
        consensus_select(fed[:, 1:], length, 33, bank)
    with pytest.raises(TypeError, match="int32"):
        consensus_select(fed.long()[:, 1:], length, 2, bank)
    with pytest.raises(ValueError, match="64"):
        consensus_select(torch.zeros(4, 66, dtype=torch.int32, device=DEV), length[:4], 2, bank)


def test_the_empty_batch_and_the_refusals_write_nothing():
    from care_amd import _lib

    bank = _bank(False)
    lib, stream = _lib.load(), _lib.stream_ptr()
    buf = torch.full((66, LD), 17, dtype=torch.int32, device=DEV)
    ln = torch.full((66,), 5, dtype=torch.int32, device=DEV)
    w_s, score = _guarded(66, torch.float32, -7.25)
    w_w, winner = _guarded(2, torch.int32, -77)
    T, L, S, Wn, B = buf.data_ptr(), ln.data_ptr(), score.data_ptr(), winner.data_ptr(), ctypes.addressof(bank.desc)
    call = lib.care_consensus_score
    assert call(T, LD, COL0, W, L, None, 0, 5, 0, EOS, B, S, None, Wn, None, stream) == 0, "clips == 0 returns at once"
    assert call(T, LD, COL0, W, L, None, 2, 33, 0, EOS, B, S, None, Wn, None, stream) == ESHAPE, "at most 32 candidates a clip"
    assert call(T, LD, COL0, W + 1, L, None, 2, 5, 0, EOS, B, S, None, Wn, None, stream) == ESHAPE, "at most 64 tokens"
    assert call(None, LD, COL0, W, L, None, 2, 5, 0, EOS, B, S, None, Wn, None, stream) == EINVAL
    assert call(T, LD, COL0, W, None, None, 2, 5, 0, EOS, B, S, None, Wn, None, stream) == EINVAL
    assert call(T, LD, COL0, W, L, None, 2, 5, 0, EOS, None, S, None, Wn, None, stream) == EINVAL
    assert call(T, LD, COL0, W, L, None, 2, 5, 0, EOS, B, None, None, Wn, None, stream) == EINVAL
    assert call(T, LD, COL0, W, L, None, 2, 5, 0, EOS, B, S, None, None, None, stream) == EINVAL
    assert call(T, LD, COL0, W, L, None, 2, 0, 0, EOS, B, S, None, Wn, None, stream) == EINVAL
    assert call(T, W, COL0, W, L, None, 2, 5, 0, EOS, B, S, None, Wn, None, stream) == EINVAL, "ld below the caption width"
    torch.cuda.synchronize()
    assert bool((w_s == -7.25).all()) and bool((w_w == -77).all())

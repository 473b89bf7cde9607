"""GPU: the kernels of self-critical training (csrc/reward.hip) through the raw ABI.

care_cider_score against tests/cider_reference.py (float64, plain Python) within 2e-6 absolute: the kernel computes in double
and rounds once to fp32, scores are at most 10, half an fp32 ulp at 10 is 4.8e-7 and the bar is four times that.
care_reward_advantage against the BITS of the same fp32 expression in torch.  care_reward_loss_fwd / _bwd under `_check`'s
yardstick rule of tests/test_gpu_backward_kernels.py: error against float64 at most FACTOR x the error of torch's own fp32
evaluation of the same formula + FLOOR x scale.  Every output lies in a guarded buffer between canaries.  The forward shares
its row sweeps with care_lang_loss_fwd (csrc/vocab_row.h): the two write the same BITS of rmax, lsum and logp.

Measured on one MI355X: care_cider_score's worst deviation from float64 1.5e-7 / 6.8e-8 / 4.8e-7 on the corpora of 2 / 3 / 40
videos (bar 2e-6; scores up to 9.6); care_reward_loss_fwd / _bwd worst error / yardstick 2.54 (V 130, 7 x 29, dlogits) and worst
error / bar 0.18 over the twelve shapes x four layouts; with unit advantages the loss has the bits of care_lang_loss_fwd's
sums[1] / counts[1] (53.769203 both, float64 53.7692067).  The whole file: 3.5 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cider_reference as C
from test_gpu_backward_kernels import DEV, _check, _gen, _Worst

pytestmark = pytest.mark.gpu

GAP = 8
CANARY = -7.25
EINVAL, EALIGN = -1, -2
BAR = 2e-6
W, COL0, LD = 64, 1, 70          # caption width, the column offset of fed[:, 1:], a padded row stride
EOS = C.EOS
UNSEEN = 3000                    # tokens from here on occur in no reference


def _guarded(n, dtype=torch.float32, fill=CANARY):
    """(whole, view): n elements between GAP canaries on either side, on the device."""
    whole = torch.full((n + 2 * GAP,), fill, dtype=dtype, device=DEV)
    return whole, whole[GAP:GAP + n]


def _intact(whole, n, fill=CANARY):
    w = whole.cpu()
    return bool((w[:GAP] == fill).all()) and bool((w[GAP + n:] == fill).all())


# ------------------------------------------------------------------------------------------------ care_cider_score
CORPORA = {"v2": (2, (1, 5)), "v3": (3, (20, 41, 1)), "v40": (40, (1, 5, 20, 41))}


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """refs of a corpus: captions of 1 .. 30 tokens over a small vocabulary (so that n-grams repeat within and between videos),
    most with a trailing EOS; one reference of 64 tokens."""
    n_videos, counts = CORPORA[name]
    rng = np.random.RandomState(100 + n_videos)
    refs = []
    for v in range(n_videos):
        video = []
        for _ in range(counts[v % len(counts)]):
            n = int(rng.randint(1, 31))
            toks = rng.randint(6, 30, size=n).tolist()
            video.append(toks + [EOS] if rng.rand() < 0.8 else toks)
        refs.append(video)
    refs[0][0] = rng.randint(6, 30, size=W).tolist()
    return refs


@functools.lru_cache(maxsize=None)
def _candidates(name):
    """130 rows (tokens [130, W] int32, length, video) that cycle through the candidate kinds, over all videos of the corpus."""
    refs = _corpus(name)
    rng = np.random.RandomState(7)
    tokens = rng.randint(6, 30, size=(130, W)).astype(np.int32)       # what lies behind a caption's end is never read
    length, video = np.zeros(130, dtype=np.int32), np.zeros(130, dtype=np.int32)
    plain = (0, 1, 2, 3, 4, 5, 30, 64)
    for r in range(130):
        v = video[r] = r % len(refs)
        kind = r % 14
        ref = refs[v][r % len(refs[v])]
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
        elif kind == 11:                               # tokens no reference holds
            tokens[r, :12] = np.arange(UNSEEN, UNSEEN + 12)
            tokens[r, 5] = tokens[r, 4]
            length[r] = 12
        elif kind == 12:                               # only EOS
            tokens[r, 0] = EOS
            length[r] = 1
        else:                                          # EOS in the last column
            tokens[r, W - 1] = EOS
            length[r] = W
    return tokens, length, video


@functools.lru_cache(maxsize=None)
def _want(name, with_eos):
    tokens, length, video = _candidates(name)
    corpus = C.Corpus(_corpus(name), with_eos=with_eos)
    return np.array(corpus.scores(tokens.tolist(), length.tolist(), video.tolist()))


@functools.lru_cache(maxsize=None)
def _bank(name, with_eos):
    from care_amd import CiderBank

    return CiderBank(_corpus(name), 4096, with_eos=with_eos, device=DEV)


def _score_raw(bank, tokens, length, video, col0=COL0, ld=LD, want_bad=False):
    """care_cider_score on rows placed at column `col0` of a [rows, ld] buffer full of another token; out between canaries."""
    from care_amd import _lib

    rows = tokens.shape[0]
    buf = torch.full((rows, ld), 17, dtype=torch.int32, device=DEV)
    buf[:, col0:col0 + W] = torch.from_numpy(tokens).to(DEV)
    whole, out = _guarded(rows)
    bad = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    len_d, vid_d = torch.from_numpy(length).to(DEV), torch.from_numpy(video).to(DEV)
    _lib.call("care_cider_score", buf.data_ptr(), ld, col0, W, len_d.data_ptr(), vid_d.data_ptr(), rows, int(bank.with_eos), EOS,
              ctypes.addressof(bank.desc), out.data_ptr(), bad[1:].data_ptr() if want_bad else None)
    torch.cuda.synchronize()
    assert _intact(whole, rows)
    if want_bad:
        assert bad.tolist()[0] == -5 and bad.tolist()[2] == -5
        return out.cpu(), int(bad[1])
    return out.cpu()


@pytest.mark.parametrize("with_eos", [False, True], ids=["no_eos", "with_eos"])
@pytest.mark.parametrize("name", sorted(CORPORA))
def test_cider_score_against_the_float64_reference(name, with_eos):
    tokens, length, video = _candidates(name)
    want, bank = _want(name, with_eos), _bank(name, with_eos)
    assert want.max() > 5 and (want == 0).sum() >= 9 and (want > 0).sum() >= 40, "the candidates must cover copies and misses"
    got = _score_raw(bank, tokens, length, video)
    err = np.abs(got.double().numpy() - want)
    print(name, "with_eos", with_eos, "rows 130: worst deviation", err.max(), "bar", BAR, "largest score", want.max())
    assert err.max() <= BAR, (name, with_eos, int(err.argmax()), err.max())
    # any row count, any place in the batch, any layout: the same bits
    for rows in (1, 3):
        part = _score_raw(bank, tokens[:rows], length[:rows], video[:rows])
        assert part.numpy().tobytes() == got[:rows].numpy().tobytes(), rows
    pick = np.array([13, 9, 127])                                      # EOS in the last column, a copy, a long one
    dense = _score_raw(bank, tokens[pick], length[pick], video[pick], col0=0, ld=W)
    assert dense.numpy().tobytes() == got[pick].numpy().tobytes()
    perm = np.random.RandomState(3).permutation(130)
    again = _score_raw(bank, tokens[perm], length[perm], video[perm])
    assert again.numpy().tobytes() == got[perm].numpy().tobytes(), "permuting the rows must permute the results bit for bit"
    assert _score_raw(bank, tokens, length, video).numpy().tobytes() == got.numpy().tobytes(), "a repeat run gives the same bits"


def test_cider_score_anchors_and_the_view_of_fed():
    """The hand-worked anchors of the issue through CiderBank.score on the `fed[:, 1:]` view of a [rows, T + 1] buffer, without a
    host synchronisation."""
    from care_amd import CiderBank

    bank = CiderBank([[[10, 11]], [[10, 12]]], 100, device=DEV)
    fed = torch.tensor([[2, 10, 11, 3, 9], [2, 10, 12, 3, 0], [2, 10, 11, 11, 3], [2, 3, 0, 0, 0], [2, 10, 11, 0, 0]],
                       dtype=torch.int32, device=DEV)
    length = torch.tensor([3, 3, 4, 1, 0], dtype=torch.int32, device=DEV)
    video = torch.zeros(5, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = bank.score(fed[:, 1:], length, video)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = [5.0, 0.0, 2.9761432456900, 0.0, 0.0]
    assert got.dtype == torch.float32 and np.abs(got.cpu().double().numpy() - np.array(want)).max() <= BAR
    assert got[0].item() == 5.0
    assert bank.score(fed, length, video, offset=1).cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    one = CiderBank([[[10, 11], [10, 12]]], 100, device=DEV)
    assert bool((one.score(fed[:, 1:], length, video) == 0).all()), "a corpus of one video has ln N = 0"
    with pytest.raises(TypeError, match="int32"):
        bank.score(fed.long()[:, 1:], length, video)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bank.score(fed.cpu()[:, 1:], length, video)
    with pytest.raises(ValueError, match="64"):
        bank.score(torch.zeros(2, 66, dtype=torch.int32, device=DEV), length[:2], video[:2])


def test_cider_score_out_of_range_videos_refusals_and_the_empty_batch():
    from care_amd import _lib

    name = "v3"
    tokens, length, video = _candidates(name)
    bank, want = _bank(name, False), _want(name, False)
    video = video[:10].copy()
    video[[2, 5, 7]] = (-1, 3, 2 ** 30)
    got, bad = _score_raw(bank, tokens[:10], length[:10], video, want_bad=True)
    assert bad == 3 and got[[2, 5, 7]].tolist() == [0.0, 0.0, 0.0]
    keep = np.array([0, 1, 3, 4, 6, 8, 9])
    assert np.abs(got.double().numpy()[keep] - want[keep]).max() <= BAR
    assert _score_raw(bank, tokens[:10], length[:10], _candidates(name)[2][:10], want_bad=True)[1] == 0
    # refusals and rows == 0 write nothing
    lib, stream = _lib.load(), _lib.stream_ptr()
    buf = torch.full((4, LD), 17, dtype=torch.int32, device=DEV)
    ln = torch.full((4,), 5, dtype=torch.int32, device=DEV)
    vd = torch.zeros(4, dtype=torch.int32, device=DEV)
    whole, out = _guarded(4)
    T, L, V_, O, B = buf.data_ptr(), ln.data_ptr(), vd.data_ptr(), out.data_ptr(), ctypes.addressof(bank.desc)
    assert lib.care_cider_score(T, LD, COL0, W, L, V_, 0, 0, EOS, B, O, None, stream) == 0
    assert lib.care_cider_score(None, LD, COL0, W, L, V_, 4, 0, EOS, B, O, None, stream) == EINVAL
    assert lib.care_cider_score(T, LD, COL0, W, None, V_, 4, 0, EOS, B, O, None, stream) == EINVAL
    assert lib.care_cider_score(T, LD, COL0, W, L, None, 4, 0, EOS, B, O, None, stream) == EINVAL
    assert lib.care_cider_score(T, LD, COL0, W, L, V_, 4, 0, EOS, None, O, None, stream) == EINVAL
    assert lib.care_cider_score(T, LD, COL0, W, L, V_, 4, 0, EOS, B, None, None, stream) == EINVAL
    assert lib.care_cider_score(T, LD, COL0, W, L, V_, -1, 0, EOS, B, O, None, stream) == EINVAL
    assert lib.care_cider_score(T, W, COL0, W, L, V_, 4, 0, EOS, B, O, None, stream) == EINVAL, "ld below the caption width"
    assert lib.care_cider_score(T, LD, COL0, W + 1, L, V_, 4, 0, EOS, B, O, None, stream) == EINVAL, "more than 64 tokens"
    keep_ptr = bank.desc.ref_w
    bank.desc.ref_w = keep_ptr + 4
    assert lib.care_cider_score(T, LD, COL0, W, L, V_, 4, 0, EOS, B, O, None, stream) == EALIGN
    bank.desc.ref_w = keep_ptr
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all()), "a refused call and an empty batch write nothing"


# ------------------------------------------------------------------------------------------------ care_reward_advantage
def _advantage(reward, baseline):
    from care_amd import _lib

    B, n = reward.shape
    w_adv, adv = _guarded(B * n)
    w_st, stats = _guarded(2, torch.float64)
    r_d = reward.to(DEV)
    b_d = None if baseline is None else baseline.to(DEV)
    _lib.call("care_reward_advantage", r_d.data_ptr(), None if b_d is None else b_d.data_ptr(), B, n, adv.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert _intact(w_adv, B * n) and _intact(w_st, 2)
    return adv.cpu().view(B, n), stats.cpu()


@pytest.mark.parametrize("B,n", [(1, 1), (1, 2), (3, 5), (130, 5)])
def test_reward_advantage_has_the_bits_of_the_fp32_expression(B, n):
    g = _gen(B, n)
    reward = (torch.rand(B, n, generator=g) * 10).float()
    reward[0, 0] = 0.0
    baseline = (torch.rand(B, generator=g) * 10).float()
    adv, stats = _advantage(reward, baseline)
    assert adv.numpy().tobytes() == (reward - baseline.view(B, 1)).numpy().tobytes()
    for got, want in ((stats[0], reward.double().mean()), (stats[1], baseline.double().mean())):
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    if n == 1:
        return
    adv, stats = _advantage(reward, None)
    s = reward[:, 0]
    for j in range(1, n):
        s = s + reward[:, j]
    base = (s.view(B, 1) - reward) / torch.tensor(float(n - 1), dtype=torch.float32)
    assert adv.numpy().tobytes() == (reward - base).numpy().tobytes()
    for got, want in ((stats[0], reward.double().mean()), (stats[1], base.double().mean())):
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


def test_reward_advantage_refusals():
    from care_amd import _lib
    from care_amd.reward import reward_advantage

    lib, stream = _lib.load(), _lib.stream_ptr()
    r = torch.ones(3, 1, device=DEV)
    w_adv, adv = _guarded(3)
    w_st, stats = _guarded(2, torch.float64)
    assert lib.care_reward_advantage(r.data_ptr(), None, 3, 1, adv.data_ptr(), stats.data_ptr(), stream) == EINVAL
    assert lib.care_reward_advantage(r.data_ptr(), r.data_ptr(), 3, 1, adv.data_ptr(), stats.data_ptr() + 4, stream) == EALIGN
    assert lib.care_reward_advantage(None, r.data_ptr(), 3, 1, adv.data_ptr(), stats.data_ptr(), stream) == EINVAL
    torch.cuda.synchronize()
    assert bool((w_adv == CANARY).all()) and bool((w_st == CANARY).all())
    with pytest.raises(ValueError, match="n_samples >= 2"):
        reward_advantage(r)


# ------------------------------------------------------------------------------------------------ the weighted log-likelihood
G_UP = 0.37   # the upstream gradient (a device scalar)


def _loss_case(V, S, P, key=0, all_pad=False, ones=False):
    """logits [S, P + 1, V] (the last position is dropped by the addressing), labels [S, P] with PAD tails, advantages [S] of
    mixed sign with one exact zero (S >= 3) - and one row with a logit spread of 1e4."""
    g = _gen(V, S, P, key)
    logits = torch.randn(S, P + 1, V, generator=g) * 3
    logits[S // 2, 0] = torch.randn(V, generator=g) * 1.5e3          # max - min of about 1e4
    labels = torch.randint(1, V, (S, P), generator=g)
    for s in range(S):
        labels[s, P - (s * 3) % (P + 1) // 2:] = 0                      # PAD tails of several lengths
    labels[S // 2, 0] = max(1, int(labels[S // 2, 0]))
    if all_pad:
        labels.zero_()
    adv = torch.randn(S, generator=g) * 2
    if S >= 3:
        adv[S - 1] = 0.0
    if ones:
        adv.fill_(1.0)
    return logits, labels, adv


def _loss_reference(logits, labels, adv, dt):
    """(loss, per-caption sum logp, dlogits for the upstream gradient G_UP) of the formula in dtype `dt`, by torch on the CPU."""
    x = logits[:, :labels.shape[1]].detach().clone().to(dt).requires_grad_(True)
    live = labels > 0
    logp = torch.log_softmax(x, dim=-1).gather(2, labels.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    logp = torch.where(live, logp, torch.zeros((), dtype=dt))
    n_live = live.sum()
    loss = -(adv.to(dt).view(-1, 1) * logp).sum() / n_live.clamp_min(1).to(dt)
    (loss * torch.tensor(G_UP, dtype=torch.float32).to(dt)).backward()
    return loss.detach(), logp.detach().sum(dim=1), x.grad


def _run_loss(logits, labels, adv, ld, drop_last, with_bwd=True):
    """The two entry points on a [S, rows_in_memory, ld] buffer (NaN in the padding and, with drop_last, in the dropped last
    position); every output guarded.  Returns a dict of CPU tensors."""
    from care_amd import _lib

    S, P = labels.shape
    V = logits.shape[2]
    tl = P + 1 if drop_last else P
    buf = torch.full((S, tl, ld), float("nan"), device=DEV)
    buf[:, :P, :V] = logits[:, :P].to(DEV)
    lab = labels.to(torch.int32).to(DEV).contiguous()
    a = adv.to(DEV)
    rows = S * P
    guards = {k: _guarded(rows) for k in ("rmax", "lsum", "logp")}
    guards["seq"] = _guarded(S)
    guards["loss"] = _guarded(1)
    w_tot, totals = _guarded(2, torch.float64)
    w_acc, acc = _guarded(2, torch.float64, fill=1.0)
    _lib.call("care_reward_loss_fwd", buf.data_ptr(), ld, tl * ld, P, V, lab.data_ptr(), a.data_ptr(), guards["rmax"][1].data_ptr(),
              guards["lsum"][1].data_ptr(), guards["logp"][1].data_ptr(), totals.data_ptr(), guards["loss"][1].data_ptr(),
              guards["seq"][1].data_ptr(), acc.data_ptr(), rows)
    out = {}
    if with_bwd:
        g = torch.tensor([G_UP], device=DEV)
        d = torch.full((GAP + S * tl * ld + GAP,), CANARY, device=DEV)
        dv = d[GAP:GAP + S * tl * ld].view(S, tl, ld)
        _lib.call("care_reward_loss_bwd", buf.data_ptr(), ld, tl * ld, P, V, lab.data_ptr(), a.data_ptr(), guards["rmax"][1].data_ptr(),
                  guards["lsum"][1].data_ptr(), totals.data_ptr(), g.data_ptr(), dv.data_ptr(), ld, tl * ld, tl, rows)
        torch.cuda.synchronize()
        assert bool((d[:GAP] == CANARY).all()) and bool((d[-GAP:] == CANARY).all()) and bool((dv[:, :, V:] == CANARY).all()), \
            "dlogits written outside its rows"
        out["dlogits"] = dv[:, :, :V].cpu()
    torch.cuda.synchronize()
    for k, (whole, view) in guards.items():
        assert _intact(whole, view.numel()), k
        out[k] = view.cpu().clone()
    assert _intact(w_tot, 2) and bool((w_acc[:GAP] == 1.0).all()) and bool((w_acc[GAP + 2:] == 1.0).all())
    out["totals"], out["acc"] = totals.cpu().clone(), acc.cpu().clone()
    return out


@pytest.mark.parametrize("S,P", [(1, 1), (3, 5), (7, 29)])
@pytest.mark.parametrize("V", [5, 130, 10547, 20011])
def test_reward_loss_against_float64(V, S, P):
    worst = _Worst("care_reward_loss V {} [{}, {}]".format(V, S, P))
    logits, labels, adv = _loss_case(V, S, P)
    ref_loss, ref_seq, ref_grad = _loss_reference(logits, labels, adv, torch.float64)
    yard_loss, yard_seq, yard_grad = _loss_reference(logits, labels, adv, torch.float32)
    live = labels > 0
    for ld, drop_last in ((V, False), (V + 5, False), (V, True), (V + 3, True)):
        tag = "ld {} drop_last {}".format(ld, drop_last)
        out = _run_loss(logits, labels, adv, ld, drop_last)
        _check(worst, tag + " loss", out["loss"].view(()), ref_loss, yard_loss)
        _check(worst, tag + " seq_logp", out["seq"], ref_seq, yard_seq)
        grad = out["dlogits"]
        _check(worst, tag + " dlogits", grad[:, :P], ref_grad, yard_grad)
        assert int(out["totals"][1]) == int(live.sum()) and float(out["acc"][1]) == 1.0 + int(live.sum())
        assert float(out["acc"][0]) == 1.0 + float(out["loss"]), "acc accumulates"
        dead = ~live | (adv == 0).view(-1, 1)
        assert bool((grad[:, :P][dead] == 0).all()), "dead rows and rows of a zero advantage are exactly 0"
        if drop_last:
            assert bool((grad[:, P] == 0).all()), "the dropped last position is zero-filled"
        assert bool((out["logp"].view(S, P)[~live] == 0).all())
        again = _run_loss(logits, labels, adv, ld, drop_last)
        for k in ("loss", "seq", "logp", "dlogits", "totals"):
            assert again[k].numpy().tobytes() == out[k].numpy().tobytes(), (k, "two runs must give the same bits")
    worst.report()


def test_reward_loss_nan_in_unread_rows_and_the_all_pad_batch():
    V, S, P = 10547, 3, 5
    logits, labels, adv = _loss_case(V, S, P, key=1)
    live = labels > 0
    ref_loss, _, ref_grad = _loss_reference(logits, labels, adv, torch.float64)
    yard_loss, _, yard_grad = _loss_reference(logits, labels, adv, torch.float32)
    poisoned = logits.clone()
    poisoned[:, :P][~live] = float("nan")         # dead rows
    out = _run_loss(poisoned, labels, adv, V, True)
    worst = _Worst("NaN in dead rows")
    _check(worst, "loss", out["loss"].view(()), ref_loss, yard_loss)
    _check(worst, "dlogits", out["dlogits"][:, :P], ref_grad, yard_grad)
    poisoned[S - 1] = float("nan")                 # ... and the sequence whose advantage is exactly 0
    assert float(adv[S - 1]) == 0.0
    out = _run_loss(poisoned, labels, adv, V, True)
    assert bool((out["dlogits"][S - 1] == 0).all()) and bool(torch.isfinite(out["dlogits"]).all())
    _check(worst, "dlogits, NaN under a zero advantage", out["dlogits"][:, :P], ref_grad, yard_grad)
    _check(worst, "loss, NaN under a zero advantage", out["loss"].view(()), ref_loss, yard_loss)
    # all PAD: loss 0 and a zero gradient, not NaN
    logits, labels, adv = _loss_case(V, S, P, key=2, all_pad=True)
    out = _run_loss(logits, labels, adv, V + 5, False)
    assert float(out["loss"]) == 0.0 and float(out["totals"][1]) == 0.0 and bool((out["dlogits"] == 0).all())
    assert bool((out["seq"] == 0).all())


def test_reward_loss_with_unit_advantages_is_the_language_loss():
    """All advantages 1: the loss is care_lang_loss_fwd's sums[1] / counts[1] at eps = 0 - both under the yardstick rule."""
    from care_amd import _lib

    V, S, P = 10547, 7, 29
    logits, labels, adv = _loss_case(V, S, P, key=3, ones=True)
    ref_loss, _, _ = _loss_reference(logits, labels, adv, torch.float64)
    yard_loss, _, _ = _loss_reference(logits, labels, adv, torch.float32)
    ours = _run_loss(logits, labels, adv, V, True, with_bwd=False)["loss"].view(())
    buf = logits.to(DEV).contiguous()
    lab = labels.to(torch.int32).to(DEV).contiguous()
    rows = S * P
    st = torch.empty(5, rows, device=DEV)
    pred, sums, counts = torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty(2, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV)
    _lib.call("care_lang_loss_fwd", buf.data_ptr(), V, (P + 1) * V, P, V, lab.data_ptr(), 0.0, st[0].data_ptr(), st[1].data_ptr(),
              st[2].data_ptr(), st[3].data_ptr(), pred.data_ptr(), st[4].data_ptr(), sums.data_ptr(), counts.data_ptr(), None, rows)
    lang = (sums[1] / counts[1]).cpu()
    worst = _Worst("unit advantages")
    _check(worst, "care_reward_loss_fwd", ours, ref_loss, yard_loss)
    _check(worst, "care_lang_loss_fwd", lang, ref_loss, yard_loss)
    print("weighted", float(ours), "language", float(lang), "float64", float(ref_loss))
    worst.report()


@pytest.mark.parametrize("V", [3, 5, 130, 4100, 12290, 16390])
def test_reward_and_language_forward_share_one_row_sweep(V):
    """care_reward_loss_fwd and care_lang_loss_fwd (eps = 0) on one buffer and one set of labels write the same BITS of rmax,
    lsum and logp: both run the sweeps of csrc/vocab_row.h - one order of every sum in every register form, and the maximum as
    a value does not depend on how ties are ordered.  V = 3 and 5 have head >= V or no float4 at some phases, 4100 puts the
    two entry points on different register forms (8 float4s a lane against 12), 12290 gives 16 against re-reading, 16390
    re-reading in both; ld = V .. V + 3 starts consecutive rows at all four 4-byte phases.  One row has a spread of 1e4,
    the labels have PAD tails, the dropped last position and the padding of a row are NaN."""
    from care_amd import _lib

    S, P = 2, 3
    rows = S * P
    logits, labels, adv = _loss_case(V, S, P, key=5)
    live = (labels > 0).view(-1)
    assert 0 < int(live.sum()) < rows, "live rows and PAD tails"
    lab = labels.to(torch.int32).to(DEV).contiguous()
    a = adv.to(DEV)
    phases = set()
    for ld in range(V, V + 4):
        buf = torch.full((S, P + 1, ld), float("nan"), device=DEV)
        buf[:, :P, :V] = logits[:, :P].to(DEV)
        phases |= {(buf.data_ptr() // 4 + (s * (P + 1) + p) * ld) % 4 for s in range(S) for p in range(P)}
        rw = {k: _guarded(rows) for k in ("rmax", "lsum", "logp", "seq", "loss")}
        lg = {k: _guarded(rows) for k in ("lse", "rmax", "lsum", "logp", "row_loss")}
        w_tot, totals = _guarded(2, torch.float64)
        pred, sums = torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty(2, device=DEV)
        counts = torch.empty(3, dtype=torch.int32, device=DEV)
        _lib.call("care_reward_loss_fwd", buf.data_ptr(), ld, (P + 1) * ld, P, V, lab.data_ptr(), a.data_ptr(), rw["rmax"][1].data_ptr(),
                  rw["lsum"][1].data_ptr(), rw["logp"][1].data_ptr(), totals.data_ptr(), rw["loss"][1].data_ptr(),
                  rw["seq"][1].data_ptr(), None, rows)
        _lib.call("care_lang_loss_fwd", buf.data_ptr(), ld, (P + 1) * ld, P, V, lab.data_ptr(), 0.0, lg["lse"][1].data_ptr(),
                  lg["rmax"][1].data_ptr(), lg["lsum"][1].data_ptr(), lg["logp"][1].data_ptr(), pred.data_ptr(),
                  lg["row_loss"][1].data_ptr(), sums.data_ptr(), counts.data_ptr(), None, rows)
        torch.cuda.synchronize()
        for k in ("rmax", "lsum", "logp"):
            assert _intact(rw[k][0], rows) and _intact(lg[k][0], rows), (ld, k)
            ours, theirs = rw[k][1].cpu(), lg[k][1].cpu()
            print("V", V, "ld", ld, k, "differing rows", int((ours.view(torch.int32) != theirs.view(torch.int32)).sum()), "of", rows)
            assert ours.numpy().tobytes() == theirs.numpy().tobytes(), (ld, k, ours.tolist(), theirs.tolist())
        got = rw["rmax"][1].cpu()
        assert bool((got[live] == logits[:, :P].reshape(rows, V)[live].max(dim=1).values).all()), "the maximum of a row is exact"
        assert bool((got[~live] == 0).all()) and bool(torch.isfinite(rw["logp"][1]).all())
    assert phases == {0, 1, 2, 3}


def test_self_critical_loss_under_autograd_without_a_synchronisation():
    from care_amd import self_critical_loss

    V, S, P = 10547, 3, 5
    logits, labels, adv = _loss_case(V, S, P, key=4)
    ref_loss, ref_seq, ref_grad = _loss_reference(logits, labels, adv, torch.float64)
    yard_loss, yard_seq, yard_grad = _loss_reference(logits, labels, adv, torch.float32)
    x = logits.to(DEV).requires_grad_(True)          # [S, P + 1, V]: the last position is skipped in place
    lab, a = labels.to(DEV), adv.to(DEV)
    up = torch.tensor(G_UP, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, seq, totals = self_critical_loss(x, lab, a, return_aux=True)
        (loss * up).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and x.grad.shape == x.shape
    worst = _Worst("self_critical_loss")
    _check(worst, "loss", loss, ref_loss, yard_loss)
    _check(worst, "seq_logp", seq, ref_seq, yard_seq)
    _check(worst, "dlogits", x.grad[:, :P], ref_grad, yard_grad)
    assert bool((x.grad[:, P] == 0).all()) and float(totals[1]) == float((labels > 0).sum())
    with pytest.raises(ValueError, match="advantages"):
        self_critical_loss(x, lab, a[:2])
    with pytest.raises(TypeError, match="fp32"):
        self_critical_loss(x.double(), lab, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        self_critical_loss(x, lab.cpu(), a)

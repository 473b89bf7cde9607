"""GPU: the training criteria (csrc/loss.hip through the C ABI, and care_amd/criterion.py on top).

Kernels are judged like tests/test_gpu_backward_kernels.py judges the other training kernels (its `_check`): the reference is
plain torch in float64 on the CPU (tests/crit_reference.py, pinned to the genuine reference by tests/test_criterion_cpu.py),
the yardstick is the same formula evaluated by torch in fp32 on the same inputs, and every element's error must be at most
    4 x yardstick + 2^-22 x scale.
Logits and gradients live in NaN-filled buffers with a spare row on each side and, for ld = V + 3, spare columns: an over-read
shows as a NaN in a result, an over-write as a missing NaN.  Rows whose label is PAD hold NaN logits too - they must not be read.

Which V reaches which form of care_lang_loss_fwd: V <= 4096 -> 4 float4 per lane in registers (5, 100, 130, 2003); <= 12288 -> 12
(10547); <= 16384 -> 16 (16384, the largest one-read V); above -> the re-reading form (20011).  ld = V = 10547 and ld = V + 3
put consecutive rows at all four 4-byte phases; the gradient buffer of the padded cases has ANOTHER leading dimension (V + 1), so
the backward's loads and stores are at different phases (its scalar-load path), in the dense cases at the same one (float4 loads).
"""
import json
import math

import numpy as np
import pytest
import torch

from crit_reference import (bce_rows, crit_cases, criterion_batches, criterion_opt, info_of_batches, lang_counts, lang_rows,
                            lang_step, load_case, total_loss, bce_step)
from test_gpu_backward_kernels import _Worst, _check, _gen

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
G_UP = 0.37   # the upstream gradient handed to the backward kernels (a device scalar)


def _call(name, *args):
    from care_amd import _lib

    _lib.call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -77, device=DEV, dtype=dtype)
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _guarded(t, ld, dead_rows=None):
    """`t` [rows, V] (CPU) inside a NaN-filled device buffer [rows + 2, ld], one spare row before and after; the rows listed in
    `dead_rows` stay NaN as well.  Returns (buffer, view of the rows)."""
    rows, V = t.shape
    buf = _nan(rows + 2, ld)
    view = buf[1: rows + 1, :V]
    view.copy_(t)
    if dead_rows is not None and len(dead_rows):
        view[dead_rows] = NAN
    return buf, view


def _only_rows_written(buf, rows, V):
    assert not torch.isnan(buf[1: rows + 1, :V]).any(), "NaN left inside"
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[rows + 1:]).all() and torch.isnan(buf[:, V:]).all(), "written outside"


class _Fwd:
    """One care_lang_loss_fwd call on [n_seq, seq_rows, V] logits (row stride ld) with labels [n_seq, t]; outputs in guarded
    arrays."""

    def __init__(self, x, labels, eps, ld, seq_rows=None, acc=None):
        n_seq, t = labels.shape
        self.V = V = x.shape[-1]
        self.seq_rows = seq_rows = seq_rows or t
        self.n_seq, self.t, self.ld, self.eps = n_seq, t, ld, eps
        flat = x.reshape(n_seq * seq_rows, V)
        lab_full = torch.zeros(n_seq, seq_rows, dtype=torch.int64)
        lab_full[:, :t] = labels
        dead = ((lab_full <= 0) | (lab_full >= V)).reshape(-1).nonzero().squeeze(1)
        self.buf, self.xd = _guarded(flat, ld, dead)
        self.lab = labels.to(DEV, torch.int32).contiguous()
        rows = n_seq * t
        self.rows = rows
        self.out = _nan(5, rows + 2)                       # lse, logp, row_loss, max, log sum exp(x - max) at [1 : rows + 1]
        self.pred = _nan(rows + 2, dtype=torch.int32)
        self.sums = _nan(4)
        self.counts = _nan(5, dtype=torch.int32)
        self.acc = acc
        self.run()

    def run(self):
        _call("care_lang_loss_fwd", _p(self.xd), self.ld, self.seq_rows * self.ld, self.t, self.V, _p(self.lab), self.eps,
              _p(self.out[0, 1:]), _p(self.out[3, 1:]), _p(self.out[4, 1:]), _p(self.out[1, 1:]), _p(self.pred[1:]), _p(self.out[2, 1:]), _p(self.sums), _p(self.counts),
              _p(self.acc), self.rows)
        torch.cuda.synchronize()
        r = self.rows
        assert torch.isnan(self.out[:, 0]).all() and torch.isnan(self.out[:, r + 1]).all() and not torch.isnan(self.out[:, 1: r + 1]).any()
        assert int(self.pred[0]) == -77 and int(self.pred[r + 1]) == -77
        assert torch.isnan(self.sums[2:]).all() and (self.counts[3:] == -77).all()
        self.lse, self.logp, self.row_loss = (self.out[i, 1: r + 1].cpu() for i in range(3))
        self.pred_rows = self.pred[1: r + 1].cpu().long()

    def bwd(self, ldd):
        """care_lang_loss_bwd into a guarded NaN buffer of leading dimension ldd; returns dlogits [n_seq * seq_rows, V] (CPU)."""
        total = self.n_seq * self.seq_rows
        dbuf = _nan(total + 2, ldd)
        g = torch.tensor([G_UP], device=DEV)
        _call("care_lang_loss_bwd", _p(self.xd), self.ld, self.seq_rows * self.ld, self.t, self.V, _p(self.lab), _p(self.out[3, 1:]),
              _p(self.out[4, 1:]), self.eps, _p(g), _p(dbuf[1]), ldd, self.seq_rows * ldd, self.seq_rows, self.rows)
        torch.cuda.synchronize()
        _only_rows_written(dbuf, total, self.V)
        self.dbuf = dbuf
        return dbuf[1: total + 1, : self.V].cpu()


def _reference(x, labels, eps, dt):
    """(lse, logp, row_loss (0 on dead rows), step sum, d (G_UP * step) / d logits) of the restated criterion in dtype dt."""
    xx = x.detach().clone().to(dt).requires_grad_(True)
    row, logp, _, lse = lang_rows(xx, labels, eps)
    live = labels.ne(0).to(dt)
    step = (row * live).sum()
    (step * G_UP).backward()
    return (lse * live).detach().reshape(-1), (logp * live).detach().reshape(-1), (row * live).detach().reshape(-1), step.detach(), xx.grad


def _lang_case(worst, V, rows, eps, padded, special=None):
    g = _gen(V, rows, int(eps * 10), padded, 7)
    x = torch.randn(1, rows, V, generator=g) * 3.0
    labels = torch.randint(1, V, (1, rows), generator=g) if V > 1 else torch.zeros(1, rows, dtype=torch.int64)
    if rows >= 5:
        labels[0, 1] = 0
        labels[0, rows - 2] = 0                             # PAD rows, one next to the end
    if special == "spread":
        x[0, 0] = (torch.rand(V, generator=g) - 0.5) * 1e4  # a row with a logit spread of 1e4
        labels[0, 0] = max(1, V // 3)
    ld = V + 3 if padded else V
    f = _Fwd(x, labels, eps, ld)
    what = "lang V {} rows {} eps {} ld {} {}".format(V, rows, eps, ld, special or "")
    lse64, logp64, row64, step64, d64 = _reference(x, labels, eps, torch.float64)
    lse32, logp32, row32, step32, d32 = _reference(x, labels, eps, torch.float32)
    _check(worst, what + " lse", f.lse, lse64, lse32)
    _check(worst, what + " logp", f.logp, logp64, logp32)
    _check(worst, what + " row_loss", f.row_loss, row64, row32)
    _check(worst, what + " sum", f.sums[0].cpu(), step64, step32, bound=row64.abs().sum())
    live = labels.reshape(-1).ne(0)
    nlogp64, nlogp32 = -(logp64.sum()), -(logp32.sum())
    _check(worst, what + " sum -logp", f.sums[1].cpu(), nlogp64, nlogp32, bound=logp64.abs().sum())
    want_pred = x[0].argmax(-1)
    assert torch.equal(f.pred_rows[live], want_pred[live]), what
    dead = ~live
    for arr in (f.lse, f.logp, f.row_loss):
        assert float(arr[dead].abs().sum()) == 0.0 if dead.any() else True, what
    assert int(f.pred_rows[dead].abs().sum()) == 0 if dead.any() else True, what
    assert f.counts[:3].tolist() == [int((want_pred == labels[0])[live].sum()), int(live.sum()), 0], what
    d = f.bwd(V + 1 if padded else V)
    _check(worst, what + " dlogits", d, d64[0], d32[0])
    if dead.any():
        assert float(d[dead].abs().max()) == 0.0, what      # exactly zero, and finite although those logits are NaN


@pytest.mark.parametrize("V", [5, 100, 130, 2003, 10547, 16384, 20011])
def test_lang_loss_kernels_against_float64(V):
    """lse, logp, row_loss, arg-max, the ordered sums and dlogits for rows 1 / 5 / 58, eps 0 / 0.1, dense and padded leading
    dimensions, and a row with a logit spread of 1e4."""
    worst = _Worst("care_lang_loss V={}".format(V))
    for rows in (1, 5, 58):
        for eps in (0.0, 0.1):
            for padded in (False, True):
                _lang_case(worst, V, rows, eps, padded)
    _lang_case(worst, V, 5, 0.1, True, special="spread")
    _lang_case(worst, V, 5, 0.0, False, special="spread")
    worst.report()


@pytest.mark.parametrize("V", [130, 10547, 20011])
def test_lang_loss_argmax_ties_take_the_lower_index(V):
    """Two equal maxima - in the peeled head and the tail, in different lanes, in different waves, next to each other: pred is the
    lower column (as care_score_logits), for every 4-byte phase of the row (ld = V + 3: four rows, four phases)."""
    far = (256, 256 + 4 * 256) if V > 2000 else (64, V - 3)   # the same lane's next float4 / another wave
    pairs = [(0, V - 1), (1, 2), (3, 4), (5, V // 2), (V // 2, V // 2 + 1), (V - 2, V - 1), far]
    rows = 4 * len(pairs)
    g = _gen(V, 99)
    x = torch.randn(1, rows, V, generator=g)
    for i in range(rows):
        a, b = pairs[i // 4]
        x[0, i, a] = x[0, i, b] = 9.0
    labels = torch.full((1, rows), 1, dtype=torch.int64)
    for ld in (V, V + 3):
        f = _Fwd(x, labels, 0.0, ld)
        assert f.pred_rows.tolist() == [min(pairs[i // 4]) for i in range(rows)], (V, ld)


@pytest.mark.parametrize("V", [100, 10547])
def test_lang_loss_all_pad_batch(V):
    """Every label PAD, every logit NaN: loss 0, the outputs 0, the gradient exactly 0 - nothing NaN."""
    labels = torch.zeros(2, 3, dtype=torch.int64)
    f = _Fwd(torch.randn(2, 3, V), labels, 0.1, V + 3)
    assert torch.isnan(f.xd).all()
    assert f.sums[:2].tolist() == [0.0, 0.0] and f.counts[:3].tolist() == [0, 0, 0]
    assert float(f.out[:, 1: 7].abs().sum()) == 0.0 and int(f.pred[1: 7].abs().sum()) == 0
    d = f.bwd(V + 1)
    assert float(d.abs().sum()) == 0.0


@pytest.mark.parametrize("V", [131, 10547])
def test_lang_loss_drops_the_last_position_in_place(V):
    """logits [N, t + 1, V] against labels [N, t] (crit_lang.py:49-50) without a copy: seq_stride = (t + 1) ld; the gradient has
    the logits' shape, its last position zero-filled.  The dropped position's logits are NaN: it is not read."""
    worst = _Worst("care_lang_loss drop-last V={}".format(V))
    N, t = 3, 4
    g = _gen(V, N, t)
    x = torch.randn(N, t + 1, V, generator=g) * 2.0
    labels = torch.randint(1, V, (N, t), generator=g)
    labels[1, 2:] = 0
    for eps, padded in ((0.0, False), (0.1, True)):
        f = _Fwd(x, labels, eps, V + 3 if padded else V, seq_rows=t + 1)
        lse64, logp64, row64, step64, d64 = _reference(x, labels, eps, torch.float64)
        lse32, logp32, row32, step32, d32 = _reference(x, labels, eps, torch.float32)
        what = "drop-last V {} eps {}".format(V, eps)
        _check(worst, what + " row_loss", f.row_loss, row64, row32)
        _check(worst, what + " logp", f.logp, logp64, logp32)
        _check(worst, what + " sum", f.sums[0].cpu(), step64, step32, bound=row64.abs().sum())
        d = f.bwd(V + 1 if padded else V).view(N, t + 1, V)
        _check(worst, what + " dlogits", d, d64, d32)
        assert float(d[:, t].abs().max()) == 0.0 and float(d64[:, t].abs().max()) == 0.0
    worst.report()


def test_lang_loss_bad_labels_are_counted_not_dereferenced():
    """Labels V and -1 on rows >= 1 of the guarded buffer: the rows contribute nothing (their logits are NaN: not read), n_bad
    counts them, the gradient rows are zero; the class raises at get_loss_info() / get_info(), naming the count."""
    from care_amd import LanguageGeneration

    V, rows = 2003, 6
    g = _gen(V, rows, 5)
    x = torch.randn(1, rows, V, generator=g)
    labels = torch.randint(1, V, (1, rows), generator=g)
    good = labels.clone()
    labels[0, 1], labels[0, 4] = V, -1
    good[0, 1] = good[0, 4] = 0
    acc = torch.zeros(5, device=DEV, dtype=torch.float64)
    f = _Fwd(x, labels, 0.1, V + 3, acc=acc)
    ref = _Fwd(x, good, 0.1, V + 3)
    assert f.counts[:3].tolist() == [int(ref.counts[0]), 4, 2] and ref.counts[:3].tolist()[1:] == [4, 0]
    assert torch.equal(f.out[:, 1: rows + 1], ref.out[:, 1: rows + 1]) and torch.equal(f.sums[:2], ref.sums[:2])   # the bits of PAD in their place
    d = f.bwd(V + 1)
    assert float(d[[1, 4]].abs().max()) == 0.0 and torch.equal(d, ref.bwd(V + 1))
    assert acc.tolist()[2:] == [float(ref.counts[0]), 4.0, 2.0] and acc.tolist()[:2] == [float(f.sums[0]), float(f.sums[1])]
    lang = LanguageGeneration({"label_smoothing": 0.1})
    lang({"logits": x.to(DEV), "labels": labels.to(DEV)})
    with pytest.raises(ValueError, match="2 label"):
        lang.get_info()


def test_lang_loss_is_bitwise_repeatable_and_accumulates():
    V, rows = 10547, 58
    g = _gen(V, rows, 3)
    x = torch.randn(2, rows // 2, V, generator=g) * 3.0
    labels = torch.randint(0, V, (2, rows // 2), generator=g)
    labels[:, 20:] = 0
    acc = torch.zeros(5, device=DEV, dtype=torch.float64)
    f = _Fwd(x, labels, 0.1, V, acc=acc)
    first = (f.out.clone(), f.pred.clone(), f.sums.clone(), f.counts.clone(), f.bwd(V).clone())
    f.out.fill_(NAN)
    f.run()
    second = (f.out, f.pred, f.sums, f.counts, f.bwd(V))
    for a, b in zip(first, second):
        assert torch.equal(torch.nan_to_num(a.float(), nan=-5.0), torch.nan_to_num(b.float(), nan=-5.0))
    # the recorder doubles: two calls added, in stream order
    want = [2.0 * float(f.sums[0]), 2.0 * float(f.sums[1]), 2.0 * int(f.counts[0]), 2.0 * int(f.counts[1]), 0.0]
    assert acc.tolist() == want


@pytest.mark.parametrize("K", [5, 64, 500, 1000])
def test_noisy_or_bce_kernels_against_float64(K):
    """row loss, denominator, the ordered sum and dpreds for 1 / 5 / 58 clips: probabilities on both sides of the clamp and on
    its ends, labels wider than the predictions (positives in the unused columns), a clip with no positive; padded leading
    dimensions, each different."""
    worst = _Worst("care_noisy_or_bce K={}".format(K))
    for B in (1, 5, 58):
        g = _gen(K, B, 1)
        preds = torch.rand(B, K, generator=g)
        preds[:, ::5] *= 0.02
        preds[:, 1::5] = 1.0 - preds[:, 1::5] * 0.02
        preds[:, 2], preds[:, 3] = 0.01, 0.99
        labels = (torch.rand(B, K + 9, generator=g) > 0.8).float()
        labels[:, K:] = 1.0
        if B > 1:
            labels[1, :K] = 0.0

        def run(dt):
            p = preds.detach().clone().to(dt).requires_grad_(True)
            row, den = bce_rows(p, labels)
            (row.sum() * G_UP).backward()
            return row.detach(), den.detach(), row.sum().detach(), p.grad

        row64, den64, sum64, d64 = run(torch.float64)
        row32, den32, sum32, d32 = run(torch.float32)
        ldp, ldl, ldd = K + 3, K + 9, K + 5
        pbuf, pd = _guarded(preds, ldp)
        lbuf = _nan(B + 2, ldl)
        ld_ = lbuf[1: B + 1]
        ld_.copy_(labels)
        out = _nan(2, B + 2)
        sums = _nan(3)
        acc = torch.full((2,), 1.5, device=DEV, dtype=torch.float64)
        _call("care_noisy_or_bce_fwd", _p(pd), ldp, _p(ld_), ldl, _p(out[0, 1:]), _p(out[1, 1:]), _p(sums), _p(acc), B, K)
        dbuf = _nan(B + 2, ldd)
        gdev = torch.tensor([G_UP], device=DEV)
        _call("care_noisy_or_bce_bwd", _p(pd), ldp, _p(ld_), ldl, _p(out[1, 1:]), _p(gdev), _p(dbuf[1]), ldd, B, K)
        torch.cuda.synchronize()
        what = "bce B {} K {}".format(B, K)
        assert torch.isnan(out[:, 0]).all() and torch.isnan(out[:, B + 1]).all() and torch.isnan(sums[1:]).all(), what
        _only_rows_written(dbuf, B, K)
        _check(worst, what + " row_loss", out[0, 1: B + 1], row64, row32)
        assert torch.equal(out[1, 1: B + 1].cpu().double(), den64), what
        _check(worst, what + " sum", sums[0].cpu(), sum64, sum32, bound=row64.abs().sum())
        assert acc.tolist() == [1.5 + float(sums[0]), 1.5], what
        _check(worst, what + " dpreds", dbuf[1: B + 1, :K], d64, d32)
        outside = (preds < 0.01) | (preds > 0.99)
        assert float(dbuf[1: B + 1, :K].cpu()[outside].abs().max()) == 0.0, what
        assert float(dbuf[1: B + 1, 2:4].abs().min()) > 0.0, what          # on the clamp's ends the gradient passes
    worst.report()


# ================================================================================ care_amd.criterion on the recorded reference
def _vs_reference(worst, what, got, ref64, recorded):
    """The same bar with the RECORDED reference (the genuine criterion in fp32, tests/golden/crit) as the fp32 yardstick."""
    _check(worst, what, torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref64, dtype=torch.float64),
           torch.as_tensor(recorded, dtype=torch.float64))


@pytest.mark.parametrize("name", ["lang_v131", "lang_v131_drop_last", "lang_v2003"])
def test_language_generation_reproduces_the_recorded_reference(name):
    from care_amd import LanguageGeneration

    worst = _Worst("LanguageGeneration " + name)
    z = load_case(name)
    labels = torch.from_numpy(z["labels"])
    for i, eps in enumerate(z["eps"].tolist()):
        x64 = torch.from_numpy(z["logits"]).double().requires_grad_(True)
        den = float(x64.shape[0])
        loss64 = lang_step(x64, labels, eps) / den
        loss64.backward()
        crit = LanguageGeneration({"label_smoothing": eps})
        crit.reset_recorder()
        x = torch.from_numpy(z["logits"]).to(DEV).requires_grad_(True)
        loss, got_den = crit({"logits": x, "labels": labels.to(DEV)})
        loss.backward()
        assert got_den == den == float(z["denominator"][i])
        _vs_reference(worst, name + " loss", loss.detach().cpu(), loss64.detach(), z["loss"][i])
        _vs_reference(worst, name + " dlogits", x.grad.cpu(), x64.grad, z["dlogits"][i])
        names, info = crit.get_info()
        hits, words, nlogp = lang_counts(x64.detach(), labels)
        assert names == ["Word Acc0", "Perplexity"] and info[0] == z["info"][i][0] == hits / words
        _vs_reference(worst, name + " Perplexity", info[1], math.exp(nlogp / words), z["info"][i][1])
        assert torch.equal(crit.last_pred.cpu().long()[labels.ne(0)], lang_rows(x64.detach(), labels, eps)[2][labels.ne(0)])
    worst.report()


@pytest.mark.parametrize("name", ["attr_b3", "attr_b3_no_positive"])
def test_noisy_or_mil_reproduces_the_recorded_reference(name):
    from care_amd import NoisyOrMIL

    worst = _Worst("NoisyOrMIL " + name)
    z = load_case(name)
    labels = torch.from_numpy(z["labels_attr"])
    p64 = torch.from_numpy(z["preds_attr"]).double().requires_grad_(True)
    den = float(p64.shape[0])
    loss64 = bce_step(p64, labels) / den
    loss64.backward()
    crit = NoisyOrMIL({"calculate_mAP": True})
    crit.reset_recorder()
    p = torch.from_numpy(z["preds_attr"]).to(DEV).requires_grad_(True)
    loss, got_den = crit({"preds_attr": p, "avg_prob_attr": None, "labels_attr": labels})   # (labels on the host, as the reference allows)
    loss.backward()
    assert got_den == den == float(z["denominator"])
    _vs_reference(worst, name + " loss", loss.detach().cpu(), loss64.detach(), z["loss"])
    _vs_reference(worst, name + " dpreds", p.grad.cpu(), p64.grad, z["dpreds"])
    names, info = crit.get_info()
    assert names == json.loads(str(z["info_names"]))
    np.testing.assert_allclose(info, z["info"], rtol=1e-6, atol=0, equal_nan=True)   # ranks and counts: the same integers on both sides
    worst.report()


def test_criterion_reproduces_the_recorded_reference_over_two_batches():
    """get_criterion(['lang', 'attribute']) with scales 0.8 / 0.3 and label smoothing 0.1 over batches of 3 and 2 clips: each
    get_loss, the gradients, and get_loss_info() - the recorders' weighting by sample count - without a synchronisation in
    between."""
    from care_amd import get_criterion

    worst = _Worst("Criterion two batches")
    z = load_case("criterion_two_batches")
    opt = criterion_opt(z)
    crit = get_criterion(opt, override_opt={"calculate_mAP": True})
    assert crit.names == json.loads(str(z["names"])) and crit.scales == z["scales"].tolist()
    crit.reset_loss_recorder()
    batches = criterion_batches(z)
    for b, (logits, labels, preds, labels_attr) in enumerate(batches):
        x64, p64 = logits.double().requires_grad_(True), preds.double().requires_grad_(True)
        loss64 = total_loss({"logits": x64, "preds_attr": p64}, labels, labels_attr, opt["label_smoothing"], crit.scales)
        loss64.backward()
        x, p = logits.to(DEV).requires_grad_(True), preds.to(DEV).requires_grad_(True)
        loss = crit.get_loss({"logits": x, "labels": labels.to(DEV), "preds_attr": p, "avg_prob_attr": None,
                              "labels_attr": labels_attr.to(DEV)})
        loss.backward()
        _vs_reference(worst, "loss {}".format(b), loss.detach().cpu(), loss64.detach(), z["loss"][b])
        _vs_reference(worst, "dlogits {}".format(b), x.grad.cpu(), x64.grad, z["b%d_dlogits" % b])
        _vs_reference(worst, "dpreds {}".format(b), p.grad.cpu(), p64.grad, z["b%d_dpreds" % b])
    want = json.loads(str(z["info_json"]))
    want64 = info_of_batches(batches, opt["label_smoothing"])
    got = crit.get_loss_info()
    assert list(got) == list(want)
    assert got["Word Acc0"] == want["Word Acc0"]
    for k in want:
        _vs_reference(worst, k, got[k], want64[k], want[k])
    crit.reset_loss_recorder()
    assert crit.get_loss_info()["Lang Loss"] == 0 and crit.get_loss_info()["Perplexity"] == 1.0
    worst.report()


# ================================================================================ on the models
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
MODEL_FIXTURES = ["msrvtt_care_b2", "msrvtt_base_ami_eos_b4"]


def _train_model(name, **over):
    from conftest import GoldenCase
    from care_amd import get_framework
    from care_amd.synth import synth_labels

    case = GoldenCase(name)
    opt, P, feats, ids = case.build()
    opt.update(NO_DROP)
    opt.update(over)
    model = get_framework(opt)
    model.load_state_dict(P, strict=True)
    model.to(DEV).train()
    batch = {"feats": [f.to(DEV) for f in feats], "input_ids": ids.to(DEV)}
    return case, opt, P, feats, ids, model, batch, synth_labels(ids)


@pytest.mark.parametrize("name", MODEL_FIXTURES)
def test_criteria_on_a_training_forward_give_the_fixtures_metrics(name):
    """model.train() with dropout 0 is the eval forward: LanguageGeneration (eps 0) on its logits gives the reference's recorded
    Word Acc0 / Perplexity, NoisyOrMIL its F1@k / mAP - the bars of tests/test_gpu_parity.py's fp32 metrics test."""
    from care_amd import LanguageGeneration, NoisyOrMIL

    case, opt, P, feats, ids, model, batch, labels = _train_model(name)
    z = case.z
    assert np.array_equal(z["tf_labels"], labels.numpy())
    out = model(batch)
    lang = LanguageGeneration({**opt, "label_smoothing": 0.0})
    lang.reset_recorder()
    lang({"logits": out["logits"], "labels": labels.to(DEV)})
    acc, ppl = lang.get_info()[1]
    assert abs(acc - z["metrics_lang"][0]) < 1e-6
    assert abs(ppl / z["metrics_lang"][1] - 1) < 1e-5
    if "metrics_attr" in z:
        crit = NoisyOrMIL({**opt, "calculate_mAP": True})
        crit.reset_recorder()
        crit({"preds_attr": out["preds_attr"], "avg_prob_attr": out["avg_prob_attr"], "labels_attr": torch.from_numpy(z["labels_attr"])})
        np.testing.assert_allclose(crit.get_info()[1], z["metrics_attr"], rtol=1e-4, atol=1e-6)
    else:
        assert "preds_attr" not in out


@pytest.mark.parametrize("name", MODEL_FIXTURES)
def test_whole_training_step_matches_the_oracle_autograd(name):
    """criterion.get_loss({**model(batch), labels, labels_attr}).backward() with label smoothing 0.1 against the oracle's forward
    and the restated criteria under torch's autograd on the CPU: every parameter at tests/test_gpu_training.py's bar (1e-4 of the
    tensor's largest gradient + 2e-5)."""
    from care_amd import get_criterion
    from care_amd.synth import synth_labels_attr
    from oracle import care_cpu

    case, opt, P, feats, ids, model, batch, labels = _train_model(name, label_smoothing=0.1)
    has_attr = "attribute" in opt["crits"]
    labels_attr = synth_labels_attr(case.meta["seed"], ids.shape[0], opt["attribute_prediction_k"]) if has_attr else None
    criterion = get_criterion(opt)
    out = model(batch)
    results = {**out, "labels": labels.to(DEV)}
    if has_attr:
        results["labels_attr"] = labels_attr.to(DEV)
    loss = criterion.get_loss(results)
    loss.backward()

    Pc = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in P.items()}
    ref = care_cpu.feedforward_step(Pc, opt, feats, ids)
    rloss = total_loss(ref, labels, labels_attr, 0.1)
    rloss.backward()
    assert abs(float(loss.detach()) - float(rloss.detach())) < 1e-4 * abs(float(rloss.detach()))
    checked = 0
    for k, p in model.named_parameters():
        gref = Pc[k].grad
        if not p.requires_grad or gref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, "no gradient for " + k
        if k == "decoder.embedding.word_embeddings.weight":
            gref = gref.clone()
            gref[0] = 0.0   # nn.Embedding(padding_idx=PAD): no gradient for the PAD row; the oracle indexes a plain tensor
        scale = float(gref.abs().max())
        diff = float((p.grad.cpu() - gref).abs().max())
        assert diff < 1e-4 * scale + 2e-5, (k, diff, scale)
        checked += 1
    assert checked >= 20, checked
    info = criterion.get_loss_info()
    assert list(info)[: 2 if has_attr else 1] == (["Lang Loss", "V-Attr"] if has_attr else ["Lang Loss"])
    hits, words, nlogp = lang_counts(ref["logits"].detach().double(), labels)
    assert abs(info["Word Acc0"] - hits / words) < 1e-6 and abs(info["Perplexity"] / math.exp(nlogp / words) - 1) < 1e-5


def test_five_sgd_steps_with_the_criterion_lower_the_language_loss():
    from care_amd import get_criterion

    case, opt, P, feats, ids, model, batch, labels = _train_model("msrvtt_base_ami_b2", label_smoothing=0.1)
    criterion = get_criterion(opt)
    optim = torch.optim.SGD(model.parameters(), lr=0.01)
    lab = labels.to(DEV)
    losses = []
    for _ in range(5):
        criterion.reset_loss_recorder()
        optim.zero_grad()
        criterion.get_loss({**model(batch), "labels": lab}).backward()
        optim.step()
        losses.append(criterion.get_loss_info()["Lang Loss"])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses

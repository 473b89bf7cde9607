"""GPU: the self-critical loss on the fused head (care_amd/reward.py: self_critical_head_loss, _HeadRewardLoss;
csrc/head_reward.hip; the EPI_HEAD_STATS / EPI_HEAD_GRAD epilogues of csrc/gemm_tile.hip as they are) against float64.

Inputs: the `_Case` of tests/test_gpu_fused_head.py - random h and W, labels with exactly R live positions over captions of
unequal length, one caption all PAD, NaN in every dead hidden row - and one advantage per caption from a fixed cycle that holds
a negative value, an exact 0 and magnitudes from 1e3 down to 1e-3.
Reference: tests/test_gpu_scst.py's `_loss64` in float64 under autograd on `h.double() @ W.double().T`.  Bars:
  * loss, seq_logp, totals[0]: `_check`'s rule of tests/test_gpu_backward_kernels.py (FACTOR, FLOOR unchanged) with the UNFUSED
    path as the yardstick - training.py's `_Linear` under set_train_gemm("fp16x3") + self_critical_loss(return_aux=True) on the
    same inputs; totals[1] == R exactly;
  * dhidden and dW of GSCALE * loss: within GRAD_BAR = 1e-4 of the reference's largest magnitude (the fused head's bar); dead rows
    of dhidden exactly 0; everything finite.
Shapes: d in {64, 512} x V in {5, 130, 10547} (under one 64-column part; a last part of 2 columns; 165 parts) x R in
{1, 63, 129, 257} (one row; either side of a 64-row fragment and of a 256-row tile).
"""
import pytest
import torch

from test_gpu_backward_kernels import DEV, _check, _gen, _Worst
from test_gpu_fused_head import GRAD_BAR, GSCALE, T, _Case, _grad_ok, _labels
from test_gpu_scst import _loss64

pytestmark = pytest.mark.gpu

ADV_CYCLE = [1e3, 7.0, -0.5, 0.0, 1e-3, 1.0, 0.03, -20.0, 250.0, 0.4]   # caption s gets ADV_CYCLE[s % 10] (caption 1 is all PAD)


def _adv(n_seq):
    adv = torch.tensor([ADV_CYCLE[s % len(ADV_CYCLE)] for s in range(n_seq)], dtype=torch.float32)
    assert bool((adv < 0).any()) and float(adv.abs().max()) == 1e3
    return adv


def _reference(case, adv):
    """float64: loss, each caption's sum of logp, sum adv logp; dh and dW of GSCALE * loss."""
    h = case.h.double().requires_grad_(True)
    W = case.W.double().requires_grad_(True)
    loss, seq_logp = _loss64(h @ W.t(), case.ref_labels, adv)
    (GSCALE * loss).backward()
    return dict(loss=loss.detach(), seq_logp=seq_logp.detach(), total=-(loss.detach() * max(int(case.live.sum()), 1)), dh=h.grad, dW=W.grad)


def _fused(case, adv, hidden=None, live=None, acc=None, labels=None):
    from care_amd import self_critical_head_loss

    h = (case.h_nan if hidden is None else hidden).detach().clone().requires_grad_(True)
    W = case.W_dev.detach().clone().requires_grad_(True)
    loss, seq_logp, totals = self_critical_head_loss(h, W, case.lab32 if labels is None else labels, adv.to(DEV), acc=acc,
                                                     return_aux=True, live=live)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and not seq_logp.requires_grad
    (GSCALE * loss).backward()
    return dict(loss=loss.detach(), seq_logp=seq_logp, totals=totals, dh=h.grad, dW=W.grad)


def _unfused(case, adv):
    """The parent's path on the same inputs: the fp16x3 `_Linear` + self_critical_loss (the yardstick)."""
    from care_amd import self_critical_loss, training

    training.set_train_gemm("fp16x3")
    try:
        logits = training._Linear.apply(case.h_zero.reshape(-1, case.d), case.W_dev, None).view(case.n_seq, case.t, case.V)
    finally:
        training.set_train_gemm("auto")
    loss, seq_logp, totals = self_critical_loss(logits, case.lab32, adv.to(DEV), return_aux=True)
    return dict(loss=loss, seq_logp=seq_logp, totals=totals)


def _verify(case, worst, adv=None):
    adv = _adv(case.n_seq) if adv is None else adv
    ref, yard, run = _reference(case, adv), _unfused(case, adv), _fused(case, adv)
    tag = "d{} V{} R{}".format(case.d, case.V, case.R)
    _check(worst, tag + " loss", run["loss"], ref["loss"], yard["loss"])
    _check(worst, tag + " seq_logp", run["seq_logp"], ref["seq_logp"], yard["seq_logp"])
    _check(worst, tag + " totals[0]", run["totals"][0], ref["total"], yard["totals"][0])
    assert float(run["totals"][1]) == float(case.R) and run["totals"].dtype == torch.float64
    worst.grad = max(getattr(worst, "grad", 0.0), _grad_ok(tag + " dhidden", run["dh"].view_as(case.h_nan), ref["dh"]),
                     _grad_ok(tag + " dW", run["dW"], ref["dW"]))
    dead = (~case.live).to(DEV)
    assert float(run["dh"].view_as(case.h_nan)[dead].abs().max()) == 0.0      # NaN went in, exact zeros come out
    assert torch.isfinite(run["dh"]).all() and torch.isfinite(run["dW"]).all() and torch.isfinite(run["loss"])
    return run, ref


@pytest.mark.parametrize("R", [1, 63, 129, 257])
@pytest.mark.parametrize("V", [5, 130, 10547])
@pytest.mark.parametrize("d", [64, 512])
def test_head_reward_against_float64(d, V, R):
    worst = _Worst("head reward d{} V{} R{}".format(d, V, R))
    _verify(_Case(d, V, R, want_margin=False), worst)
    worst.report()
    print("worst gradient error / (1e-4 of the largest magnitude): {:.3g}".format(worst.grad))


def test_rows_scale_vector_and_scalar_forms():
    """care_rows_scale: 16-byte form (cols % 4 == 0, aligned), scalar form (odd cols; an odd stride; a misaligned view), in place;
    the bits of torch's elementwise product, nothing written outside the matrix."""
    from care_amd import _lib

    g = _gen(11, 5)
    for rows, cols, ld, off in ((1, 4, 4, 0), (67, 64, 64, 0), (67, 64, 68, 0), (5, 7, 7, 0), (33, 64, 65, 0), (9, 64, 64, 1), (300, 512, 512, 0)):
        src = torch.randn(rows, cols, generator=g).to(DEV)
        w = torch.randn(rows, generator=g).to(DEV)
        w[0] = 0.0
        buf = torch.full((rows * ld + off + 3,), float("nan"), device=DEV)
        dst = buf[off: off + rows * ld].view(rows, ld)
        _lib.call("care_rows_scale", src.data_ptr(), cols, w.data_ptr(), dst.data_ptr(), ld, rows, cols)
        assert torch.equal(dst[:, :cols], src * w.view(-1, 1)), (rows, cols, ld, off)
        assert torch.isnan(dst[:, cols:]).all() and torch.isnan(buf[:off]).all() and torch.isnan(buf[off + rows * ld:]).all()
        inplace = src.clone()
        _lib.call("care_rows_scale", inplace.data_ptr(), cols, w.data_ptr(), inplace.data_ptr(), cols, rows, cols)
        assert torch.equal(inplace, src * w.view(-1, 1))


def test_all_advantages_zero():
    case = _Case(64, 130, 63, want_margin=False)
    run = _fused(case, torch.zeros(case.n_seq))
    assert float(run["loss"]) == 0.0 and float(run["totals"][0]) == 0.0 and float(run["totals"][1]) == 63.0
    assert float(run["dh"].abs().max()) == 0.0 and float(run["dW"].abs().max()) == 0.0
    assert torch.isfinite(run["seq_logp"]).all() and float(run["seq_logp"].abs().max()) > 0.0


@pytest.mark.parametrize("give_live", [False, True])
def test_all_pad_batch(give_live, monkeypatch):
    from care_amd import _lib, self_critical_head_loss

    launched = []
    real = _lib.call

    def spy(name, *args, **kw):
        launched.append(name)
        return real(name, *args, **kw)

    V, d = 130, 64
    h = torch.full((3, 5, d), float("nan"), device=DEV, requires_grad=True)
    W = torch.randn(V, d, device=DEV, requires_grad=True)
    labels = torch.zeros(3, 5, dtype=torch.int64, device=DEV)
    acc = torch.zeros(2, device=DEV, dtype=torch.float64)
    monkeypatch.setattr(_lib, "call", spy)
    loss, seq_logp, totals = self_critical_head_loss(h, W, labels, torch.ones(3, device=DEV), acc=acc, return_aux=True,
                                                     live=0 if give_live else None)
    loss.backward()
    monkeypatch.undo()
    assert float(loss.detach()) == 0.0 and totals.tolist() == [0.0, 0.0] and seq_logp.tolist() == [0.0, 0.0, 0.0] and acc.tolist() == [0.0, 0.0]
    assert h.grad.shape == h.shape and float(h.grad.abs().max()) == 0.0
    assert W.grad.shape == W.shape and float(W.grad.abs().max()) == 0.0
    assert sorted(set(launched)) == ["care_head_live_rows", "care_head_reward_reduce"]      # no GEMM, nothing with M = 0


def test_out_of_range_labels_are_dead_rows():
    V = 2003
    labels = _labels(129, V, 9)
    labels[1, 0], labels[1, 5], labels[2, T - 1], labels[2, T - 2] = V, -1, V + 7, -(2 ** 31)
    case = _Case(64, V, 129, labels=labels, want_margin=False)
    assert int(case.live.sum()) == 129
    worst = _Worst("bad labels")
    _verify(case, worst)
    worst.report()


def test_hidden_with_one_more_position_than_the_labels():
    """[N, t + 1, d] hidden against [N, t] labels: the last position is dead - NaN there changes nothing."""
    case = _Case(64, 130, 63, want_margin=False)
    adv = _adv(case.n_seq)
    a = _fused(case, adv)
    longer = torch.cat([case.h_nan, torch.full((case.n_seq, 1, case.d), float("nan"), device=DEV)], dim=1)
    b = _fused(case, adv, hidden=longer)
    assert b["dh"].shape == (case.n_seq, T + 1, case.d) and float(b["dh"][:, T].abs().max()) == 0.0
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["seq_logp"], b["seq_logp"]) and torch.equal(a["totals"], b["totals"])
    assert torch.equal(a["dh"], b["dh"][:, :T]) and torch.equal(a["dW"], b["dW"])


def test_two_calls_give_identical_bits():
    case = _Case(512, 2003, 257, want_margin=False)
    adv = _adv(case.n_seq)
    acc = torch.zeros(2, device=DEV, dtype=torch.float64)
    a, b = _fused(case, adv, acc=acc), _fused(case, adv, live=257, acc=acc)
    for k in ("loss", "seq_logp", "totals", "dh", "dW"):
        assert torch.equal(a[k], b[k]), k
    assert acc.tolist() == [2.0 * float(a["loss"]), 2.0 * 257]       # the recorder's doubles: += (loss, n_live) per call


def test_chunked_against_whole(monkeypatch):
    """HEAD_CHUNK_ROWS forced to 100 at 257 live rows (3 chunks): loss and seq_logp are the single-chunk run's bits (a row's
    results do not depend on the rows beside it); the gradients stay within the bar."""
    import care_amd.criterion as criterion

    case = _Case(512, 2003, 257, want_margin=False)
    adv = _adv(case.n_seq)
    whole = _fused(case, adv)
    monkeypatch.setattr(criterion, "HEAD_CHUNK_ROWS", 100)
    assert len(criterion.head_chunks(257)) == 3
    parts = _fused(case, adv)
    for k in ("loss", "seq_logp", "totals"):
        assert torch.equal(whole[k], parts[k]), k
    ref = _reference(case, adv)
    for run in (whole, parts):
        _grad_ok("dhidden", run["dh"], ref["dh"])
        _grad_ok("dW", run["dW"], ref["dW"])


def test_dw_in_slabs():
    """Few output tiles and a long reduction (V = 130, d = 64, 1100 live rows): dW = dl^T (w (.) h) runs in K slabs of live rows."""
    from care_amd.training import _x3_slabs

    assert _x3_slabs(130, 64, 1100) > 1
    worst = _Worst("dW in slabs")
    _verify(_Case(64, 130, 1100, want_margin=False), worst)
    worst.report()


def test_no_host_synchronisation_when_the_live_count_is_given():
    case = _Case(64, 130, 129, want_margin=False)
    adv = _adv(case.n_seq).to(DEV)
    _fused(case, adv, live=129)      # (first launches load code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run = _fused(case, adv, live=129)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = _reference(case, adv.cpu())
    _grad_ok("dhidden", run["dh"], ref["dh"])
    _grad_ok("dW", run["dW"], ref["dW"])


def test_peak_memory_stays_below_one_copy_of_the_logits():
    """64 captions x 29 x 10547, a quarter of the positions live at most: forward + backward of the fused loss allocates less than
    ONE [N, t, V] fp32 tensor above its starting level (the gradient's pieces are 8 R V <= 2 N t V bytes); the unfused path more
    than two (the logits and their gradient)."""
    from care_amd import self_critical_head_loss, self_critical_loss, training

    N, V, d = 64, 10547, 512
    g = _gen(64, 29, 10547)
    labels = torch.zeros(N, T, dtype=torch.int64)
    labels[:, :7] = torch.randint(1, V, (N, 7), generator=g)
    assert 4 * int((labels > 0).sum()) <= N * T
    labels = labels.to(DEV)
    h = torch.randn(N, T, d, generator=g).to(DEV).requires_grad_(True)
    W = (torch.randn(V, d, generator=g) * 0.1).to(DEV).requires_grad_(True)
    adv = torch.randn(N, generator=g).to(DEV)
    one = N * T * V * 4

    def rise(loss_of):
        h.grad = W.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss_of().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = rise(lambda: self_critical_head_loss(h, W, labels, adv, live=N * 7))
    unfused = rise(lambda: self_critical_loss(training._Linear.apply(h.view(N * T, d), W, None).view(N, T, V), labels, adv))
    print("peak rise: fused {:.1f} MB, unfused {:.1f} MB, one [N, t, V] fp32 tensor {:.1f} MB".format(fused / 2 ** 20, unfused / 2 ** 20, one / 2 ** 20))
    assert fused < one, (fused, one)
    assert unfused > 2 * one, (unfused, one)

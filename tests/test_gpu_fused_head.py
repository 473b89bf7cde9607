"""GPU: the training head fused with the language loss (care_amd/criterion.py: DeferredLogits, _HeadLoss; csrc/head_loss.hip, the
EPI_HEAD_STATS / EPI_HEAD_GRAD epilogues of csrc/gemm_tile.hip) against float64.

References: tests/crit_reference.py in float64 on `hidden @ W.T`, also computed in float64.  Bars:
  * the scalar loss, sum -logp and the per-row lse / logp / row loss: `_check`'s rule of tests/test_gpu_backward_kernels.py with the
    UNFUSED path as the yardstick - training.py's `_Linear` under set_train_gemm("fp16x3") + care_lang_loss_fwd on the same inputs:
    error <= 4 x that path's error against float64 + 2^-22 x the reference's largest magnitude;
  * dhidden and dW: within 1e-4 of the tensor's largest magnitude (the training bar of tests/test_gpu_training.py, without its
    absolute floor);
  * pred, hits, words, bad labels: exactly - on inputs whose float64 top-1 / top-2 margin is >= 1e-3 on EVERY live row (asserted on
    the CPU; the generator's seed is stepped until it holds).
Shapes: d in {64, 512} (one and eight K steps), V in {5, 130, 2003, 10547} (one part narrower than a lane's 16 columns; three parts,
the last 2 wide, ks = 192; odd; the workload's), live rows in {1, 63, 129, 257} (the edges of the 128- and 256-row tiles +- 1) spread
over sequences of unequal length with one sequence all PAD; the hidden rows of every dead position are NaN on the device.

*Measured* on one MI355X (pytest -s): worst error / bar over the 32 shape cases 0.33 (the ordered loss sum at d 512, V 5, R 129),
0.15 - 0.22 elsewhere; gradients at most 0.040 of their bar; the loss through the model 0.15 of its bar.
"""
import math

import pytest
import torch

from crit_reference import lang_rows, total_loss
from test_gpu_backward_kernels import DEV, _check, _gen, _Worst

pytestmark = pytest.mark.gpu

T = 29
GSCALE = 0.37          # the upstream gradient of the loss (a device scalar in the backward)
GRAD_BAR = 1e-4


def _labels(R, V, key):
    """[n_seq, T] labels with exactly R live positions: captions of unequal length (prefixes), sequence 1 all PAD."""
    n_seq = max(3, -(-R // (T - 4)) + 2)
    g = _gen(R, V, key)
    labels = torch.zeros(n_seq, T, dtype=torch.int64)
    left = R
    for s in [i for i in range(n_seq) if i != 1]:
        n = min(T - (s % 5), left)
        labels[s, :n] = torch.randint(1, V, (n,), generator=g)
        left -= n
    assert left == 0 and int((labels > 0).sum()) == R and int(labels[1].abs().sum()) == 0
    return labels


class _Case:
    """Inputs on the CPU (float64 reference computed once) and on the device (NaN at the dead positions)."""

    def __init__(self, d, V, R, labels=None, tie=None, want_margin=True):
        self.d, self.V, self.R = d, V, R
        self.labels = _labels(R, V, d) if labels is None else labels
        self.n_seq, self.t = self.labels.shape
        live = (self.labels > 0) & (self.labels < V)
        self.live = live
        self.ref_labels = torch.where(live, self.labels, torch.zeros_like(self.labels))   # bad labels: left out, like PAD
        for attempt in range(64):
            g = _gen(d, V, R, attempt)
            h = torch.randn(self.n_seq, self.t, d, generator=g)
            W = torch.randn(V, d, generator=g) * (2.0 / math.sqrt(d))
            if tie is not None:
                W[tie[0]] *= 4.0
                W[tie[1]] = W[tie[0]]
            h[~live] = 0.0
            logits = h.double() @ W.double().t()
            top2 = logits[live].topk(min(2, V), dim=-1)[0]
            if not want_margin or V < 2 or float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3:
                break
        self.h, self.W, self.logits64 = h, W, logits
        if want_margin and V >= 2:
            assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3, "no input with a top-1 / top-2 margin of 1e-3 on every live row"
        self.W_dev = W.to(DEV)
        self.h_zero = h.to(DEV)
        self.h_nan = self.h_zero.clone()
        self.h_nan[(~live).to(DEV)] = float("nan")
        self.lab32 = self.labels.to(DEV, torch.int32).contiguous()

    def reference(self, eps):
        """float64: per-row (row loss, logp, pred, lse) at the live rows, loss, sum -logp, hits; dh and dW of GSCALE * loss."""
        h = self.h.double().requires_grad_(True)
        W = self.W.double().requires_grad_(True)
        row, logp, pred, lse = lang_rows(h @ W.t(), self.ref_labels, eps)
        m = self.live.double()
        loss = (row * m).sum()
        (GSCALE * loss).backward()
        return dict(row=(row * m).detach(), logp=(logp * m).detach(), lse=(lse * m).detach(), pred=pred * self.live, loss=loss.detach(),
                    nlogp=-(logp * m).sum().detach(), hits=int(((pred == self.ref_labels) & self.live).sum()), dh=h.grad, dW=W.grad)

    def fused(self, eps, hidden=None, live=None, acc=None):
        from care_amd.criterion import _HeadLoss

        h = (self.h_nan if hidden is None else hidden).detach().clone().requires_grad_(True)
        W = self.W_dev.detach().clone().requires_grad_(True)
        loss, pred, counts = _HeadLoss.apply(h.reshape(-1, self.d), W, self.lab32, eps, acc, live)
        (GSCALE * loss).backward()
        return dict(loss=loss.detach(), pred=pred, counts=counts, dh=h.grad, dW=W.grad)

    def fused_rows(self, eps):
        from care_amd.criterion import _head_forward

        sums, pred, counts, stats, R, _ = _head_forward(self.h_nan.reshape(-1, self.d), self.W_dev, self.lab32, eps, None)
        assert R == int(self.live.sum())
        shape = (self.n_seq, self.t)
        return dict(lse=stats[0].view(shape), logp=stats[3].view(shape), row=stats[4].view(shape), loss=sums[0], nlogp=sums[1],
                    pred=pred.view(shape), counts=counts)

    def unfused(self, eps):
        """The parent's path on the same inputs: the fp16x3 `_Linear` + care_lang_loss_fwd (the yardstick)."""
        from care_amd import _lib, training

        training.set_train_gemm("fp16x3")
        try:
            logits = training._Linear.apply(self.h_zero.reshape(-1, self.d), self.W_dev, None)
        finally:
            training.set_train_gemm("auto")
        rows = self.n_seq * self.t
        stats = torch.zeros(5, rows, device=DEV)
        pred = torch.zeros(rows, device=DEV, dtype=torch.int32)
        sums = torch.zeros(2, device=DEV)
        counts = torch.zeros(3, device=DEV, dtype=torch.int32)
        p = lambda x: x.data_ptr()
        _lib.call("care_lang_loss_fwd", p(logits), self.V, self.t * self.V, self.t, self.V, p(self.lab32), eps, p(stats[0]), p(stats[1]),
                  p(stats[2]), p(stats[3]), p(pred), p(stats[4]), p(sums), p(counts), None, rows)
        shape = (self.n_seq, self.t)
        return dict(lse=stats[0].view(shape), logp=stats[3].view(shape), row=stats[4].view(shape), loss=sums[0], nlogp=sums[1])


def _grad_ok(what, got, ref64):
    got, ref64 = got.detach().double().cpu(), ref64.double()
    assert got.shape == ref64.shape and torch.isfinite(got).all(), what
    scale, diff = float(ref64.abs().max()), float((got - ref64).abs().max())
    assert diff <= GRAD_BAR * scale, (what, diff, scale)
    return diff / max(scale, 1e-300) / GRAD_BAR


def _verify(case, worst, eps_list=(0.0, 0.1)):
    for eps in eps_list:
        ref, rows, yard, run = case.reference(eps), case.fused_rows(eps), case.unfused(eps), case.fused(eps)
        tag = "d{} V{} R{} eps{}".format(case.d, case.V, case.R, eps)
        for k in ("lse", "logp", "row", "loss", "nlogp"):
            _check(worst, tag + " " + k, rows[k], ref[k], yard[k])
        _check(worst, tag + " loss (autograd)", run["loss"], ref["loss"], yard["loss"])
        assert torch.equal(run["loss"], rows["loss"])
        assert torch.equal(rows["pred"].cpu().long(), ref["pred"]), tag
        assert torch.equal(run["pred"].cpu().long(), ref["pred"]), tag
        assert run["counts"].tolist() == [ref["hits"], case.R, int(((case.labels < 0) | (case.labels >= case.V)).sum())], tag
        worst.grad = max(getattr(worst, "grad", 0.0), _grad_ok(tag + " dhidden", run["dh"], ref["dh"]), _grad_ok(tag + " dW", run["dW"], ref["dW"]))
        # dead positions: NaN went in, exact zeros come out
        dead = (~case.live).to(DEV)
        assert float(run["dh"][dead].abs().max()) == 0.0 if bool(dead.any()) else True
        assert torch.isfinite(run["dh"]).all() and torch.isfinite(run["dW"]).all() and torch.isfinite(run["loss"])


@pytest.mark.parametrize("R", [1, 63, 129, 257])
@pytest.mark.parametrize("V", [5, 130, 2003, 10547])
@pytest.mark.parametrize("d", [64, 512])
def test_fused_head_against_float64(d, V, R):
    worst = _Worst("fused head d{} V{} R{}".format(d, V, R))
    _verify(_Case(d, V, R), worst)
    worst.report()
    print("worst gradient error / (1e-4 of the largest magnitude): {:.3g}".format(worst.grad))


@pytest.mark.parametrize("V", [130, 10547])
def test_labels_at_the_edges_of_a_part(V):
    """Labels at columns 1, 63, 64 and V - 1 (0 is PAD): the first and last column of a lane's 16, of a 64-column part, of the row."""
    labels = _labels(63, V, 3)
    pos = (labels > 0).nonzero()
    for (s, p), y in zip(pos[:8].tolist(), [1, 63, 64, V - 1] * 2):
        labels[s, p] = y
    worst = _Worst("edge labels V{}".format(V))
    _verify(_Case(64, V, 63, labels=labels), worst)
    worst.report()


def test_a_tie_across_two_parts_predicts_the_first_index():
    """Two identical rows of W (columns 10 and 100: parts 0 and 1): an exact tie of a row's maximum; the lower column is predicted."""
    V, lo, hi = 130, 10, 100
    case = _Case(64, V, 63, tie=(lo, hi), want_margin=False)
    lg = case.logits64[case.live]
    tied = (lg[:, lo] == lg.max(-1)[0])
    assert int(tied.sum()) >= 10 and torch.equal(lg[:, lo], lg[:, hi])
    masked = lg.clone()
    masked[:, hi] = -float("inf")
    top2 = masked.topk(2, dim=-1)[0]
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3      # nothing else is close on any live row
    want = masked.argmax(-1)
    for eps in (0.0, 0.1):
        run = case.fused(eps)
        got = run["pred"].cpu().long()[case.live]
        assert torch.equal(got, want) and int((got == lo).sum()) == int(tied.sum()) and int((got == hi).sum()) == 0


def test_pad_and_out_of_range_labels():
    """NaN hidden rows under PAD and bad labels: finite results, exactly zero dhidden rows there; bad labels are counted and
    get_loss_info() raises with the count."""
    from care_amd.criterion import DeferredLogits, get_criterion
    from care_amd.configs import make_opt

    V = 2003
    labels = _labels(129, V, 9)
    labels[1, 0], labels[1, 5], labels[2, T - 1], labels[2, T - 2] = V, -1, V + 7, -(2 ** 31)
    case = _Case(64, V, 129, labels=labels)
    assert int(case.live.sum()) == 129
    worst = _Worst("bad labels")
    _verify(case, worst, eps_list=(0.1,))
    crit = get_criterion(make_opt("msrvtt_base_ami", label_smoothing=0.1, vocab_size=V))
    for device_labels in (False, True):
        crit.reset_loss_recorder()
        h = case.h_nan.clone().requires_grad_(True)
        loss = crit.get_loss({"logits": DeferredLogits(h, case.W_dev), "labels": labels.to(DEV) if device_labels else labels})
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(h.grad).all()
        assert float(h.grad[(~case.live).to(DEV)].abs().max()) == 0.0
        assert crit.crit_objects[0].last_counts.tolist()[1:] == [129, 4]
        with pytest.raises(ValueError, match=r"^4 label\(s\) outside"):
            crit.get_loss_info()


@pytest.mark.parametrize("device_labels", [False, True])
def test_all_pad_batch(device_labels):
    from care_amd import _lib
    from care_amd.criterion import DeferredLogits, LanguageGeneration
    from care_amd.configs import make_opt

    launched = []
    real = _lib.call

    def spy(name, *args, **kw):
        launched.append(name)
        return real(name, *args, **kw)

    V, d = 130, 64
    h = torch.full((3, 5, d), float("nan"), device=DEV, requires_grad=True)
    W = torch.randn(V, d, device=DEV, requires_grad=True)
    labels = torch.zeros(3, 5, dtype=torch.int64)
    lang = LanguageGeneration(make_opt("msrvtt_base_ami", label_smoothing=0.1, vocab_size=V))
    import care_amd.criterion as criterion
    criterion.call, keep = spy, criterion.call
    try:
        loss, _ = lang({"logits": DeferredLogits(h, W), "labels": labels.to(DEV) if device_labels else labels})
        loss.backward()
    finally:
        criterion.call = keep
    assert float(loss.detach()) == 0.0 and lang.last_counts.tolist() == [0, 0, 0] and int(lang.last_pred.abs().sum()) == 0
    assert h.grad.shape == h.shape and float(h.grad.abs().max()) == 0.0
    assert W.grad.shape == W.shape and float(W.grad.abs().max()) == 0.0
    assert sorted(set(launched)) == ["care_head_live_rows", "care_lang_loss_reduce"]      # nothing with M = 0
    assert lang.get_info()[1] == [0, 1.0]


def test_two_calls_give_identical_bits():
    case = _Case(512, 2003, 257)
    a, b = case.fused(0.1), case.fused(0.1, live=257)
    for k in ("loss", "pred", "dh", "dW", "counts"):
        assert torch.equal(a[k], b[k]), k


def test_hidden_with_one_more_position_than_the_labels():
    """[N, t + 1, d] hidden against [N, t] labels (crit_lang.py:49-52): the last position is dead - NaN there changes nothing."""
    from care_amd.criterion import DeferredLogits, LanguageGeneration
    from care_amd.configs import make_opt

    case = _Case(64, 130, 63)
    lang = LanguageGeneration(make_opt("msrvtt_base_ami", label_smoothing=0.1, vocab_size=130))
    res = []
    for extra in (False, True):
        h = case.h_nan
        if extra:
            h = torch.cat([h, torch.full((case.n_seq, 1, case.d), float("nan"), device=DEV)], dim=1)
        h = h.clone().requires_grad_(True)
        W = case.W_dev.clone().requires_grad_(True)
        loss, _ = lang({"logits": DeferredLogits(h, W), "labels": case.labels})
        loss.backward()
        res.append((loss.detach(), lang.last_pred, h.grad, W.grad))
    (l0, p0, h0, w0), (l1, p1, h1, w1) = res
    assert h1.shape == (case.n_seq, T + 1, case.d) and float(h1[:, T].abs().max()) == 0.0
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(h0, h1[:, :T]) and torch.equal(w0, w1)
    ref = case.reference(0.1)
    _grad_ok("dhidden", h1[:, :T], ref["dh"] / GSCALE / case.n_seq)


def test_chunked_against_whole(monkeypatch):
    """HEAD_CHUNK_ROWS forced to 64 at 257 live rows (5 chunks, the last of one row): loss, pred and dhidden are the single-chunk
    run's bits (a row's results do not depend on the rows beside it); dW's sums regroup and stay within the gradient bar."""
    import care_amd.criterion as criterion

    case = _Case(512, 2003, 257)
    whole = case.fused(0.1)
    monkeypatch.setattr(criterion, "HEAD_CHUNK_ROWS", 64)
    assert len(criterion.head_chunks(257)) == 5
    parts = case.fused(0.1)
    for k in ("loss", "pred", "dh", "counts"):
        assert torch.equal(whole[k], parts[k]), k
    ref = case.reference(0.1)
    _grad_ok("dW in chunks", parts["dW"], ref["dW"])
    _grad_ok("dW whole", whole["dW"], ref["dW"])


def test_dw_in_slabs():
    """Few output tiles and a long reduction (V = 130, d = 64, 1100 live rows): dW = dl^T h runs in K slabs of live rows
    (training._x3_slabs), the transposed pieces slab-major."""
    from care_amd.training import _x3_slabs

    assert _x3_slabs(130, 64, 1100) > 1
    worst = _Worst("dW in slabs")
    _verify(_Case(64, 130, 1100), worst, eps_list=(0.1,))
    worst.report()


# ================================================================================ through the model
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _train_model(name):
    from conftest import GoldenCase
    from care_amd import get_framework
    from care_amd.synth import synth_labels, synth_labels_attr

    case = GoldenCase(name)
    opt, P, feats, ids = case.build()
    opt.update(NO_DROP)
    opt["label_smoothing"] = 0.1
    model = get_framework(opt)
    model.load_state_dict(P, strict=True)
    model.to(DEV).train()
    batch = {"feats": [f.to(DEV) for f in feats], "input_ids": ids.to(DEV)}
    labels_attr = synth_labels_attr(case.meta["seed"], ids.shape[0], opt["attribute_prediction_k"]) if "attribute" in opt["crits"] else None
    return opt, P, feats, ids, model, batch, synth_labels(ids), labels_attr


def _two_steps(model, batch, labels, labels_attr, opt):
    from care_amd import get_criterion

    criterion = get_criterion(opt)
    for step in range(2):
        for p in model.parameters():
            p.grad = None
        results = {**model(batch), "labels": labels}      # labels on the host, as a loader hands them over
        if labels_attr is not None:
            results["labels_attr"] = labels_attr.to(DEV)
        loss = criterion.get_loss(results)
        loss.backward()
    return loss.detach(), criterion.get_loss_info(), results


@pytest.mark.parametrize("name", ["msrvtt_base_ami_b2", "msrvtt_care_b2"])
def test_fused_head_through_the_model(name):
    """set_fused_head(True) on the smallest training fixtures (one with the concept head): every parameter's gradient within
    tests/test_gpu_training.py's bar of the oracle's autograd, the loss within the bar above (yardstick: the unfused run), the
    metrics of two steps equal to the unfused run's."""
    from care_amd.criterion import DeferredLogits
    from oracle import care_cpu

    from care_amd import training

    opt, P, feats, ids, model, batch, labels, labels_attr = _train_model(name)
    # The unfused run is the yardstick's: set_train_gemm("fp16x3"), the arithmetic the fused head always uses.  (Under "auto" these
    # 58-row batches send the unfused head to the exact-f32 kernel, and two steps' perplexity of msrvtt_care_b2 then differs
    # from the fused run's by 1.05e-6 relative - the 2^-22 of a split product on logits of ~20 - *measured*.)
    training.set_train_gemm("fp16x3")
    try:
        loss_u, info_u, res_u = _two_steps(model, batch, labels, labels_attr, opt)
        assert isinstance(res_u["logits"], torch.Tensor)
        model.set_fused_head(True)
        loss_f, info_f, res_f = _two_steps(model, batch, labels, labels_attr, opt)
    finally:
        training.set_train_gemm("auto")
    assert isinstance(res_f["logits"], DeferredLogits) and tuple(res_f["logits"].shape) == tuple(res_u["logits"].shape)
    assert torch.equal(res_f["hidden_states"], res_u["hidden_states"])

    Pc = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in P.items()}
    ref = care_cpu.feedforward_step(Pc, opt, feats, ids)
    total_loss(ref, labels, labels_attr, 0.1).backward()
    # the loss in float64: the oracle's forward on float64 parameters
    P64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in P.items()}
    with torch.no_grad():
        ref64 = care_cpu.feedforward_step(P64, opt, [f.double() for f in feats], ids)
        assert ref64["logits"].dtype == torch.float64
        loss64 = total_loss(ref64, labels, labels_attr.double() if labels_attr is not None else None, 0.1)
    worst = _Worst("model " + name)
    _check(worst, "loss", loss_f, loss64, loss_u)
    worst.report()
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
    for k in ("Word Acc0", "Perplexity"):
        print(name, k, "fused", info_f[k], "unfused", info_u[k], "|difference| / |unfused| = {:.3g}".format(abs(info_f[k] - info_u[k]) / max(abs(info_u[k]), 1e-300)))
        assert abs(info_f[k] - info_u[k]) <= 1e-6 * abs(info_u[k]), (k, info_f[k], info_u[k])
    assert abs(info_f["Lang Loss"] - info_u["Lang Loss"]) <= 1e-5 * abs(info_u["Lang Loss"])


def test_switch_off_is_the_parents_path_bit_for_bit():
    """Off (the default): a plain tensor under `logits`, the same bits before the switch was ever touched and after it was turned on
    and off again; on: the deferred object, whose materialize() is that tensor."""
    from care_amd.criterion import DeferredLogits

    opt, P, feats, ids, model, batch, labels, _ = _train_model("msrvtt_base_ami_b2")
    assert model.fused_head is False
    before = model(batch)["logits"]
    assert isinstance(before, torch.Tensor) and before.requires_grad
    model.set_fused_head(True)
    deferred = model(batch)["logits"]
    assert isinstance(deferred, DeferredLogits)
    assert torch.equal(deferred.materialize(), before)
    model.set_fused_head(False)
    after = model(batch)["logits"]
    assert isinstance(after, torch.Tensor) and torch.equal(after, before)


def test_peak_memory_stays_below_one_copy_of_the_logits():
    """64 clips x 29 x 10547, a quarter of the positions live at most: forward + backward of the fused criterion allocates less than
    ONE [N, t, V] fp32 tensor above its starting level (the gradient's pieces are 8 R V <= 2 N t V bytes); the unfused path more
    than two (the logits and their gradient)."""
    from care_amd.criterion import DeferredLogits, LanguageGeneration
    from care_amd.configs import make_opt
    from care_amd import training

    N, V, d = 64, 10547, 512
    g = _gen(64, 29, 10547)
    labels = torch.zeros(N, T, dtype=torch.int64)
    labels[:, :7] = torch.randint(1, V, (N, 7), generator=g)
    assert 4 * int((labels > 0).sum()) <= N * T
    h = torch.randn(N, T, d, generator=g).to(DEV).requires_grad_(True)
    W = (torch.randn(V, d, generator=g) * 0.1).to(DEV).requires_grad_(True)
    lang = LanguageGeneration(make_opt("msrvtt_base_ami", label_smoothing=0.1))
    one = N * T * V * 4

    def rise(make_logits):
        h.grad = W.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, _ = lang({"logits": make_logits(), "labels": labels})
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = rise(lambda: DeferredLogits(h, W))
    unfused = rise(lambda: training._Linear.apply(h.view(N * T, d), W, None).view(N, T, V))
    print("peak rise: fused {:.1f} MB, unfused {:.1f} MB, one [N, t, V] fp32 tensor {:.1f} MB".format(fused / 2 ** 20, unfused / 2 ** 20, one / 2 ** 20))
    assert fused < one, (fused, one)
    assert unfused > 2 * one, (unfused, one)

"""GPU: the mean-teacher step at the module level (care_amd/interplay.py; models/Wrapper.py:550-614) - `distillation_mse` under
autograd, `ema_update` over the parameters of real modules, and `InterplayStep.training_step` on msrvtt_base_ami / msrvtt_care with 4
clips and captions of 3 to 9 tokens: the teacher must follow, bit for bit, the CPU recursion of torch's three `_foreach` calls over
the student's weights, and validation inside `evaluating()` must decode with the teacher the kernels just wrote."""
import copy
import gc

import pytest
import torch

import interplay_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
CLIPS, T = 4, 9
LENGTHS = (3, 5, 7, 9)


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    """These tests build modules, optimisers and - where they evaluate - inference engines with captured hipGraphs and side
    streams.  The first optimiser a process constructs pins its callers' frames in a reference cycle (torch's lazy imports), so a
    test's modules and engines can outlive it until the cyclic collector runs - and if that is in the middle of ANOTHER test's
    graph capture, destroying a captured graph there frees device memory on the capturing thread, which a capture does not
    survive.  Whatever a test here leaves is collected right behind it, outside any capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _opt(config, **over):
    from care_amd.configs import make_opt

    return make_opt(config, max_len=T + 1, label_smoothing=0.1, learning_rate=1e-3, gradient_clip_val=5.0, **over)


def _batch(opt, seed=3):
    from care_amd.configs import feat_shapes
    from care_amd.constants import BOS, EOS, PAD
    from care_amd.synth import synth_labels, synth_labels_attr

    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(s, generator=g) for s in feat_shapes(opt, CLIPS)]
    ids = torch.full((CLIPS, T), PAD, dtype=torch.long)
    for r, n in enumerate(LENGTHS):          # BOS, words, EOS (the longest caption's EOS is its last label's business), then PAD
        ids[r, 0] = BOS
        ids[r, 1:n] = torch.randint(6, opt["vocab_size"], (n - 1,), generator=g)
        if n < T:
            ids[r, n - 1] = EOS
    batch = {"feats": [f.to(DEV) for f in feats], "input_ids": ids.to(DEV), "labels": synth_labels(ids)}
    if "attribute" in opt["crits"]:
        batch["labels_attr"] = synth_labels_attr(seed, CLIPS, opt["attribute_prediction_k"]).to(DEV)
    return batch


def _model(opt, seed, like=None):
    from care_amd import get_framework

    torch.manual_seed(seed)
    model = get_framework(opt)
    if like is not None:
        model.load_state_dict({k: v.detach().cpu().clone() for k, v in like.state_dict().items()}, strict=True)
    return model.to(DEV).train()


def _snapshot(model):
    return [p.detach().cpu().clone() for p in model.parameters()]


def _same_bits(params, want):
    return all(torch.equal(R.bits(p), R.bits(w)) for p, w in zip(params, want))


def _capture_logits(model, into):
    return model.register_forward_hook(lambda mod, args, out: into.append(out["logits"].detach().clone()))


def test_distillation_mse_under_autograd():
    from care_amd import distillation_mse

    g = torch.Generator().manual_seed(5)
    a = torch.randn(CLIPS, T, 10547, generator=g)
    b = a + 0.05 * torch.randn(CLIPS, T, 10547, generator=g)
    sa, tb = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    loss = distillation_mse(sa, tb)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda" and loss.requires_grad
    (loss * 0.25).backward()
    want, want_grad = R.mse_reference64(a, b), R.mse_grad_reference64(a, b, 0.25)
    got = float(loss.detach())
    dev = ((sa.grad.cpu().double() - want_grad).abs() / want_grad.abs()).max().item()
    print("loss", got, "float64", want, "relative deviation", abs(got - want) / want, "gradient: worst relative deviation", dev, "bar", R.BAR)
    assert abs(got - want) <= R.BAR * want
    assert bool((want_grad != 0).all()) and dev <= R.BAR
    assert tb.grad is None, "the teacher's logits get no gradient"
    # other layouts and dtypes are brought to contiguous fp32; nothing in forward or backward waits for the device
    half = sa.detach()[:, ::2].requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l2 = distillation_mse(half, tb.detach()[:, ::2].double())
        l2.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want2 = R.mse_reference64(a[:, ::2], b[:, ::2])
    assert abs(float(l2.detach()) - want2) <= R.BAR * want2 and half.grad.shape == half.shape


def test_ema_update_over_the_parameters_of_two_real_modules():
    from care_amd import ema_update

    opt = _opt("msrvtt_care")
    student, teacher = _model(opt, 1), _model(opt, 2)
    t0, s0 = _snapshot(teacher), _snapshot(student)
    vt, vs = [p._version for p in teacher.parameters()], [p._version for p in student.parameters()]
    ema_update(teacher.parameters(), student.parameters(), 0.999)
    torch.cuda.synchronize()
    assert len(t0) >= 50 and _same_bits(teacher.parameters(), R.ema_reference(t0, s0, 0.999))
    assert not _same_bits(teacher.parameters(), t0)
    assert _same_bits(student.parameters(), s0)
    assert all(p._version > v for p, v in zip(teacher.parameters(), vt)), "every teacher parameter's version must move"
    assert [p._version for p in student.parameters()] == vs, "the student is read, never written"


@pytest.mark.parametrize("config", ["msrvtt_base_ami", "msrvtt_care"])
def test_three_training_steps_with_dropout(config):
    from care_amd import InterplayStep

    opt = _opt(config)
    batch = _batch(opt)
    student = _model(opt, 1)
    step = InterplayStep(opt, student)
    teacher = step.teacher_captioner
    assert teacher is not student and next(teacher.parameters()).device == next(student.parameters()).device and teacher.training
    s_logits, t_logits = [], []
    hooks = [_capture_logits(student, s_logits), _capture_logits(teacher, t_logits)]
    expect = _snapshot(teacher)
    assert step.distillation_weight == 0.01 and step.ema_weight == 0.999
    for i in range(3):
        loss = step.training_step(batch, current_epoch=0)
        assert loss.requires_grad and len(s_logits) == len(t_logits) == i + 1
        expect = R.ema_reference(expect, _snapshot(student), 0.999)
        assert _same_bits(teacher.parameters(), expect), "step {}: the teacher left the recursion of the three _foreach calls".format(i)
        last = step.last
        assert sorted(last) == ["captioning_loss", "distillation_loss", "total_loss"]
        assert all(v.device.type == "cuda" and v.dim() == 0 and not v.requires_grad for v in last.values())
        want = R.mse_reference64(s_logits[i], t_logits[i])
        got = float(last["distillation_loss"])
        print(config, "step", i, "distillation", got, "float64", want, "relative deviation", abs(got - want) / want,
              "captioning", float(last["captioning_loss"]))
        assert want > 0 and abs(got - want) <= R.BAR * want
        cap, dist = last["captioning_loss"].cpu(), last["distillation_loss"].cpu()
        assert torch.equal(R.bits(last["total_loss"]), R.bits(cap + 0.01 * dist)) and torch.equal(last["total_loss"], loss.detach())
        assert torch.isfinite(loss)
        for n, p in student.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert all(p.grad is None for p in teacher.parameters()), "the teacher runs under no_grad"
    for h in hooks:
        h.remove()


@pytest.mark.parametrize("w", [1.0, 0.0])
def test_the_ends_of_the_ema_weight(w):
    from care_amd import InterplayStep

    opt = _opt("msrvtt_base_ami", ema_weight=w)
    batch = _batch(opt)
    student = _model(opt, 1)
    step = InterplayStep(opt, student)
    t0, s0 = _snapshot(step.teacher_captioner), _snapshot(student)
    step.training_step(batch)
    assert not _same_bits(student.parameters(), s0), "the optimiser must have moved the student"
    if w == 1.0:
        assert _same_bits(step.teacher_captioner.parameters(), t0)
    else:
        assert all(torch.equal(t.detach(), s.detach()) for t, s in zip(step.teacher_captioner.parameters(), student.parameters()))


def _capture_logits_grad(model, into):
    """The TOTAL gradient that reaches the logits of the next forward (autograd sums a tensor's consumers before its hooks run)."""
    def hook(mod, args, out):
        out["logits"].register_hook(lambda g: into.append(g.detach().clone()))

    return model.register_forward_hook(hook)


def test_student_gradients_with_identical_weights():
    """Teacher = student (weights), no dropout, ema_weight 1, distillation_weight 0.5: the distillation term is exactly 0 and its
    gradient exactly zero, so what reaches the student's logits is, bit for bit, the gradient of a criterion-only step on a third
    copy with the same weights and batch - and with it the vocabulary head's weight gradient, one ordered GEMM further on.

    The training FORWARD is bit-reproducible between two modules with equal weights (asserted first: the test relies on it).
    The training BACKWARD behind the head is not, run to run: care_ln_bwd (dgamma, dbeta), care_scatter_add_rows and the attention
    bias gradient add with floating-point atomics (csrc/backward.hip).  Measured on an MI355X: with bit-equal logits and a
    bit-equal gradient at the logits, the gradient of encoder.Encoder_A.1.weight (a LayerNorm weight) differed from the criterion-only
    run's in one element, by one unit in the last place.  So the remaining parameters are not compared bit for bit here: their
    gradients are the same kernels over the same bits, in an order of summation no two runs share."""
    from care_amd import InterplayStep, get_criterion

    opt = _opt("msrvtt_care", ema_weight=1.0, distillation_weight=0.5, **NO_DROP)
    batch = _batch(opt)
    student = _model(opt, 1)
    teacher, third = _model(opt, 2, like=student), _model(opt, 3, like=student)
    step = InterplayStep(opt, student, teacher=teacher)
    s_logits, t_logits, s_grad, c_logits, c_grad = [], [], [], [], []
    hooks = [_capture_logits(student, s_logits), _capture_logits(teacher, t_logits), _capture_logits_grad(student, s_grad)]
    step.training_step(batch)
    for h in hooks:
        h.remove()
    assert torch.equal(R.bits(s_logits[0]), R.bits(t_logits[0])), \
        "the training forward is not bit-reproducible between two modules with equal weights: this test relies on it"
    assert float(step.last["distillation_loss"]) == 0.0
    assert torch.equal(R.bits(step.last["total_loss"]), R.bits(step.last["captioning_loss"]))
    hooks = [_capture_logits(third, c_logits), _capture_logits_grad(third, c_grad)]
    criterion = get_criterion(opt, override_opt={"calculate_mAP": False})
    criterion.get_loss({**third(batch, current_epoch=0), **batch}).backward()
    for h in hooks:
        h.remove()
    assert torch.equal(R.bits(c_logits[0]), R.bits(s_logits[0]))
    assert len(s_grad) == len(c_grad) == 1 and bool((c_grad[0] != 0).any())
    assert torch.equal(R.bits(s_grad[0]), R.bits(c_grad[0])), "the distillation term moved the gradient at the student's logits"
    head_s, head_c = student.cls_head.tgt_word_prj.weight.grad, third.cls_head.tgt_word_prj.weight.grad
    assert head_s is not None and bool((head_s != 0).any()) and torch.equal(R.bits(head_s), R.bits(head_c))
    checked = 0
    for (n, p), q in zip(student.named_parameters(), third.named_parameters()):
        if p.requires_grad:
            assert p.grad is not None and q[1].grad is not None and bool(torch.isfinite(p.grad).all()), n
            checked += 1
    assert checked >= 40


def _encoded(model, batch):
    out = model.encoding_phase(batch["feats"])
    flat = []
    for k in sorted(out):
        for v in (out[k] if isinstance(out[k], (list, tuple)) else [out[k]]):
            if isinstance(v, torch.Tensor):
                flat.append(v.detach().clone())
    assert flat
    return flat


def test_evaluating_decodes_with_the_updated_teacher():
    from care_amd import InterplayStep, get_framework, get_translator

    opt = _opt("msrvtt_care", ema_weight=0.5, **NO_DROP)
    batch = _batch(opt)
    student = _model(opt, 1)
    step = InterplayStep(opt, student)
    teacher = step.teacher_captioner
    initial = copy.deepcopy({k: v.detach().cpu() for k, v in teacher.state_dict().items()})
    teacher.eval()
    before = _encoded(teacher, batch)        # the teacher's engine now holds its INITIAL weights
    teacher.train()
    step.training_step(batch)

    def fresh(state):
        m = get_framework(opt)
        m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
        return m.to(DEV).eval()

    tr = get_translator(opt)
    with step.evaluating():
        assert step.captioner is teacher and step.teacher_captioner is student
        student.eval(), teacher.eval()
        hyps = tr.translate_batch([step.captioner], batch)
        now = _encoded(step.captioner, batch)
    assert step.captioner is student and step.teacher_captioner is teacher
    current = fresh({k: v.detach().cpu() for k, v in teacher.state_dict().items()})
    want = _encoded(current, batch)
    assert len(now) == len(want) and all(torch.equal(a, b) for a, b in zip(now, want)), "the teacher decoded with stale weights"
    assert hyps == get_translator(opt).translate_batch([current], batch)
    old = _encoded(fresh(initial), batch)
    assert all(torch.equal(a, b) for a, b in zip(before, old))
    assert any(not torch.equal(a, b) for a, b in zip(now, old)), "one step at ema_weight 0.5 did not move the encoder's output"


def test_the_fused_head_is_refused_by_name():
    from care_amd import InterplayStep

    opt = _opt("msrvtt_base_ami")
    batch = _batch(opt)
    student = _model(opt, 1)
    step = InterplayStep(opt, student)
    student.set_fused_head(True)
    s0, t0 = _snapshot(student), _snapshot(step.teacher_captioner)
    with pytest.raises(NotImplementedError, match="fused head"):
        step.training_step(batch)
    assert _same_bits(student.parameters(), s0) and _same_bits(step.teacher_captioner.parameters(), t0)
    student.set_fused_head(False)
    assert torch.isfinite(step.training_step(batch))

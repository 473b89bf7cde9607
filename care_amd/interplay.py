"""The mean-teacher training step of train.py's `--wrapper InterplayModel` on the MI355X (csrc/interplay.hip).

    from care_amd.interplay import InterplayStep, distillation_mse, ema_update

The reference's second training wrapper (opts.py:26, models/Wrapper.py:550-614; its options at opts.py:253-255) trains a student
with the usual criterion plus a distillation term towards a teacher, `((student_logits - teacher_logits) ** 2).mean()` weighted
by `distillation_weight`, and after every optimiser step moves each teacher parameter towards the student's by an exponential
moving average with `ema_weight`; validation and test run on the teacher (`eval_model`).  Here the distillation term is two
sweeps over the logits (`care_mse_fwd`, and `care_mse_bwd` which recomputes the difference: nothing of logits size is kept
between forward and backward) and the average is ONE sweep over all parameter tensors (`care_ema_step`), the tensor list
travelling in the kernel's arguments.  Nothing in a step waits for the GPU.

The average has torch's bits: per element `t = fl(fl(t w) + fl(s (1 - w)))` in fp32, what `torch._foreach_mul_(t, w)`,
`torch._foreach_mul(s, 1 - w)` and `torch._foreach_add_` compute.  The distillation term takes the difference in fp32 as torch
does and sums its squares in double, in a fixed order: the same logits give the same bits.

As everywhere in care_amd there is no CPU fallback: CPU tensors raise.  The distillation term is over all N t V logits, which a
student with `set_fused_head(True)` never materialises: a `DeferredLogits` is refused by name.
"""
import contextlib

import torch

from . import _lib
from .criterion import DeferredLogits

__all__ = ["InterplayStep", "distillation_mse", "ema_update"]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


class _MSE(torch.autograd.Function):
    """mean((a - b)^2); the gradient goes to `a` only."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32c(a), _f32c(b)
        n = a.numel()
        partials = torch.empty(_lib.load().care_mse_partials(n), dtype=torch.float64, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            _lib.call("care_mse_fwd", _lib.ptr(a), _lib.ptr(b), n, _lib.ptr(partials), _lib.ptr(loss), tag="mse_fwd")
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernel reads it, the host never does
        da = torch.empty(a.shape, dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            _lib.call("care_mse_bwd", _lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(g), _lib.ptr(da), tag="mse_bwd")
        return da, None


def _refuse_deferred(what, t) -> None:
    if isinstance(t, DeferredLogits):
        raise NotImplementedError(
            "`{}` is a DeferredLogits: the fused head (set_fused_head(True)) never materialises the [N, t, V] logits the "
            "distillation term is taken over - call set_fused_head(False) on the module".format(what))


def distillation_mse(student_logits, teacher_logits) -> torch.Tensor:
    """Wrapper.py:565: `((student_logits - teacher_logits) ** 2).mean()` as a 0-dim fp32 device tensor; under autograd the
    gradient goes to the student's logits only."""
    for what, t in (("student_logits", student_logits), ("teacher_logits", teacher_logits)):
        _refuse_deferred(what, t)
        if not isinstance(t, torch.Tensor):
            raise TypeError("`{}` must be a tensor, got {}".format(what, type(t).__name__))
    if tuple(student_logits.shape) != tuple(teacher_logits.shape):
        raise ValueError("student_logits {} and teacher_logits {} differ in shape".format(tuple(student_logits.shape),
                                                                                          tuple(teacher_logits.shape)))
    for what, t in (("student_logits", student_logits), ("teacher_logits", teacher_logits)):
        if t.device.type != "cuda":
            raise RuntimeError("`{}` is on `{}`: the distillation term runs on the MI355X (no CPU fallback)".format(what, t.device))
    if teacher_logits.device != student_logits.device:
        raise RuntimeError("student_logits are on `{}`, teacher_logits on `{}`".format(student_logits.device, teacher_logits.device))
    if student_logits.numel() == 0:
        raise ValueError("the distillation term of empty logits {} is undefined".format(tuple(student_logits.shape)))
    return _MSE.apply(student_logits, teacher_logits.detach())


@torch.no_grad()
def ema_update(teacher_params, student_params, ema_weight) -> None:
    """Wrapper.py:574-581: every teacher tensor becomes `ema_weight * teacher + (1 - ema_weight) * student`, with the bits of
    torch's three `_foreach` calls, as one `care_ema_step` over the whole list.  Everything is checked before the launch."""
    teacher, student = list(teacher_params), list(student_params)
    w = float(ema_weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError("Invalid ema_weight: {} (0 <= ema_weight <= 1)".format(ema_weight))
    if len(teacher) != len(student):
        raise ValueError("{} teacher tensors against {} student tensors".format(len(teacher), len(student)))
    for i, (t, s) in enumerate(zip(teacher, student)):
        if t is s or (t.numel() and t.data_ptr() == s.data_ptr()):
            raise ValueError("tensor {} is paired with itself: teacher and student must be distinct".format(i))
        if t.numel() != s.numel():
            raise ValueError("tensor {}: teacher {} and student {} differ in size".format(i, tuple(t.shape), tuple(s.shape)))
        if t.dtype != torch.float32 or s.dtype != torch.float32:
            raise NotImplementedError("tensor {}: parameters must be fp32, got {} / {}".format(i, t.dtype, s.dtype))
        if not t.is_contiguous() or not s.is_contiguous():
            raise NotImplementedError("tensor {} of shape {} is not contiguous: the HIP moving average walks contiguous fp32 "
                                      "storage".format(i, tuple(t.shape)))
    if not teacher:
        return
    device = teacher[0].device
    for i, (t, s) in enumerate(zip(teacher, student)):
        if t.device.type != "cuda" or s.device.type != "cuda":
            raise RuntimeError("tensor {} is on `{}` / `{}`: the moving average runs on the MI355X (no CPU fallback)".format(
                i, t.device, s.device))
        if t.device != device or s.device != device:
            raise NotImplementedError("tensor {} is on `{}` / `{}`, the first on `{}`: one device per update".format(
                i, t.device, s.device, device))
    live = [(t, s) for t, s in zip(teacher, student) if t.numel()]
    descs = (_lib.EmaTensor * max(1, len(live)))()
    for d, (t, s) in zip(descs, live):
        d.t, d.s, d.n = t.data_ptr(), s.data_ptr(), t.numel()
    with torch.cuda.device(device):
        _lib.call("care_ema_step", descs, len(live), w, 1 - w, tag="ema_step")
    # the kernel wrote through raw pointers: TransformerSeq2Seq.engine() re-packs its weights and drops its captured graphs
    # when a parameter's _version moved - without this the teacher would decode with the weights of its last evaluation
    torch.autograd.graph.increment_version(teacher)


class InterplayStep(object):
    """`InterplayModel` (models/Wrapper.py:550-614) without Lightning: a student `captioner`, a `teacher` of the same
    architecture, the criterion, the optimiser of the student and its scheduler.

    `teacher` defaults to a freshly initialised `get_framework(opt)` on the student's device - as in the reference an
    independent random initialisation, not a copy of the student."""

    def __init__(self, opt, captioner, criterion=None, optimizer=None, scheduler=None, teacher=None):
        from .criterion import get_criterion
        from .framework import get_framework
        from .optim import configure_optimizers

        self.opt = opt
        self.captioner = captioner
        self.criterion = criterion if criterion is not None else get_criterion(opt, override_opt={"calculate_mAP": False})
        if optimizer is None:
            built = configure_optimizers(opt, captioner)
            optimizer = built["optimizer"]
            if scheduler is None:
                scheduler = built["lr_scheduler"]["scheduler"]
        self.optimizer, self.scheduler = optimizer, scheduler
        if teacher is None:
            teacher = get_framework(opt)
            p = next(captioner.parameters(), None)
            if p is not None:
                teacher.to(p.device)
            teacher.train(captioner.training)
        self.teacher_captioner = teacher
        self.last = {}

    @property
    def distillation_weight(self) -> float:
        return self.opt.get("distillation_weight", 0.01)

    @property
    def ema_weight(self) -> float:
        return self.opt.get("ema_weight", 0.999)

    @property
    def eval_model(self) -> str:
        return self.opt.get("eval_model", "teacher")

    def training_step(self, batch, current_epoch=0):
        """Wrapper.py:557-586.  Returns the loss; `last` holds captioning_loss, distillation_loss and total_loss as device
        scalars (the reference logs them) - reading one is the caller's synchronisation."""
        student_results = self.captioner(batch, current_epoch=current_epoch)
        _refuse_deferred("student_logits", student_results["logits"])   # before the criterion's recorders see the batch
        captioning_loss = self.criterion.get_loss({**student_results, **batch})
        with torch.no_grad():
            teacher_results = self.teacher_captioner(batch, current_epoch=current_epoch)
        distillation_loss = distillation_mse(student_results["logits"], teacher_results["logits"])
        loss = captioning_loss + self.distillation_weight * distillation_loss
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        ema_update(self.teacher_captioner.parameters(), self.captioner.parameters(), self.ema_weight)
        self.last = {"captioning_loss": captioning_loss.detach(), "distillation_loss": distillation_loss.detach(),
                     "total_loss": loss.detach()}
        return loss

    def swap_captioners(self) -> None:
        """Wrapper.py:604-606: student and teacher change places when the teacher is the model to evaluate."""
        if self.eval_model == "teacher":
            self.teacher_captioner, self.captioner = self.captioner, self.teacher_captioner

    @contextlib.contextmanager
    def evaluating(self):
        """The on_validation / on_test _epoch_start and _epoch_end hooks (Wrapper.py:588-602): inside the block `captioner` is
        the model to evaluate; the pair is back afterwards, also when the block raises."""
        self.swap_captioners()
        try:
            yield self
        finally:
            self.swap_captioners()

    def training_epoch_end(self) -> None:
        """Wrapper.py:608-611: the scheduler is stepped by hand (manual optimisation)."""
        if self.scheduler is not None:
            self.scheduler.step()

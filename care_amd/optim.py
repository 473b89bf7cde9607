"""The optimiser step of train.py on the MI355X: Adam with the gradient clipping folded in (csrc/optim.hip).

    from care_amd.optim import Adam, configure_optimizers, filter_weight_decay

The reference builds `torch.optim.Adam` in `Wrapper.configure_optimizers` (models/Wrapper.py:316-386), has Lightning clip the
gradients with `gradient_clip_val` (train.py:128, opts.py:145: `clip_grad_norm_`, norm type 2) and groups the parameters for
weight decay in misc/utils.py:282-304.  Here the update of ALL parameter tensors is one sweep (`care_adam_step`) and, with
`max_grad_norm > 0`, the norm of all gradients one more (`care_grad_sqnorm`); the clipping coefficient is read from the
device inside the update, so a step never waits for the GPU and uploads nothing: the tensor list travels in the kernels'
arguments.

`Adam` is a `torch.optim.Optimizer`: torch's schedulers drive it through `param_groups[i]['lr']`, its state per parameter is
torch's (`step`, `exp_avg`, `exp_avg_sq`) and its `state_dict()` loads into `torch.optim.Adam` and the reverse, so a run can
move between the two mid-training.  The arithmetic per element is torch 2.10's `_single_tensor_adam` in fp32.

ONE visible difference from `clip_grad_norm_` + `torch.optim.Adam`: `.grad` is read and never written, so after a clipped step
it still holds the UNSCALED gradient (clip_grad_norm_ scales it in place).  `last_grad_norm` is the norm before clipping, as
clip_grad_norm_ returns it - a one-element device tensor; reading it is the caller's synchronisation.

As everywhere in care_amd there is no CPU fallback: CPU parameters raise.  What the kernels do not cover is refused by name
before anything is launched: amsgrad, maximize, capturable, differentiable, sparse gradients, parameters that are not
contiguous fp32.  Out of scope: AdamW's decoupled decay, master weights, graph capture of the step.
"""
import ctypes
import math

import torch

from . import _lib

_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")
_REFUSALS = {
    "amsgrad": "`amsgrad` (torch/optim/adam.py: the running maximum of exp_avg_sq) is not covered by the HIP optimiser step",
    "maximize": "`maximize` (ascent on the negated gradient) is not covered by the HIP optimiser step",
    "capturable": "`capturable` (device-side step counts for graph capture) is not covered by the HIP optimiser step: the step "
                  "count is a host integer",
    "differentiable": "`differentiable` (autograd through the update) is not covered by the HIP optimiser step: the kernels "
                      "write through raw pointers",
}


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, amsgrad = maximize = False) with Lightning's gradient_clip_val as `max_grad_norm`
    (0 = no clipping), over all parameters of the optimiser."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=0.0, amsgrad=False,
                 maximize=False, capturable=False, differentiable=False):
        for name, value in zip(_REFUSED_FLAGS, (amsgrad, maximize, capturable, differentiable)):
            if value:
                raise NotImplementedError(_REFUSALS[name])
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("a tensor `lr` (torch keeps it for capturable steps) is not covered: pass a float")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if not 0.0 <= max_grad_norm:
            raise ValueError("Invalid max_grad_norm value: {}".format(max_grad_norm))
        # every key torch.optim.Adam's groups carry, so that a state dict of this class steps in torch's unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self.max_grad_norm = float(max_grad_norm)   # of the optimiser, not of a group: one norm over all parameters
        self.last_grad_norm = None
        self._partials = None

    def __getstate__(self):
        state = super().__getstate__()
        state["max_grad_norm"] = self.max_grad_norm
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", 0.0)
        self.__dict__.setdefault("last_grad_norm", None)
        self.__dict__.setdefault("_partials", None)
        # torch keeps `step` as a tensor; here it is a host integer (read once, at load - never in a step)
        for st in self.state.values():
            if "step" in st and not isinstance(st["step"], int):
                st["step"] = int(round(float(st["step"])))

    def state_dict(self):
        """torch.optim.Adam's layout: `step` as a float32 CPU scalar tensor, `exp_avg`, `exp_avg_sq`."""
        sd = super().state_dict()
        sd["state"] = {k: {kk: (torch.tensor(float(vv), dtype=torch.float32) if kk == "step" else vv) for kk, vv in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    # ------------------------------------------------------------------ the step
    def _collect(self):
        """Every check of a step, before state is touched or anything is launched: [(param, grad, group)]."""
        todo = []
        for group in self.param_groups:
            for name in _REFUSED_FLAGS:
                if group.get(name, False):
                    raise NotImplementedError(_REFUSALS[name])
            if group.get("decoupled_weight_decay", False):
                raise NotImplementedError("`decoupled_weight_decay` (AdamW) is not covered by the HIP optimiser step")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError("a tensor `lr` is not covered by the HIP optimiser step: set a float")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("sparse gradients (torch.optim.SparseAdam's case) are not covered by the HIP optimiser step")
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise NotImplementedError("parameters and gradients must be fp32, got {} / {} (mixed-precision master weights "
                                              "are not covered)".format(p.dtype, g.dtype))
                if not p.is_contiguous():
                    raise NotImplementedError("a parameter of shape {} with strides {} is not contiguous: the HIP optimiser step "
                                              "walks contiguous fp32 storage".format(tuple(p.shape), p.stride()))
                if p.device.type != "cuda":
                    raise RuntimeError("a parameter is on `{}`: the optimiser step runs on the MI355X (no CPU fallback)".format(p.device))
                if g.device != p.device:
                    raise RuntimeError("a gradient is on `{}`, its parameter on `{}`".format(g.device, p.device))
                if p.numel() == 0:
                    continue
                todo.append((p, g if g.is_contiguous() else g.contiguous(), group))
        return todo

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = self._collect()
        if not todo:
            return loss
        device = todo[0][0].device
        if any(p.device != device for p, _, _ in todo):
            raise NotImplementedError("parameters on several devices: one optimiser per device (no gradient all-reduce here)")
        # launches: one per (betas, eps, step count) - one in all unless parameters were skipped in some steps
        descs = (_lib.OptTensor * len(todo))()
        buckets = {}
        for i, (p, g, group) in enumerate(todo):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if m.device != device or m.dtype != torch.float32 or not m.is_contiguous() or v.device != device or \
                    v.dtype != torch.float32 or not v.is_contiguous() or m.numel() != p.numel() or v.numel() != p.numel():
                raise RuntimeError("optimiser state of a parameter of shape {} is not contiguous fp32 on {}".format(tuple(p.shape), device))
            st["step"] = t = st["step"] + 1
            beta1, beta2 = group["betas"]
            d = descs[i]
            d.p, d.g, d.m, d.v, d.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            d.step_size = float(group["lr"]) / (1.0 - beta1 ** t)
            d.weight_decay = group["weight_decay"]
            buckets.setdefault((float(beta1), float(beta2), float(group["eps"]), t), []).append(i)
        with torch.cuda.device(device):
            norm = None
            if self.max_grad_norm > 0:
                total = sum(p.numel() for p, _, _ in todo)
                need = _lib.load().care_grad_sqnorm_partials(total)
                if self._partials is None or self._partials.device != device or self._partials.numel() < need:
                    self._partials = torch.empty(need, dtype=torch.float64, device=device)
                self.last_grad_norm = norm = torch.empty(1, dtype=torch.float32, device=device)
                _lib.call("care_grad_sqnorm", descs, len(todo), _lib.ptr(self._partials), _lib.ptr(norm), tag="grad_sqnorm")
            for (beta1, beta2, eps, t), idx in buckets.items():
                if len(buckets) == 1:
                    part = descs
                else:
                    part = (_lib.OptTensor * len(idx))()
                    for j, i in enumerate(idx):
                        ctypes.memmove(ctypes.byref(part[j]), ctypes.byref(descs[i]), ctypes.sizeof(_lib.OptTensor))
                _lib.call("care_adam_step", part, len(idx), beta1, beta2, eps, math.sqrt(1.0 - beta2 ** t), _lib.ptr(norm),
                          self.max_grad_norm, tag="adam_step")
        # the kernels wrote through raw pointers: autograd's saved-tensor checks and TransformerSeq2Seq.engine() (which
        # re-packs weights and drops captured graphs when a parameter's _version moved) must see the write
        torch.autograd.graph.increment_version([p for p, _, _ in todo])
        return loss


def filter_weight_decay(model, weight_decay=1e-5, filter_biases=False, skip_list=(), skip_substr_list=()):
    """misc/utils.py:282-304: [{no decay}, {decay}] - trainable parameters that are one-dimensional (with `filter_biases`), named
    in `skip_list` or whose name contains an entry of `skip_substr_list` get weight_decay 0."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if (filter_biases and param.dim() == 1) or name in skip_list or any(s in name for s in skip_substr_list):
            no_decay.append(param)
        else:
            decay.append(param)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, last_epoch=-1):
    """misc/optim.py:5-34: the factor rises linearly from 0 to 1 over the warm-up steps, then falls linearly to 0 at
    `num_training_steps` (a torch LambdaLR)."""
    from torch.optim.lr_scheduler import LambdaLR

    def factor(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))

    return LambdaLR(optimizer, factor, last_epoch)


def configure_optimizers(opt, captioner, max_steps=None):
    """Wrapper.configure_optimizers (models/Wrapper.py:316-386) with `Adam` above in place of torch's: the same option keys and
    defaults, torch's own scheduler classes, the same dict.  `opt['gradient_clip_val']` (Lightning's, train.py:128) becomes
    `max_grad_norm`; `max_steps` stands in for `self.trainer.max_steps` in the cosine branch."""
    lr = opt.get("learning_rate", 5e-4)
    weight_decay = opt.get("weight_decay", 5e-4)
    clip = float(opt.get("gradient_clip_val", 0.0) or 0.0)
    if opt.get("filter_weight_decay", False):
        parameters = filter_weight_decay(model=captioner, weight_decay=weight_decay, filter_biases=opt.get("filter_biases", False),
                                         skip_list=(), skip_substr_list=opt.get("skip_substr_list", []))
        optimizer = Adam(parameters, lr=lr, max_grad_norm=clip)
    else:
        optimizer = Adam(filter(lambda p: p.requires_grad, captioner.parameters()), lr=lr, weight_decay=weight_decay, max_grad_norm=clip)

    kind = opt.get("lr_scheduler_type", "linear")
    if kind == "linear":
        from torch.optim.lr_scheduler import StepLR
        scheduler = StepLR(optimizer, step_size=opt.get("lr_step_size", 1), gamma=opt.get("lr_decay", 0.9))
        other = {}
    elif kind == "cosine":
        from torch.optim.lr_scheduler import CosineAnnealingLR
        if max_steps is None:
            raise ValueError("lr_scheduler_type 'cosine' needs `max_steps` (the trainer's, Wrapper.py:344)")
        scheduler = CosineAnnealingLR(optimizer, T_max=max_steps, eta_min=opt.get("min_lr", 1e-6))
        other = {"interval": "step"}
    elif kind == "linear_with_warmup":
        if opt["learning_rate_warmup_ratio"]:
            warmup = int(opt["max_steps"] * opt["learning_rate_warmup_ratio"])
        else:
            warmup = opt["learning_rate_warmup_steps"]
        scheduler = linear_schedule_with_warmup(optimizer, num_warmup_steps=warmup, num_training_steps=opt["max_steps"])
        other = {"interval": "step"}
    else:
        from torch.optim.lr_scheduler import ReduceLROnPlateau
        scheduler = ReduceLROnPlateau(optimizer, mode=opt.get("lr_monitor_mode", "max"), factor=opt.get("lr_decay", 0.9),
                                      patience=opt.get("lr_monitor_patience", 1), min_lr=opt.get("min_lr", 1e-6))
        other = {"monitor": opt.get("lr_monitor_metric", "CIDEr"), "strict": True}
    return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "interval": "epoch", "frequency": 1, **other}}

"""The yardsticks of the mean-teacher tests, restated in our own words (models/Wrapper.py:550-614 is ten lines of torch calls):
the moving average as torch's three `_foreach` calls on CPU clones - the kernel must reproduce their BITS - and the
distillation term with its gradient in float64 from the fp32 inputs."""
import torch

# |got - ref64| <= BAR * |ref64| for the loss and for every non-zero gradient element.  The fp32 difference carries one
# rounding (2^-24 relative); its square twice that; every term is non-negative, so the sum carries at most 2^-23; the
# double sums add nothing visible; the narrowing to fp32 adds 2^-24: 3 * 2^-24, and the bar is the next power of two.  The
# gradient has three roundings (the difference, the coefficient, the product): the same bar.
BAR = 4 * 2.0 ** -24


def ema_reference(teacher_list, student_list, w):
    """New teacher tensors (CPU, fp32): `_foreach_mul_(t, w)`, `_foreach_mul(s, 1 - w)`, `_foreach_add_` on clones."""
    t = [x.detach().cpu().clone() for x in teacher_list]
    s = [x.detach().cpu().clone() for x in student_list]
    if not t:
        return t
    torch._foreach_mul_(t, w)
    torch._foreach_add_(t, torch._foreach_mul(s, 1 - w))
    return t


def mse_reference64(a, b):
    """mean((a - b)^2) as a Python float, in float64 from the fp32 values."""
    d = a.detach().cpu().double().reshape(-1) - b.detach().cpu().double().reshape(-1)
    return float((d * d).sum() / d.numel())


def mse_grad_reference64(a, b, g):
    """d mean((a - b)^2) / d a times the upstream gradient g, float64 [same shape as a]."""
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
    return (a64 - b64) * (2.0 * float(g) / a64.numel())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)

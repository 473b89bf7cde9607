"""The yardstick of the optimiser tests: a float64 restatement of the optimiser step's formulas (include/care_hip.h, "The
optimiser step") - the gradient norm, clip_grad_norm_'s coefficient and torch.optim.Adam's update - and the trajectory
recipe the CPU and the GPU tests share.  tests/test_optim_cpu.py pins it to torch.optim.Adam + clip_grad_norm_ on float64
tensors; tests/test_gpu_optim.py measures the HIP kernels against it.  No test imports the reference.
"""
import math

import numpy as np
import torch

SIZES = [1, 3, 4, 5, 500, 912, 1023, 1025, 65537, 300001]
OFFSET_VIEW = 777          # one more tensor: a view at storage offset 1 of a larger buffer (not 16-byte aligned)
BASE_LR, ODD_LR, ODD_WD, MAX_NORM = 5e-4, 2e-4, 1e-3, 5.0
BETAS, EPS = (0.9, 0.999), 1e-8


def grad_norm(grads):
    """L2 norm of all gradients together (float64)."""
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient: max_norm / (norm + 1e-6), at most 1."""
    c = max_norm / (norm + 1e-6)
    return c if c < 1.0 else (1.0 if c == c else c)


def adam_update(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, c=1.0):
    """One step of one tensor, float64 numpy arrays; returns the new (p, m, v).  t: the step count AFTER this step."""
    g = c * g
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1.0 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** t)
    bias2_sqrt = math.sqrt(1.0 - beta2 ** t)
    p = p - step_size * m / (np.sqrt(v) / bias2_sqrt + eps)
    return p, m, v


class RefAdam:
    """float64 Adam over a list of tensors with per-tensor (lr, weight_decay) and one clipping norm over all of them."""

    def __init__(self, params, lrs, wds, betas=BETAS, eps=EPS, max_grad_norm=0.0):
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.lrs, self.wds, self.betas, self.eps, self.max_grad_norm = list(lrs), list(wds), betas, eps, max_grad_norm
        self.last_grad_norm = None

    def step(self, grads):
        """grads[i] None: tensor i is skipped (no state change, no step count)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        c = 1.0
        if self.max_grad_norm > 0:
            self.last_grad_norm = grad_norm([grads[i] for i in live])
            c = clip_coef(self.last_grad_norm, self.max_grad_norm)
        for i in live:
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = adam_update(self.p[i], np.asarray(grads[i], dtype=np.float64), self.m[i], self.v[i],
                                                          self.t[i], self.lrs[i], self.betas[0], self.betas[1], self.eps,
                                                          self.wds[i], c)


# ------------------------------------------------------------------ the trajectory recipe
def recipe_params(seed=0):
    """The tensor list of the tests as float32 CPU tensors: SIZES, uniform in [-0.5, 0.5), + the OFFSET_VIEW tensor."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, generator=g) - 0.5 for n in SIZES + [OFFSET_VIEW]]


def recipe_grads(step, seed=0, scales=(1e-3, 10.0)):
    """Seeded gradients of step `step` (0-based): N(0, 1) times scales[step % 2] - 1e-3 (clipping idle) and 10 (active)."""
    g = torch.Generator().manual_seed(1000 * (seed + 1) + step)
    s = scales[step % len(scales)]
    return [torch.randn(n, generator=g) * s for n in SIZES + [OFFSET_VIEW]]


def recipe_groups(n):
    """Two groups: even indices with weight_decay 0 (base lr), odd indices with weight_decay 1e-3 and lr 2e-4."""
    even, odd = [i for i in range(n) if i % 2 == 0], [i for i in range(n) if i % 2 == 1]
    lrs = [BASE_LR if i % 2 == 0 else ODD_LR for i in range(n)]
    wds = [0.0 if i % 2 == 0 else ODD_WD for i in range(n)]
    return even, odd, lrs, wds


def torch_groups(params):
    even, odd, _, _ = recipe_groups(len(params))
    return [{"params": [params[i] for i in even], "weight_decay": 0.0},
            {"params": [params[i] for i in odd], "weight_decay": ODD_WD, "lr": ODD_LR}]


def run_reference(steps, max_grad_norm=MAX_NORM, seed=0, scales=(1e-3, 10.0)):
    params = recipe_params(seed)
    _, _, lrs, wds = recipe_groups(len(params))
    ref = RefAdam([p.numpy() for p in params], lrs, wds, max_grad_norm=max_grad_norm)
    norms = []
    for s in range(steps):
        ref.step([g.numpy() for g in recipe_grads(s, seed, scales)])
        norms.append(ref.last_grad_norm)
    return ref, norms


def run_torch(steps, dtype, max_grad_norm=MAX_NORM, seed=0, scales=(1e-3, 10.0)):
    """torch.optim.Adam + clip_grad_norm_ on CPU tensors of `dtype`: (params, optimiser, norms)."""
    params = [torch.nn.Parameter(p.to(dtype)) for p in recipe_params(seed)]
    optim = torch.optim.Adam(torch_groups(params), lr=BASE_LR, betas=BETAS, eps=EPS)
    norms = []
    for s in range(steps):
        for p, g in zip(params, recipe_grads(s, seed, scales)):
            p.grad = g.to(dtype)
        if max_grad_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_grad_norm)))
        optim.step()
    return params, optim, norms


def deviations(ref, params, exp_avg, exp_avg_sq):
    """Largest deviation from the float64 run: absolute over parameters and exp_avg, relative over exp_avg_sq."""
    dp = max(float(np.abs(np.asarray(p, dtype=np.float64).reshape(-1) - r).max()) for p, r in zip(params, ref.p))
    dm = max(float(np.abs(np.asarray(m, dtype=np.float64).reshape(-1) - r).max()) for m, r in zip(exp_avg, ref.m))
    dv = max(float((np.abs(np.asarray(v, dtype=np.float64).reshape(-1) - r) / np.maximum(r, 1e-300)).max()) for v, r in zip(exp_avg_sq, ref.v))
    return dp, dm, dv


def torch_fp32_bound(steps, **kw):
    """The tolerance of the GPU tests, MEASURED: torch's own float32 run of the recipe against float64, doubled, plus one
    float32 ulp of the largest parameter magnitude (absolute: parameters, exp_avg) / of 1 (relative: exp_avg_sq, the norm).
    The factor of two covers another summation order in the norm and fused multiply-adds - one rounding per operation."""
    ref, ref_norms = run_reference(steps, **kw)
    params, optim, norms = run_torch(steps, torch.float32, **kw)
    st = [optim.state[p] for p in params]
    dp, dm, dv = deviations(ref, [p.detach().numpy() for p in params], [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st])
    dn = max([abs(a - b) / b for a, b in zip(norms, ref_norms)] or [0.0])
    ulp = 2.0 ** -23
    pmax = max(float(np.abs(p).max()) for p in ref.p)
    mmax = max(float(np.abs(m).max()) for m in ref.m)
    return {"param": 2 * dp + ulp * pmax, "exp_avg": 2 * dm + ulp * mmax, "exp_avg_sq": 2 * dv + ulp, "norm": 2 * dn + ulp,
            "torch": {"param": dp, "exp_avg": dm, "exp_avg_sq": dv, "norm": dn}}

"""GPU: the optimiser step (csrc/optim.hip, care_amd/optim.py) against the float64 restatement of tests/optim_reference.py.

The tolerance is MEASURED, not chosen: torch.optim.Adam + clip_grad_norm_ run the same recipe on float32 CPU tensors, and
the HIP result may deviate from float64 by at most twice what torch's does, plus one float32 ulp of the largest magnitude
(optim_reference.torch_fp32_bound).  The tensor list has the sizes at which vector bodies, scalar tails, chunk boundaries and
launch splitting can go wrong, one tensor at an odd storage offset among them."""
import math

import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64           # sentinel floats in front of and behind every buffer
SENTINEL = -7.25
T_STEP = 3         # the step count of the by-name update


@pytest.fixture(scope="module")
def bound10():
    b = R.torch_fp32_bound(10)
    print("torch fp32 vs float64, 10 steps:", b["torch"])
    return b


def _guarded(values, misaligned=False):
    """A device buffer of 64 sentinels | (one more float when `misaligned`) values | 64 sentinels; returns (whole, view)."""
    v = torch.as_tensor(np.asarray(values), dtype=torch.float32).reshape(-1)
    off = PAD + (1 if misaligned else 0)
    whole = torch.full((off + v.numel() + PAD,), SENTINEL, dtype=torch.float32)
    whole[off:off + v.numel()] = v
    whole = whole.to(DEV)
    view = whole[off:off + v.numel()]
    assert (view.data_ptr() % 16 != 0) == misaligned
    return whole, view


def _sentinels_intact(whole, n, misaligned=False):
    off = PAD + (1 if misaligned else 0)
    w = whole.cpu()
    return bool((w[:off] == SENTINEL).all()) and bool((w[off + n:] == SENTINEL).all())


def _descs(ps, gs, ms, vs, step_sizes, wds):
    from care_amd import _lib

    d = (_lib.OptTensor * len(ps))()
    for i in range(len(ps)):
        d[i].p, d[i].g, d[i].m, d[i].v, d[i].n = ps[i].data_ptr(), gs[i].data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), ps[i].numel()
        d[i].step_size, d[i].weight_decay = step_sizes[i], wds[i]
    return d


def _norm_of(d, count, total):
    from care_amd import _lib

    partials = torch.full((_lib.load().care_grad_sqnorm_partials(total),), float("nan"), dtype=torch.float64, device=DEV)
    norm = torch.full((1,), float("nan"), device=DEV)
    _lib.call("care_grad_sqnorm", d, count, partials.data_ptr(), norm.data_ptr())
    return norm


def test_grad_sqnorm_by_name(bound10):
    from care_amd import _lib

    grads = R.recipe_grads(1)
    mis = [i == len(grads) - 1 for i in range(len(grads))]
    held = [_guarded(g.numpy(), m) for g, m in zip(grads, mis)]
    views = [v for _, v in held]
    d = _descs(views, views, views, views, [0.0] * len(views), [0.0] * len(views))     # p, m, v: anything non-NULL, never touched
    total = sum(g.numel() for g in grads)
    want = R.grad_norm([g.numpy() for g in grads])
    a, b = _norm_of(d, len(views), total), _norm_of(d, len(views), total)
    got = float(a)
    print("norm", got, "float64", want, "relative deviation", abs(got - want) / want, "bound", bound10["norm"])
    assert abs(got - want) <= bound10["norm"] * want
    assert a.view(torch.int32).item() == b.view(torch.int32).item(), "two calls must give the same bits"
    for (whole, view), g, m in zip(held, grads, mis):
        assert _sentinels_intact(whole, g.numel(), m) and torch.equal(view.cpu(), g)
    # more tensors than one launch holds: 80 tensors of 5 elements
    g80 = torch.Generator().manual_seed(80)
    small = [(torch.randn(5, generator=g80) * 3).to(DEV) for _ in range(80)]
    assert len(small) > 64
    d80 = _descs(small, small, small, small, [0.0] * 80, [0.0] * 80)
    want80 = R.grad_norm([s.cpu().numpy() for s in small])
    assert abs(float(_norm_of(d80, 80, 400)) - want80) <= bound10["norm"] * want80
    assert float(_norm_of(None, 0, 0)) == 0.0
    # a list that fills the grid cap: every workgroup walks several chunks, across tensor boundaries
    gb = torch.Generator().manual_seed(81)
    big = [torch.randn(n, generator=gb) for n in (1500001, 5, 700003)]
    bigd = [b_.to(DEV) for b_ in big]
    total = sum(b_.numel() for b_ in big)
    assert _lib.load().care_grad_sqnorm_partials(total) == 2048 and sum(-(-b_.numel() // 1024) for b_ in big) > 2048
    wantb = R.grad_norm([b_.numpy() for b_ in big])
    gotb = float(_norm_of(_descs(bigd, bigd, bigd, bigd, [0.0] * 3, [0.0] * 3), 3, total))
    assert abs(gotb - wantb) <= bound10["norm"] * wantb


@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_step_by_name(bound10, wd, with_norm):
    """One step from non-zero m and v over the whole list, against float64; sentinels around every buffer; g untouched."""
    from care_amd import _lib

    # gradients of 10 with the norm (the coefficient scales them to the trajectory's magnitudes), of 1e-3 without
    params, grads = R.recipe_params(5), R.recipe_grads(1 if with_norm else 0, seed=5)
    gen = torch.Generator().manual_seed(55)
    ms = [torch.randn(p.numel(), generator=gen) * 1e-3 for p in params]    # (the magnitudes of the trajectory the bound is measured on)
    vs = [torch.rand(p.numel(), generator=gen) * 1e-3 + 1e-8 for p in params]
    n = len(params)
    mis = [i == n - 1 for i in range(n)]
    hp, hg, hm, hv = ([_guarded(x.numpy(), m) for x, m in zip(xs, mis)] for xs in (params, grads, ms, vs))
    beta1, beta2 = R.BETAS
    lrs = [R.BASE_LR if i % 2 == 0 else R.ODD_LR for i in range(n)]
    d = _descs([v for _, v in hp], [v for _, v in hg], [v for _, v in hm], [v for _, v in hv],
               [lr / (1.0 - beta1 ** T_STEP) for lr in lrs], [wd] * n)
    norm64 = R.grad_norm([g.numpy() for g in grads])
    norm = torch.tensor([norm64], dtype=torch.float32, device=DEV) if with_norm else None
    c = R.clip_coef(float(np.float32(norm64)), R.MAX_NORM) if with_norm else 1.0
    assert not with_norm or c < 0.01
    _lib.call("care_adam_step", d, n, beta1, beta2, R.EPS, math.sqrt(1.0 - beta2 ** T_STEP), _lib.ptr(norm), R.MAX_NORM)
    torch.cuda.synchronize()
    for i in range(n):
        wp, wm, wv = R.adam_update(params[i].double().numpy(), grads[i].double().numpy(), ms[i].double().numpy(), vs[i].double().numpy(),
                                   T_STEP, lrs[i], beta1, beta2, R.EPS, wd, c)
        gp, gm, gv = hp[i][1].cpu().double().numpy(), hm[i][1].cpu().double().numpy(), hv[i][1].cpu().double().numpy()
        assert np.abs(gp - wp).max() <= bound10["param"], (i, np.abs(gp - wp).max())
        assert np.abs(gm - wm).max() <= bound10["exp_avg"], (i, np.abs(gm - wm).max())
        assert (np.abs(gv - wv) / wv).max() <= bound10["exp_avg_sq"], (i, (np.abs(gv - wv) / wv).max())
        assert np.abs(gp - params[i].double().numpy()).max() > 0, "the step must move the parameters"
        for held in (hp, hg, hm, hv):
            assert _sentinels_intact(held[i][0], params[i].numel(), mis[i]), i
        assert torch.equal(hg[i][1].cpu().view(torch.int32), grads[i].view(torch.int32)), "g is read, never written"


def test_adam_step_beyond_the_grid_cap_and_bad_arguments(bound10):
    from care_amd import _lib

    lib = _lib.load()
    gen = torch.Generator().manual_seed(91)
    sizes = (1500001, 5, 700003)     # 2151 chunks for 2048 workgroups: ranges of one and two chunks, across tensor boundaries
    ps = [torch.rand(n, generator=gen) - 0.5 for n in sizes]
    gs = [torch.randn(n, generator=gen) * 1e-3 for n in sizes]
    ms = [torch.randn(n, generator=gen) * 1e-3 for n in sizes]
    vs = [torch.rand(n, generator=gen) * 1e-3 + 1e-8 for n in sizes]
    hp, hg, hm, hv = ([_guarded(x.numpy()) for x in xs] for xs in (ps, gs, ms, vs))
    beta1, beta2 = R.BETAS
    d = _descs([v for _, v in hp], [v for _, v in hg], [v for _, v in hm], [v for _, v in hv], [R.BASE_LR / (1.0 - beta1 ** T_STEP)] * 3, [1e-3] * 3)
    _lib.call("care_adam_step", d, 3, beta1, beta2, R.EPS, math.sqrt(1.0 - beta2 ** T_STEP), None, 0.0)
    torch.cuda.synchronize()
    for i in range(3):
        wp, wm, wv = R.adam_update(ps[i].double().numpy(), gs[i].double().numpy(), ms[i].double().numpy(), vs[i].double().numpy(),
                                   T_STEP, R.BASE_LR, beta1, beta2, R.EPS, 1e-3)
        assert np.abs(hp[i][1].cpu().double().numpy() - wp).max() <= bound10["param"]
        assert np.abs(hm[i][1].cpu().double().numpy() - wm).max() <= bound10["exp_avg"]
        assert (np.abs(hv[i][1].cpu().double().numpy() - wv) / wv).max() <= bound10["exp_avg_sq"]
        for held in (hp, hg, hm, hv):
            assert _sentinels_intact(held[i][0], sizes[i])
    # refused before anything is launched: the buffers keep their bits
    before = hp[1][0].clone()
    args = (beta1, beta2, R.EPS, 1.0, None, 0.0, None)
    assert lib.care_adam_step(None, 0, *args) == 0
    assert lib.care_adam_step(None, 3, *args) == -1 and lib.care_adam_step(d, -1, *args) == -1
    keep = d[1].n
    d[1].n = -1
    assert lib.care_adam_step(d, 3, *args) == -1
    d[1].n = keep
    keep = d[2].v
    d[2].v = None
    assert lib.care_adam_step(d, 3, *args) == -1
    d[2].v = keep + 2
    assert lib.care_adam_step(d, 3, *args) == -2
    partials = torch.zeros(2048, dtype=torch.float64, device=DEV)
    norm = torch.zeros(2, device=DEV)
    assert lib.care_grad_sqnorm(d, 3, partials.data_ptr(), norm.data_ptr(), None) == -2
    d[2].v = keep
    assert lib.care_grad_sqnorm(d, 3, None, norm.data_ptr(), None) == -1 and lib.care_grad_sqnorm(d, 3, partials.data_ptr(), None, None) == -1
    assert lib.care_grad_sqnorm(d, 3, partials.data_ptr() + 4, norm.data_ptr(), None) == -2
    assert lib.care_adam_step(d, 3, beta1, beta2, R.EPS, 1.0, norm.data_ptr() + 2, 5.0, None) == -2
    torch.cuda.synchronize()
    assert torch.equal(before, hp[1][0])


# ------------------------------------------------------------------ care_amd.optim.Adam
def _device_params(seed=0):
    """The recipe's tensors as device Parameters; the last one a view at storage offset 1 of a larger buffer."""
    cpu = R.recipe_params(seed)
    out = []
    for i, p in enumerate(cpu):
        if i == len(cpu) - 1:
            buf = torch.zeros(p.numel() + 8, device=DEV)
            buf[1:1 + p.numel()] = p.to(DEV)
            q = torch.nn.Parameter(buf[1:1 + p.numel()])
            assert q.storage_offset() == 1 and q.data_ptr() % 16 != 0 and q.is_contiguous()
        else:
            q = torch.nn.Parameter(p.to(DEV))
        out.append(q)
    return out


def _set_grads(params, grads):
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
        elif i == len(params) - 1:      # the gradient of the offset view: at an odd offset as well
            buf = torch.zeros(g.numel() + 8, device=DEV)
            buf[3:3 + g.numel()] = g.to(DEV)
            p.grad = buf[3:3 + g.numel()]
        else:
            p.grad = g.to(DEV)


def _ours(params, **kw):
    from care_amd.optim import Adam

    return Adam(R.torch_groups(params), lr=R.BASE_LR, betas=R.BETAS, eps=R.EPS, **kw)


def _check(ref, params, optim, bound, what=""):
    st = [optim.state[p] for p in params]
    dp, dm, dv = R.deviations(ref, [p.detach().cpu().numpy() for p in params], [s["exp_avg"].cpu().numpy() for s in st],
                              [s["exp_avg_sq"].cpu().numpy() for s in st])
    print(what, "deviation from float64: param", dp, "exp_avg", dm, "exp_avg_sq (relative)", dv, "| bounds", bound["param"],
          bound["exp_avg"], bound["exp_avg_sq"], "| torch's own", bound["torch"])
    assert dp <= bound["param"] and dm <= bound["exp_avg"] and dv <= bound["exp_avg_sq"], (dp, dm, dv, bound)


def test_trajectory_of_ten_clipped_steps(bound10):
    ref, ref_norms = R.run_reference(10)
    params = _device_params()
    optim = _ours(params, max_grad_norm=R.MAX_NORM)
    for s in range(10):
        grads = R.recipe_grads(s)
        _set_grads(params, grads)
        optim.step()
        got = float(optim.last_grad_norm)
        assert abs(got - ref_norms[s]) <= bound10["norm"] * ref_norms[s], (s, got, ref_norms[s])
        for p, g in zip(params, grads):      # .grad stays unscaled after a clipped step
            assert torch.equal(p.grad.cpu(), g)
    _check(ref, params, optim, bound10, "10 steps")
    assert all(optim.state[p]["step"] == 10 for p in params)


def test_idle_clipping_is_bit_identical_to_no_clipping():
    runs = []
    for max_norm in (R.MAX_NORM, 0.0):
        params = _device_params()
        optim = _ours(params, max_grad_norm=max_norm)
        for s in range(4):
            _set_grads(params, R.recipe_grads(s, scales=(1e-3, 1e-3)))
            optim.step()
        if max_norm:
            assert 0 < float(optim.last_grad_norm) < max_norm
        else:
            assert optim.last_grad_norm is None
        runs.append([torch.cat([p.detach().cpu().view(torch.int32), optim.state[p]["exp_avg"].cpu().view(torch.int32),
                                optim.state[p]["exp_avg_sq"].cpu().view(torch.int32)]) for p in params])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_schedulers_and_skipped_parameters(bound10):
    from torch.optim.lr_scheduler import StepLR

    cpu = R.recipe_params()
    n = len(cpu)
    _, _, lrs, wds = R.recipe_groups(n)
    ref = R.RefAdam([p.numpy() for p in cpu], lrs, wds, max_grad_norm=R.MAX_NORM)
    params = _device_params()
    optim = _ours(params, max_grad_norm=R.MAX_NORM)
    sched = StepLR(optim, step_size=1, gamma=0.5)
    untouched = None
    for s in range(5):
        grads = R.recipe_grads(s)
        if s in (1, 3):
            grads[2], grads[5] = None, None          # skipped in these steps: no update, no step count
            untouched = [params[i].detach().clone() for i in (2, 5)]
        _set_grads(params, grads)
        optim.step()
        ref.step([None if g is None else g.numpy() for g in grads])
        if s in (1, 3):
            assert all(torch.equal(a, params[i].detach()) for a, i in zip(untouched, (2, 5)))
        sched.step()
        ref.lrs = [lr * 0.5 for lr in ref.lrs]
        assert [g["lr"] for g in optim.param_groups] == pytest.approx([ref.lrs[0], ref.lrs[1]], rel=1e-12)
    assert [optim.state[p]["step"] for p in params] == ref.t and ref.t[2] == ref.t[5] == 3 and ref.t[0] == 5
    _check(ref, params, optim, bound10, "StepLR + skipped")
    # a parameter that never had a gradient has no state at all
    extra = torch.nn.Parameter(torch.ones(7, device=DEV))
    optim.add_param_group({"params": [extra]})
    _set_grads(params, R.recipe_grads(9))
    optim.step()
    assert extra not in optim.state and bool((extra == 1).all())


def test_state_moves_from_torch_adam_on_the_device():
    bound = R.torch_fp32_bound(6)
    ref, _ = R.run_reference(6)
    params = _device_params()
    theirs = torch.optim.Adam(R.torch_groups(params), lr=R.BASE_LR, betas=R.BETAS, eps=R.EPS)
    for s in range(3):
        _set_grads(params, R.recipe_grads(s))
        torch.nn.utils.clip_grad_norm_(params, R.MAX_NORM)
        theirs.step()
    optim = _ours(params, max_grad_norm=R.MAX_NORM)
    optim.load_state_dict(theirs.state_dict())
    assert all(optim.state[p]["step"] == 3 for p in params)
    for s in range(3, 6):
        _set_grads(params, R.recipe_grads(s))
        optim.step()
    _check(ref, params, optim, bound, "3 torch + 3 HIP steps")
    # ... and back: torch's optimiser takes our state dict and steps from it
    theirs.load_state_dict(optim.state_dict())
    _set_grads(params, R.recipe_grads(6))
    theirs.step()
    assert all(float(theirs.state[p]["step"]) == 7 for p in params)


def test_a_non_finite_gradient_behaves_as_in_torch():
    params = _device_params()
    optim = _ours(params, max_grad_norm=R.MAX_NORM)
    grads = R.recipe_grads(1)
    grads[4][17] = float("inf")
    _set_grads(params, grads)
    optim.step()            # no exception, no skipped step
    assert not math.isfinite(float(optim.last_grad_norm))
    assert all(optim.state[p]["step"] == 1 for p in params)
    assert not bool(torch.isfinite(params[4]).all()), "clip_grad_norm_ + Adam leave non-finite parameters behind; so must this"


@pytest.mark.parametrize("max_norm", [0.0, R.MAX_NORM])
def test_a_step_never_waits_for_the_device(max_norm):
    params = _device_params()
    optim = _ours(params, max_grad_norm=max_norm)
    all_grads = []
    for s in range(10):
        _set_grads(params, R.recipe_grads(s))
        all_grads.append([p.grad for p in params])
    noncontig = torch.randn(1025, 2, device=DEV)[:, 0]     # one gradient that needs the contiguous copy
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(10):
            for p, g in zip(params, all_grads[s]):
                p.grad = g
            if s == 4:
                params[7].grad = noncontig
            optim.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(optim.state[p]["step"] == 10 for p in params) and all(bool(torch.isfinite(p).all()) for p in params)


# ------------------------------------------------------------------ the model
def _build(golden, **over):
    from care_amd import get_framework

    opt, P, feats, ids = golden.build()
    opt.update(over)
    model = get_framework(opt)
    model.load_state_dict(P, strict=True)
    return opt, P, feats, ids, model.to(DEV)


NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def test_a_few_steps_of_configure_optimizers_reduce_the_loss():
    """test_gpu_training.py::test_a_few_optimizer_steps_reduce_the_loss's loop with this package's optimiser."""
    from conftest import GoldenCase
    from care_amd import configure_optimizers
    from care_amd.optim import Adam

    opt, P, feats, ids, model = _build(GoldenCase("msrvtt_base_ami_b2"), learning_rate=1e-3, gradient_clip_val=5.0, **NO_DROP)
    model.train()
    batch = {"feats": [f.to(DEV) for f in feats], "input_ids": ids.to(DEV)}
    labels = torch.roll(ids, -1, dims=1).to(DEV)
    optim = configure_optimizers(opt, model)["optimizer"]
    assert type(optim) is Adam and optim.max_grad_norm == 5.0 and optim.param_groups[0]["lr"] == 1e-3
    losses = []
    for _ in range(6):
        optim.zero_grad()
        lg = model(batch)["logits"]
        loss = torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1))
        loss.backward()
        optim.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] - 0.5, losses
    model.eval()
    assert torch.isfinite(model.feedforward_step(batch, output_auxiliary=False)["logits"]).all()


def test_validation_after_training_sees_the_weights_the_kernels_wrote():
    """Captions from the graph-replayed eval pass, four optimiser steps, captions again: they must be those of a FRESH module
    loaded with the updated state dict.  The engine decides from the parameters' version counters whether to re-pack its
    weights and drop its graphs; the kernels write through raw pointers, so the optimiser has to move the counters itself."""
    from conftest import GoldenCase
    from care_amd import get_framework, get_translator
    from care_amd.optim import Adam

    opt, P, feats, ids, model = _build(GoldenCase("msrvtt_care_eos_b4"), **NO_DROP)
    tr = get_translator(dict(opt, beam_size=5, topk=2))
    batch = {"feats": [f.to(DEV) for f in feats], "input_ids": ids.to(DEV)}
    labels = torch.roll(ids, -1, dims=1).to(DEV)
    optim = Adam(model.parameters(), lr=5e-3, max_grad_norm=5.0)

    def captions():
        model.eval()
        for _ in range(3):   # eager, captured, replayed
            now = tr.translate_batch([model], batch)
        return now

    first = captions()
    versions = [p._version for p in model.parameters()]
    model.train()
    for _ in range(4):
        optim.zero_grad()
        lg = model(batch)["logits"]
        torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1)).backward()
        optim.step()
    stepped = [p for p in model.parameters() if p in optim.state]
    assert stepped and all(p._version > v for p, v in zip(model.parameters(), versions) if p in optim.state)
    second = captions()
    fresh = get_framework(opt).eval()
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
    fresh.to(DEV)
    assert second == get_translator(dict(opt, beam_size=5, topk=2)).translate_batch([fresh], batch)
    assert first != second, "four Adam steps at lr 5e-3 did not change one caption: the test does not test"

"""CPU: care_amd.optim without a GPU - the float64 yardstick of the optimiser tests against torch's own Adam and
clip_grad_norm_, the parameter groups and schedulers against the genuine reference's (tests/golden/optim/groups.json,
recorded by tools/gen_optim_golden.py; models/Wrapper.py:316-386), the state exchange with torch.optim.Adam, the refusals,
and the agreement of include/care_hip.h, care_amd/_lib.py and the libraries on the new entry points."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import optim_reference as R
from c_layout import c_layout
from care_amd import optim as care_optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = json.load(open(os.path.join(ROOT, "tests", "golden", "optim", "groups.json")))


def test_float64_yardstick_is_torch_adam_with_clip_grad_norm():
    """10 steps of the recipe: the restated formulas against torch.optim.Adam + clip_grad_norm_ on float64 tensors, 1e-12
    relative - parameters, both moments and the norm of every step."""
    ref, ref_norms = R.run_reference(10)
    params, optim, norms = R.run_torch(10, torch.float64)
    assert len(norms) == 10 and max(norms) > R.MAX_NORM > min(norms), "the recipe must clip in some steps and idle in others"
    for a, b in zip(norms, ref_norms):
        assert abs(a - b) <= 1e-12 * b
    for i, p in enumerate(params):
        st = optim.state[p]
        assert int(st["step"]) == ref.t[i] == 10
        for got, want in ((p.detach().numpy(), ref.p[i]), (st["exp_avg"].numpy(), ref.m[i]), (st["exp_avg_sq"].numpy(), ref.v[i])):
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), i
    # ... and without clipping (the coefficient is exactly 1, not applied)
    ref0, _ = R.run_reference(3, max_grad_norm=0.0)
    params0, _, _ = R.run_torch(3, torch.float64, max_grad_norm=0.0)
    for p, want in zip(params0, ref0.p):
        assert np.abs(p.detach().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert R.clip_coef(1.0, 5.0) == 1.0 and R.clip_coef(10.0, 5.0) == 5.0 / (10.0 + 1e-6)
    assert R.clip_coef(float("inf"), 5.0) == 0.0 and np.isnan(R.clip_coef(float("nan"), 5.0))


def _model(config):
    from care_amd import get_framework
    from care_amd.configs import make_opt

    return get_framework(make_opt(config))


@pytest.fixture(scope="module")
def models():
    return {c: _model(c) for c in GROUPS["models"]}


def test_filter_weight_decay_groups_are_the_references(models):
    assert len(GROUPS["cases"]) == 8
    for case in GROUPS["cases"]:
        model = models[case["config"]]
        names = {id(p): n for n, p in model.named_parameters()}
        info = GROUPS["models"][case["config"]]
        assert len(names) == info["tensors"] and sum(p.numel() for p in model.parameters()) == info["elements"]
        groups = care_optim.filter_weight_decay(model, GROUPS["weight_decay"], case["filter_biases"], (), case["skip_substr_list"])
        assert len(groups) == len(case["groups"]) == 2
        for got, want in zip(groups, case["groups"]):
            assert sorted(got) == ["params", "weight_decay"] and got["weight_decay"] == want["weight_decay"]
            assert [names[id(p)] for p in got["params"]] == want["params"], case
    # skip_list: by full name
    model = models["msrvtt_care"]
    first = next(n for n, _ in model.named_parameters())
    groups = care_optim.filter_weight_decay(model, 1e-2, False, (first,), ())
    assert [id(p) for p in groups[0]["params"]] == [id(dict(model.named_parameters())[first])]


@pytest.mark.parametrize("kind", ["linear", "cosine", "linear_with_warmup", "plateau"])
def test_configure_optimizers_matches_the_wrapper(models, kind):
    """Wrapper.py:316-386: the optimiser's groups, each scheduler's class and constructor values, the returned dict's keys."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, ReduceLROnPlateau, StepLR

    from care_amd.configs import make_opt

    model = models["msrvtt_care"]
    names = {id(p): n for n, p in model.named_parameters()}
    opt = make_opt("msrvtt_care")
    opt.update(lr_scheduler_type=kind, learning_rate=3e-4, weight_decay=2e-4, gradient_clip_val=5.0)
    if kind == "linear_with_warmup":
        opt.update(max_steps=1000, learning_rate_warmup_ratio=0.1, learning_rate_warmup_steps=7)
    out = care_optim.configure_optimizers(opt, model, max_steps=400)
    optim, sch = out["optimizer"], out["lr_scheduler"]["scheduler"]
    assert isinstance(optim, care_optim.Adam) and isinstance(optim, torch.optim.Optimizer) and optim.max_grad_norm == 5.0
    assert sorted(out) == ["lr_scheduler", "optimizer"]
    # without filter_weight_decay: ONE group of every trainable parameter with the decay (Wrapper.py:331-332)
    assert len(optim.param_groups) == 1 and optim.param_groups[0]["weight_decay"] == 2e-4 and optim.param_groups[0]["lr"] in (3e-4, 0.0)
    assert [names[id(p)] for p in optim.param_groups[0]["params"]] == GROUPS["models"]["msrvtt_care"]["trainable"]
    common = {"scheduler", "interval", "frequency"}
    if kind == "linear":
        assert type(sch) is StepLR and sch.step_size == 1 and sch.gamma == 0.9
        assert set(out["lr_scheduler"]) == common and out["lr_scheduler"]["interval"] == "epoch"
    elif kind == "cosine":
        assert type(sch) is CosineAnnealingLR and sch.T_max == 400 and sch.eta_min == 1e-6
        assert set(out["lr_scheduler"]) == common and out["lr_scheduler"]["interval"] == "step"
        with pytest.raises(ValueError, match="max_steps"):
            care_optim.configure_optimizers(opt, model)
    elif kind == "linear_with_warmup":
        assert type(sch) is LambdaLR and set(out["lr_scheduler"]) == common and out["lr_scheduler"]["interval"] == "step"
        f = sch.lr_lambdas[0]   # misc/optim.py:27-32 with 100 warm-up steps of 1000
        assert [f(0), f(50), f(100), f(550), f(1000), f(1200)] == [0.0, 0.5, 1.0, 0.5, 0.0, 0.0]
        opt.update(learning_rate_warmup_ratio=0)
        f = care_optim.configure_optimizers(opt, model)["lr_scheduler"]["scheduler"].lr_lambdas[0]
        assert f(7) == 1.0 and f(3) == 3 / 7
    else:
        assert type(sch) is ReduceLROnPlateau and sch.mode == "max" and sch.factor == 0.9 and sch.patience == 1 and sch.min_lrs == [1e-6]
        assert set(out["lr_scheduler"]) == common | {"monitor", "strict"}
        assert out["lr_scheduler"]["monitor"] == "CIDEr" and out["lr_scheduler"]["strict"] is True and out["lr_scheduler"]["interval"] == "epoch"
    assert out["lr_scheduler"]["frequency"] == 1
    # the reference's defaults, and the grouped form (Wrapper.py:321-329: the groups carry the decay, the optimiser none)
    bare = care_optim.configure_optimizers({"lr_scheduler_type": "linear"}, model)["optimizer"]
    assert bare.param_groups[0]["lr"] == 5e-4 and bare.param_groups[0]["weight_decay"] == 5e-4 and bare.max_grad_norm == 0.0
    opt.update(filter_weight_decay=True, filter_biases=True, skip_substr_list=["LayerNorm", "embedding"], lr_scheduler_type="linear")
    grouped = care_optim.configure_optimizers(opt, model)["optimizer"]
    want = next(c for c in GROUPS["cases"] if c["config"] == "msrvtt_care" and c["filter_biases"] and c["skip_substr_list"])
    assert [g["weight_decay"] for g in grouped.param_groups] == [0.0, 2e-4]
    assert [[names[id(p)] for p in g["params"]] for g in grouped.param_groups] == [g["params"] for g in want["groups"]]


def _state_equal(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"])
    for k in a["state"]:
        assert sorted(a["state"][k]) == sorted(b["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(a["state"][k]["step"]) == float(b["state"][k]["step"])
        assert torch.is_tensor(a["state"][k]["step"]) and torch.is_tensor(b["state"][k]["step"])
        assert a["state"][k]["step"].dtype == b["state"][k]["step"].dtype
        for kk in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][k][kk], b["state"][k][kk])


def test_state_dict_moves_between_torch_adam_and_ours():
    g = torch.Generator().manual_seed(3)
    mk = lambda: [torch.nn.Parameter(torch.rand(n, generator=torch.Generator().manual_seed(n))) for n in (5, 12, 7)]
    ps = mk()
    groups = lambda ps: [{"params": ps[:2], "weight_decay": 1e-3}, {"params": ps[2:], "lr": 2e-4, "betas": (0.8, 0.99), "eps": 1e-6}]
    theirs = torch.optim.Adam(groups(ps), lr=5e-4)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        theirs.step()
    sd = copy.deepcopy(theirs.state_dict())   # (load_state_dict adopts tensors that need no cast: no sharing between the runs)
    ours = care_optim.Adam(groups(mk()), lr=1.0, weight_decay=0.5)
    ours.load_state_dict(sd)
    assert all(isinstance(st["step"], int) and st["step"] == 2 for st in ours.state.values())   # a host integer from here on
    assert ours.param_groups[1]["lr"] == 2e-4 and ours.param_groups[1]["betas"] == (0.8, 0.99) and ours.param_groups[1]["eps"] == 1e-6
    assert ours.param_groups[0]["lr"] == 5e-4 and ours.param_groups[0]["weight_decay"] == 1e-3
    back = ours.state_dict()
    _state_equal(back, sd)
    # ... and the reverse: our state dict steps in torch's optimiser (every key its step reads is there)
    ps2 = mk()
    again = torch.optim.Adam(groups(ps2), lr=9.0)
    again.load_state_dict(copy.deepcopy(back))
    for p, q in zip(ps2, ps):
        p.data.copy_(q.data)
    g2 = torch.Generator().manual_seed(4)
    grads = [torch.randn(p.shape, generator=g2) for p in ps]
    for opt_, plist in ((theirs, ps), (again, ps2)):
        for p, gr in zip(plist, grads):
            p.grad = gr.clone()
        opt_.step()
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
    _state_equal(again.state_dict(), theirs.state_dict())
    # a fresh optimiser of ours has torch's group keys, and a pickle round trip keeps the clipping norm
    fresh = care_optim.Adam(mk(), max_grad_norm=2.5)
    assert set(torch.optim.Adam(mk()).param_groups[0]) == set(fresh.param_groups[0])
    import pickle
    assert pickle.loads(pickle.dumps(fresh)).max_grad_norm == 2.5


def test_refusals_by_name():
    p = [torch.nn.Parameter(torch.zeros(4))]
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            care_optim.Adam(p, **{flag: True})
        opt = care_optim.Adam(p)
        opt.param_groups[0][flag] = True        # as a loaded torch state dict would set it
        p[0].grad = torch.zeros(4)
        with pytest.raises(NotImplementedError, match=flag):
            opt.step()
    with pytest.raises(ValueError):
        care_optim.Adam(p, lr=-1.0)
    with pytest.raises(ValueError):
        care_optim.Adam(p, betas=(1.0, 0.9))
    with pytest.raises(ValueError):
        care_optim.Adam(p, max_grad_norm=-1.0)
    opt = care_optim.Adam(p)
    p[0].grad = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state) == 0, "a refused step leaves no state behind"
    p[0].grad = None
    assert opt.step() is None and opt.step(lambda: 3.0) == 3.0      # nothing to step: nothing is launched
    # sparse gradients, other dtypes, non-contiguous parameters: refused by name, whatever the device
    emb = torch.nn.Embedding(6, 3, sparse=True)
    emb(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(NotImplementedError, match="sparse gradients"):
        care_optim.Adam(emb.parameters()).step()
    for dtype in (torch.float64, torch.bfloat16):
        q = torch.nn.Parameter(torch.zeros(4, dtype=dtype))
        q.grad = torch.zeros(4, dtype=dtype)
        with pytest.raises(NotImplementedError, match="must be fp32"):
            care_optim.Adam([q]).step()
    q = torch.nn.Parameter(torch.zeros(4, 6).t())
    q.grad = torch.zeros(6, 4)
    with pytest.raises(NotImplementedError, match="not contiguous"):
        care_optim.Adam([q]).step()
    with pytest.raises(NotImplementedError, match="tensor `lr`"):
        care_optim.Adam(p, lr=torch.tensor(1e-3))


def test_header_binding_and_libraries_agree_on_the_optimiser_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 25
    assert "optim.hip" in build.SOURCES
    build.build_all()
    for name in ("care_grad_sqnorm", "care_adam_step"):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "void* stream"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params)
        for ctype, decl in zip(sig, params):
            want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else \
                ctypes.c_double if decl.startswith("double") else ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            assert hasattr(ctypes.CDLL(build.lib_path(variant)), name)
    assert "care_grad_sqnorm_partials" in _lib.PLAIN
    block = header[header.index("The optimiser step"):header.index("int care_grad_sqnorm_partials")]
    for cite in ("models/Wrapper.py:316-386", "train.py:128", "misc/utils.py:282-304"):
        assert cite in block
    # the descriptor: ctypes mirror against the C compiler's layout of the header
    sizes = c_layout(["sizeof(care_opt_tensor)", "offsetof(care_opt_tensor, n)", "offsetof(care_opt_tensor, step_size)",
                      "offsetof(care_opt_tensor, weight_decay)", "CARE_OPT_PACK"])
    T = _lib.OptTensor
    assert sizes == [ctypes.sizeof(T), T.n.offset, T.step_size.offset, T.weight_decay.offset, 64]
    # the host-side checks need no device: they return before anything is launched
    lib = _lib.load()
    assert lib.care_grad_sqnorm_partials(0) == 1 and lib.care_grad_sqnorm_partials(1024) == 1 and lib.care_grad_sqnorm_partials(1025) == 2
    assert lib.care_grad_sqnorm_partials(18218884) == 2048
    assert lib.care_adam_step(None, 0, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == 0          # count == 0: a no-op
    d = (T * 2)()
    for x in d:
        x.p, x.g, x.m, x.v, x.n = 64, 128, 192, 256, 8
    assert lib.care_adam_step(None, 2, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == -1         # CARE_EINVAL
    assert lib.care_adam_step(d, -1, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == -1
    d[1].n = -1
    assert lib.care_adam_step(d, 2, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == -1
    d[1].n, d[1].m = 8, None
    assert lib.care_adam_step(d, 2, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == -1
    d[1].m = 194
    assert lib.care_adam_step(d, 2, 0.9, 0.999, 1e-8, 1.0, None, 0.0, None) == -2         # CARE_EALIGN
    assert lib.care_grad_sqnorm(d, 2, 512, 1024, None) == -2
    d[1].m = 196
    assert lib.care_grad_sqnorm(d, 2, None, 1024, None) == -1 and lib.care_grad_sqnorm(d, 2, 516, 1024, None) == -2
    assert lib.care_adam_step(d, 2, 0.9, 0.999, 1e-8, 1.0, 1026, 5.0, None) == -2

"""CPU: the mean-teacher step (care_amd/interplay.py, csrc/interplay.hip) without a GPU - the agreement of include/care_hip.h,
care_amd/_lib.py and both libraries on care_ema_step / care_mse_fwd / care_mse_bwd, the refusals (all of them come before any
launch), and `InterplayStep`'s bookkeeping on CPU modules (models/Wrapper.py:550-614, opts.py:253-255)."""
import ctypes
import os
import re

import pytest
import torch

import interplay_reference as R
from c_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("care_ema_step", "care_mse_fwd", "care_mse_bwd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3


def test_header_binding_and_libraries_agree_on_the_mean_teacher_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "interplay.hip" in build.SOURCES
    build.build_all()
    for name in ENTRY_POINTS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "void* stream"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), name
        for ctype, decl in zip(sig, params):
            want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else \
                ctypes.c_double if decl.startswith("double") else ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            assert hasattr(ctypes.CDLL(build.lib_path(variant)), name), (variant, name)
    assert "care_mse_partials" in _lib.PLAIN and _lib.PLAIN["care_mse_partials"] == (ctypes.c_int, [ctypes.c_int64])
    assert set(ENTRY_POINTS) | {"care_mse_partials"} <= set(_lib.exported_symbols())
    block = header[header.index("The mean-teacher step"):header.index("int care_ema_step")]
    for cite in ("models/Wrapper.py:550-614", "opts.py:253-255"):
        assert cite in block
    # the library is this tree's: its version is the header's, whatever the number
    for variant in build.VARIANTS:
        assert _lib.load(variant=variant).care_version() == int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1))
        assert _lib.source_hash(variant) == build.source_hash(variant)


def test_the_descriptor_mirrors_the_c_layout():
    from care_amd import _lib

    sizes = c_layout(["sizeof(care_ema_tensor)", "offsetof(care_ema_tensor, t)", "offsetof(care_ema_tensor, s)",
                      "offsetof(care_ema_tensor, n)", "CARE_EMA_PACK"])
    T = _lib.EmaTensor
    assert sizes[:4] == [ctypes.sizeof(T), T.t.offset, T.s.offset, T.n.offset]
    # the pack (descriptors, a first chunk each and one more, the count) and the kernel's three scalars fit the 4-KB argument block
    pack = sizes[4]
    assert pack >= 64 and pack * sizes[0] + (pack + 2) * 4 + 3 * 4 <= 4096


def test_the_host_checks_refuse_before_any_launch():
    """No device here: every call below must return before it launches anything."""
    from care_amd import _lib

    lib = _lib.load()
    assert lib.care_mse_partials(0) == 1 and lib.care_mse_partials(1) == 1 and lib.care_mse_partials(1024) == 1
    assert lib.care_mse_partials(1025) == 2 and lib.care_mse_partials(2 * 7 * 10547) == 145 and lib.care_mse_partials(1 << 40) == 2048
    T = _lib.EmaTensor
    assert lib.care_ema_step(None, 0, 0.999, 1 - 0.999, None) == 0          # count == 0: a no-op
    d = (T * 2)()
    for x in d:
        x.t, x.s, x.n = 64, 128, 8
    assert lib.care_ema_step(None, 2, 0.5, 0.5, None) == EINVAL
    assert lib.care_ema_step(d, -1, 0.5, 0.5, None) == EINVAL
    d[1].n = -1
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EINVAL
    d[1].n, d[1].t = 8, None
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EINVAL
    d[1].t, d[1].s = 64, None
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EINVAL
    d[1].s = 64                                                             # t == s
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EINVAL
    d[1].s = 130
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EALIGN
    d[1].s, d[1].t = 128, 66
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == EALIGN
    d[1].t, d[1].n = 64, 1 << 42                                            # more chunks than a launch can number
    assert lib.care_ema_step(d, 2, 0.5, 0.5, None) == ESHAPE
    # the distillation term
    assert lib.care_mse_fwd(None, 128, 8, 256, 512, None) == EINVAL and lib.care_mse_fwd(64, None, 8, 256, 512, None) == EINVAL
    assert lib.care_mse_fwd(64, 128, 8, None, 512, None) == EINVAL and lib.care_mse_fwd(64, 128, 8, 256, None, None) == EINVAL
    assert lib.care_mse_fwd(64, 128, 0, 256, 512, None) == EINVAL and lib.care_mse_fwd(64, 128, -3, 256, 512, None) == EINVAL
    assert lib.care_mse_fwd(66, 128, 8, 256, 512, None) == EALIGN and lib.care_mse_fwd(64, 129, 8, 256, 512, None) == EALIGN
    assert lib.care_mse_fwd(64, 128, 8, 260, 512, None) == EALIGN and lib.care_mse_fwd(64, 128, 8, 256, 514, None) == EALIGN
    assert lib.care_mse_bwd(None, 128, 8, 256, 512, None) == EINVAL and lib.care_mse_bwd(64, None, 8, 256, 512, None) == EINVAL
    assert lib.care_mse_bwd(64, 128, 8, None, 512, None) == EINVAL and lib.care_mse_bwd(64, 128, 8, 256, None, None) == EINVAL
    assert lib.care_mse_bwd(64, 128, 0, 256, 512, None) == EINVAL
    assert lib.care_mse_bwd(66, 128, 8, 256, 512, None) == EALIGN and lib.care_mse_bwd(64, 128, 8, 258, 512, None) == EALIGN
    assert lib.care_mse_bwd(64, 128, 8, 256, 513, None) == EALIGN


def test_the_yardstick_restates_the_wrapper():
    """interplay_reference.py against the expressions of Wrapper.py:565 and 574-581 written out with plain tensor operations."""
    g = torch.Generator().manual_seed(11)
    t = [torch.randn(n, generator=g) for n in (1, 5, 1025)]
    s = [torch.randn(n, generator=g) for n in (1, 5, 1025)]
    for w in (0.999, 0.5, 0.0, 1.0):
        got = R.ema_reference(t, s, w)
        for a, x, y in zip(got, t, s):
            assert torch.equal(R.bits(a), R.bits(x * w + y * (1 - w)))      # three roundings, elementwise: the same bits
    assert all(torch.equal(a, b) for a, b in zip(R.ema_reference(t, s, 1.0), t))
    a, b = torch.randn(4, 7, 33, generator=g), torch.randn(4, 7, 33, generator=g)
    a64 = a.double().requires_grad_(True)
    loss = ((a64 - b.double()) ** 2).mean()
    (loss * 0.25).backward()
    loss = loss.detach()
    assert abs(R.mse_reference64(a, b) - float(loss)) <= 1e-15 * float(loss)
    assert torch.allclose(R.mse_grad_reference64(a, b, 0.25), a64.grad, rtol=1e-14, atol=0)
    assert abs(float(((a - b) ** 2).mean()) - R.mse_reference64(a, b)) <= 16 * R.BAR * R.mse_reference64(a, b)


def test_refusals():
    from care_amd import distillation_mse, ema_update
    from care_amd.criterion import DeferredLogits

    a, b = torch.zeros(2, 3, 5), torch.zeros(2, 3, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distillation_mse(a, b)
    with pytest.raises(ValueError, match="shape"):
        distillation_mse(a, torch.zeros(2, 3, 6))
    deferred = DeferredLogits(torch.zeros(2, 3, 4), torch.zeros(5, 4))
    with pytest.raises(NotImplementedError, match="fused head"):
        distillation_mse(deferred, b)
    with pytest.raises(NotImplementedError, match="set_fused_head"):
        distillation_mse(a, deferred)
    t, s = [torch.zeros(4), torch.zeros(7)], [torch.ones(4), torch.ones(7)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ema_update(t, s, 0.999)
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_weight"):
            ema_update(t, s, w)
    with pytest.raises(ValueError, match="2 teacher tensors against 1"):
        ema_update(t, s[:1], 0.5)
    with pytest.raises(ValueError, match="differ in size"):
        ema_update(t, [torch.ones(4), torch.ones(8)], 0.5)
    with pytest.raises(ValueError, match="paired with itself"):
        ema_update(t, [s[0], t[1]], 0.5)
    with pytest.raises(ValueError, match="paired with itself"):
        ema_update(t, [s[0], t[1].view(7)], 0.5)                    # another tensor object over the same storage
    with pytest.raises(NotImplementedError, match="fp32"):
        ema_update([torch.zeros(4, dtype=torch.float64)], [torch.ones(4, dtype=torch.float64)], 0.5)
    with pytest.raises(NotImplementedError, match="not contiguous"):
        ema_update([torch.zeros(4, 6).t()], [torch.ones(6, 4)], 0.5)
    assert all(bool((x == 0).all()) for x in t), "a refused update writes nothing"
    assert ema_update([], [], 0.5) is None                          # nothing to average: nothing is launched


@pytest.fixture(scope="module")
def student():
    from care_amd import get_framework
    from care_amd.configs import make_opt

    opt = make_opt("msrvtt_base_ami")
    torch.manual_seed(1)
    return opt, get_framework(opt)


def test_interplay_step_defaults(student):
    from care_amd import InterplayStep
    from care_amd.criterion import Criterion
    from care_amd.optim import Adam

    opt, model = student
    assert not any(k in opt for k in ("distillation_weight", "ema_weight", "eval_model"))
    step = InterplayStep(opt, model)
    assert (step.distillation_weight, step.ema_weight, step.eval_model) == (0.01, 0.999, "teacher")        # opts.py:253-255
    over = InterplayStep(dict(opt, distillation_weight=0.5, ema_weight=0.9, eval_model="student"), model, teacher=step.teacher_captioner)
    assert (over.distillation_weight, over.ema_weight, over.eval_model) == (0.5, 0.9, "student")
    assert over.teacher_captioner is step.teacher_captioner
    assert isinstance(step.criterion, Criterion) and type(step.optimizer) is Adam and step.scheduler is not None
    assert [id(p) for g in step.optimizer.param_groups for p in g["params"]] == [id(p) for p in model.parameters() if p.requires_grad]
    # the default teacher: a distinct module of the same architecture with weights of its own
    teacher = step.teacher_captioner
    assert teacher is not model and type(teacher) is type(model) and step.captioner is model
    sd_s, sd_t = model.state_dict(), teacher.state_dict()
    assert list(sd_s) == list(sd_t) and all(sd_s[k].shape == sd_t[k].shape for k in sd_s)
    assert not set(p.data_ptr() for p in model.parameters()) & set(p.data_ptr() for p in teacher.parameters())
    assert not torch.equal(sd_s["cls_head.tgt_word_prj.weight"], sd_t["cls_head.tgt_word_prj.weight"])
    assert teacher.training == model.training
    assert step.last == {}
    # what is handed in is kept
    crit, sched = object(), torch.optim.lr_scheduler.StepLR(step.optimizer, 1)
    kept = InterplayStep(opt, model, criterion=crit, optimizer=step.optimizer, scheduler=sched, teacher=teacher)
    assert kept.criterion is crit and kept.optimizer is step.optimizer and kept.scheduler is sched
    lr = step.optimizer.param_groups[0]["lr"]
    step.training_epoch_end()
    assert step.optimizer.param_groups[0]["lr"] == pytest.approx(lr * opt.get("lr_decay", 0.9))


def test_swapping_and_evaluating(student):
    from care_amd import InterplayStep

    opt, model = student
    step = InterplayStep(opt, model)
    teacher = step.teacher_captioner
    step.swap_captioners()
    assert step.captioner is teacher and step.teacher_captioner is model
    step.swap_captioners()
    assert step.captioner is model and step.teacher_captioner is teacher
    with step.evaluating() as inside:
        assert inside is step and step.captioner is teacher and step.teacher_captioner is model
    assert step.captioner is model and step.teacher_captioner is teacher
    with pytest.raises(KeyError):
        with step.evaluating():
            assert step.captioner is teacher
            raise KeyError("the body fails")
    assert step.captioner is model and step.teacher_captioner is teacher, "the pair is back also when the body raises"
    own = InterplayStep(dict(opt, eval_model="student"), model, teacher=teacher)
    own.swap_captioners()
    assert own.captioner is model and own.teacher_captioner is teacher
    with own.evaluating():
        assert own.captioner is model

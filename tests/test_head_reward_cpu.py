"""No GPU: the interface of self-critical training on the fused head (care_amd/reward.py,
self_critical_head_loss; care_amd/scst.py, SelfCriticalStep(fused_head=True)): the agreement of include/care_hip.h,
care_amd/_lib.py and the two libraries on the new entry points with the ABI number unchanged, the export, the refusals by
name before anything runs, the argument checks of the entry points, and the step's keyword.  What runs on the GPU is
tests/test_gpu_head_reward.py's and tests/test_gpu_scst_fused.py's."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["care_head_reward_finish", "care_head_reward_reduce", "care_head_reward_gscale", "care_rows_scale"]
EINVAL, EALIGN, ESHAPE = -1, -2, -3
TWO = [[[10, 11, 12, 3], [10, 11, 13, 3]], [[20, 21, 3]]]


def test_header_binding_and_libraries_agree_on_the_new_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1)) == 25 and _lib.ABI_VERSION == 25   # additive
    assert "head_reward.hip" in build.SOURCES
    build.build_all()
    for name in NEW_SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name + " is not declared in include/care_hip.h"
        params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "void* stream", (name, params[-1])
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), (name, len(sig), len(params))
        for ctype, decl in zip(sig, params):   # pointers, 64-bit and 32-bit integers, floats: each in its place
            want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else \
                ctypes.c_double if decl.startswith("double") else ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            assert hasattr(ctypes.CDLL(build.lib_path(variant)), name), (variant, name)
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    for variant in build.VARIANTS:
        assert _lib.load(variant=variant).care_version() == 25
    block = header[header.index("The training head fused with the self-critical loss"):header.index("int care_head_reward_finish")]
    assert "models/Head.py:26-32" in block and "misc/Crit/crit_lang.py:57-60" in block


def test_entry_points_refuse_before_any_launch():
    """Pointers that are never dereferenced (no GPU here: a launch would fail): every refusal, and the calls that launch nothing."""
    from care_amd import _lib

    lib = _lib.load()
    P = 0x10000   # an aligned non-NULL address

    def finish(pmax=P, psum=P, plab=P, parts=3, idx_l=P, adv=P, t=29, V=130, R=0, rmax=P, lsum=P, logp=P, w=P):
        return lib.care_head_reward_finish(pmax, psum, plab, parts, idx_l, adv, t, V, R, rmax, lsum, logp, w, None)

    assert finish() == 0, "R == 0 is valid and launches nothing"
    for k in ("pmax", "psum", "plab", "idx_l", "adv", "rmax", "lsum", "logp", "w"):
        assert finish(**{k: None}) == EINVAL, k
    assert finish(R=-1) == EINVAL and finish(V=0) == EINVAL and finish(t=0) == EINVAL
    assert finish(parts=2) == ESHAPE and finish(parts=4) == ESHAPE

    def reduce(logp=P, w=P, idx_l=P, R=0, t=29, n_seq=4, totals=P, loss=P, seq_logp=P, acc=None):
        return lib.care_head_reward_reduce(logp, w, idx_l, R, t, n_seq, totals, loss, seq_logp, acc, None)

    for k in ("logp", "w", "idx_l", "totals", "loss"):
        assert reduce(**{k: None}) == EINVAL, k
    assert reduce(R=-1) == EINVAL and reduce(t=0) == EINVAL and reduce(n_seq=0) == EINVAL
    assert reduce(R=4 * 29 + 1) == ESHAPE
    assert reduce(totals=P + 4) == EALIGN and reduce(acc=P + 4) == EALIGN

    assert lib.care_head_reward_gscale(None, P, P, P, None) == EINVAL and lib.care_head_reward_gscale(P, None, P, P, None) == EINVAL
    assert lib.care_head_reward_gscale(P, P, None, P, None) == EINVAL and lib.care_head_reward_gscale(P, P, P, None, None) == EINVAL
    assert lib.care_head_reward_gscale(P, P + 4, P, P, None) == EALIGN

    def scale(src=P, ld_src=64, w=P, dst=P, ld_dst=64, rows=0, cols=64):
        return lib.care_rows_scale(src, ld_src, w, dst, ld_dst, rows, cols, None)

    assert scale() == 0 and scale(rows=5, cols=0) == 0, "no rows or no columns: valid, nothing is launched"
    for k in ("src", "w", "dst"):
        assert scale(**{k: None}) == EINVAL, k
    assert scale(rows=-1) == EINVAL and scale(cols=-1) == EINVAL
    assert scale(ld_src=63) == ESHAPE and scale(ld_dst=63) == ESHAPE


def test_the_function_is_exported():
    import care_amd
    from care_amd import reward

    assert care_amd.self_critical_head_loss is reward.self_critical_head_loss
    assert "self_critical_head_loss" in care_amd.__all__ and "self_critical_head_loss" in reward.__all__


def test_refusals_by_name_before_anything_runs():
    from care_amd import self_critical_head_loss

    h, W, labels, adv = torch.zeros(2, 3, 4), torch.zeros(7, 4), torch.ones(2, 3, dtype=torch.long), torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        self_critical_head_loss(h, W, labels, adv)
    with pytest.raises(TypeError, match="must be a tensor"):
        self_critical_head_loss(None, W, labels, adv)
    # shapes and dtypes are judged on meta tensors of a device that is never touched
    dev = torch.device("cuda")
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="meta")

    class OnDevice(torch.Tensor):
        """A meta tensor that reports a cuda device: the checks read shape, dtype and device only."""

        @property
        def device(self):
            return dev

    d = lambda t: t.as_subclass(OnDevice)
    good = dict(hidden=d(m(2, 3, 4)), weight=d(m(7, 4)), labels=d(m(2, 3, dtype=torch.long)), advantages=d(m(2)))

    def refused(exc, match, **change):
        with pytest.raises(exc, match=match):
            self_critical_head_loss(**{**good, **change})

    refused(TypeError, "`hidden` must be fp32", hidden=d(m(2, 3, 4, dtype=torch.float16)))
    refused(TypeError, "`weight` must be fp32", weight=d(m(7, 4, dtype=torch.float64)))
    refused(ValueError, "weight \\[V, d\\] expected", hidden=d(m(6, 4)))
    refused(ValueError, "weight \\[V, d\\] expected", weight=d(m(7, 5)))
    refused(ValueError, "labels \\[N, t\\] expected", labels=d(m(3, 3, dtype=torch.long)))
    refused(ValueError, "labels \\[N, t\\] expected", labels=d(m(2, 5, dtype=torch.long)))
    refused(ValueError, "labels \\[N, t\\] expected", labels=d(m(6, dtype=torch.long)))
    refused(ValueError, "`advantages` holds 3 entries", advantages=d(m(3)))
    refused(ValueError, "empty", hidden=d(m(2, 0, 4)), labels=d(m(2, 0, dtype=torch.long)))
    refused(ValueError, "`acc` must hold 2 float64", acc=d(m(2)))
    refused(ValueError, "`live` = 7 for 6 label positions", live=7)
    refused(ValueError, "`live` = -1", live=-1)


def test_the_step_takes_the_keyword_and_refuses_without_it():
    from care_amd import CiderBank, SelfCriticalStep

    host = CiderBank(TWO, 100, device=None, video_ids=["a", "b"])

    class Fused(object):      # the stub of tests/test_cider_cpu.py
        fused_head = True

    class Plain(object):
        fused_head = False

    sgd = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1)   # (a stub has no parameters to build one from)
    with pytest.raises(NotImplementedError, match="fused head"):
        SelfCriticalStep({}, Fused(), host)
    with pytest.raises(NotImplementedError, match="fused head"):
        SelfCriticalStep({}, Fused(), host, optimizer=sgd)
    with pytest.raises(NotImplementedError, match="fused head"):
        SelfCriticalStep({}, Fused(), host, optimizer=sgd, fused_head=False)
    step = SelfCriticalStep({}, Fused(), host, optimizer=sgd, fused_head=True)
    assert step.fused_head is True and step.optimizer is sgd
    assert SelfCriticalStep({}, Plain(), host, optimizer=sgd, fused_head=True).fused_head is True
    assert SelfCriticalStep({}, Plain(), host, optimizer=sgd).fused_head is False
    # the other refusals come first, with or without the keyword
    with pytest.raises(NotImplementedError, match="ensemble"):
        SelfCriticalStep({}, [Fused(), Fused()], host, fused_head=True)
    with pytest.raises(ValueError, match="baseline"):
        SelfCriticalStep({}, Fused(), host, baseline="median", fused_head=True)
    # the batch is judged before anything is sampled, and the stub is left as it was
    with pytest.raises(KeyError, match="video_ids"):
        step.training_step({"feats": []})
    assert Fused.fused_head is True


def test_the_pinned_refusals_stay():
    from care_amd import self_critical_loss
    from care_amd.criterion import DeferredLogits

    with pytest.raises(NotImplementedError, match="DeferredLogits"):
        self_critical_loss(DeferredLogits(torch.zeros(2, 3, 4), torch.zeros(7, 4)), torch.ones(2, 3, dtype=torch.long), torch.ones(2))

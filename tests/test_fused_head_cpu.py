"""No GPU: the interface of the training head fused with the language loss (care_amd/criterion.py, _HeadLoss):
the switch and its default, DeferredLogits, the refusals, the chunk planner and the agreement of include/care_hip.h,
care_amd/_lib.py and the two libraries on the new entry points.  What runs on the GPU is tests/test_gpu_fused_head.py's."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["care_head_live_rows", "care_gemm_tile_split3_head_stats", "care_head_loss_finish", "care_lang_loss_reduce",
               "care_head_grad_scale", "care_gemm_tile_split3_head_grad", "care_pieces_transpose"]


def _model():
    from care_amd import get_framework
    from care_amd.configs import make_opt

    return get_framework(make_opt("msrvtt_base_ami"))


def test_switch_is_off_by_default_and_follows_the_environment(monkeypatch):
    monkeypatch.delenv("CARE_TRAIN_FUSED_HEAD", raising=False)
    model = _model()
    assert model.fused_head is False
    assert model.set_fused_head(True) is model and model.fused_head is True
    assert model.set_fused_head(False).fused_head is False
    monkeypatch.setenv("CARE_TRAIN_FUSED_HEAD", "1")
    assert _model().fused_head is True
    monkeypatch.setenv("CARE_TRAIN_FUSED_HEAD", "0")
    assert _model().fused_head is False


def test_deferred_logits_stand_for_the_logits_and_have_no_cpu_fallback():
    from care_amd.criterion import DeferredLogits, get_criterion
    from care_amd.configs import make_opt

    hidden = torch.randn(3, 7, 64, requires_grad=True)
    W = torch.randn(130, 64, requires_grad=True)
    dl = DeferredLogits(hidden, W)
    assert dl.shape == torch.Size((3, 7, 130)) and tuple(dl.size()) == (3, 7, 130)
    assert [dl.size(i) for i in range(3)] == [3, 7, 130] and dl.size(-1) == 130
    assert dl.dim() == 3 and dl.device == hidden.device
    assert dl.hidden is hidden and dl.weight is W and callable(dl.materialize)
    with pytest.raises(ValueError):
        DeferredLogits(hidden, torch.randn(130, 32))
    crit = get_criterion(make_opt("msrvtt_base_ami"))
    labels = torch.randint(1, 130, (3, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit.get_loss({"logits": dl, "labels": labels})


def test_named_refusals_hold_for_deferred_logits():
    from care_amd.criterion import DeferredLogits, LanguageGeneration, get_criterion
    from care_amd.configs import make_opt

    dl = DeferredLogits(torch.randn(2, 5, 64), torch.randn(100, 64))
    labels = torch.randint(1, 100, (2, 5))
    lang = LanguageGeneration(make_opt("msrvtt_base_ami"))
    with pytest.raises(NotImplementedError, match="probs"):
        lang({"logits": dl, "labels": labels, "probs": torch.rand(2, 5, 100)})
    with pytest.raises(NotImplementedError, match="visual_word_generation"):
        get_criterion(make_opt("msrvtt_base_ami", visual_word_generation=True))
    for kind in ("prefix", "pp"):
        with pytest.raises(NotImplementedError, match="prefix / pp"):
            get_criterion(make_opt("msrvtt_care", use_attr=True, use_attr_type=kind))
    with pytest.raises(NotImplementedError, match="list"):
        lang({"logits": [dl, dl], "labels": labels})


def test_chunk_planner():
    from care_amd import criterion
    from care_amd.criterion import head_chunks

    C = criterion.HEAD_CHUNK_ROWS
    assert C >= 64
    assert head_chunks(0) == []
    assert head_chunks(1) == [(0, 1)]
    assert head_chunks(C) == [(0, C)]
    assert head_chunks(C + 1) == [(0, C), (C, C + 1)]
    assert head_chunks(257, 64) == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 257)]
    for n in (0, 1, 63, 64, 65, 257, 3 * C + 5):
        for c in (64, C):
            plan = head_chunks(n, c)
            assert [a for a, _ in plan] == list(range(0, n, c)) and all(0 < b - a <= c for a, b in plan)
            assert (plan[-1][1] if plan else 0) == n and all(plan[i][1] == plan[i + 1][0] for i in range(len(plan) - 1))
    with pytest.raises(ValueError):
        head_chunks(5, 0)


def test_header_binding_and_libraries_agree_on_the_new_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 24
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
                ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert ctype is want, (name, decl, ctype)
        for variant in build.VARIANTS:
            assert hasattr(ctypes.CDLL(build.lib_path(variant)), name), (variant, name)
    assert "head_loss.hip" in build.SOURCES
    # every entry point names the reference lines it stands for
    block = header[header.index("The training head fused with the language loss"):header.index("int care_head_live_rows")]
    assert "models/Head.py:26-32" in block and "misc/Crit/crit_lang.py:49-71" in block

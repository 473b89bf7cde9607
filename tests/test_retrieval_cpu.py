"""CPU: caption retrieval (care_amd/retrieval.py, csrc/retrieval.hip) without a GPU - the agreement of include/care_hip.h,
care_amd/_lib.py and both libraries on care_l2_normalize_rows / care_retrieval_query / care_retrieval_topk /
care_retrieval_gather, the refusals (all of them come before any launch), the float64 restatement against the genuine reference's
recorded ids (tests/golden/retrieval, tools/gen_retrieval_golden.py), the scan's O(1) eligibility rule against the reference's
walk, and the host side of `CaptionBank` / `attach_retrieval`."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import retrieval_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("care_l2_normalize_rows", "care_retrieval_query", "care_retrieval_topk", "care_retrieval_gather")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "retrieval", "*.npz")))


def test_header_binding_and_libraries_agree_on_the_retrieval_entry_points():
    from care_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "retrieval.hip" in build.SOURCES
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
    assert _lib.PLAIN["care_retrieval_scratch"] == (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int])
    assert set(ENTRY_POINTS) | {"care_retrieval_scratch"} <= set(_lib.exported_symbols())
    block = header[header.index("Caption retrieval"):header.index("int care_l2_normalize_rows")]
    for cite in ("pretreatment/clip_retrieval.py:47-83", ":175-176", ":305-321", "dataloader.py:808-814"):
        assert cite in block
    for variant in build.VARIANTS:
        assert _lib.load(variant=variant).care_version() == int(re.search(r"#define CARE_ABI_VERSION (\d+)", header).group(1))
        assert _lib.source_hash(variant) == build.source_hash(variant)


def test_the_host_checks_refuse_before_any_launch():
    """No device here: every call below must return before it launches anything."""
    from care_amd import _lib

    lib = _lib.load()
    # the scratch of a call: group maxima fp32 [B, 4 ceil(M / 64)], chosen groups int32 [B, topk], their count int32 [B],
    # candidate keys uint64 [B, topk, 16], each piece rounded up to 16 bytes
    assert lib.care_retrieval_scratch(1, 1000, 20) == 64 * 4 + 80 + 16 + 20 * 16 * 8
    assert lib.care_retrieval_scratch(37, 130260, 100) == 37 * 8144 * 4 + 37 * 100 * 4 + 160 + 37 * 100 * 128
    for bad in ((0, 1000, 20), (-1, 1000, 20), (1, 0, 20), (1, -5, 20), (1, 1000, 0), (1, 1000, 129), (1, 2 ** 31 - 1, 20)):
        assert lib.care_retrieval_scratch(*bad) < 0, bad
    big = 1 << 30

    def topk(q=64, bank=128, B=3, M=1000, D=512, k=20, start=None, end=None, first=None, prev=None, orig=None, ids=256, scores=512,
             count=1024, scratch=2048, nbytes=big):
        return lib.care_retrieval_topk(q, bank, B, M, D, k, start, end, first, prev, orig, ids, scores, count, scratch, nbytes, None)

    for null in ("q", "bank", "ids", "scores", "count", "scratch"):
        assert topk(**{null: None}) == EINVAL, null
    assert topk(first=4096) == EINVAL and topk(prev=4096) == EINVAL            # a `first` without a `prev`, and the reverse
    assert topk(start=4096) == EINVAL and topk(end=4096) == EINVAL
    assert topk(nbytes=lib.care_retrieval_scratch(3, 1000, 20) - 1) == EINVAL
    for D in (0, 8, 24, 500, 1040, 2048, -16):
        assert topk(D=D) == ESHAPE, D
    assert topk(k=0) == ESHAPE and topk(k=129) == ESHAPE and topk(M=0) == ESHAPE and topk(B=-1) == ESHAPE and topk(B=0) == ESHAPE
    assert topk(q=68) == EALIGN and topk(bank=136) == EALIGN and topk(scratch=2056) == EALIGN and topk(ids=260) == EALIGN
    assert topk(scores=514) == EALIGN and topk(count=1026) == EALIGN and topk(orig=4098) == EALIGN
    assert topk(start=4096, end=8194) == EALIGN and topk(first=4096, prev=8193) == EALIGN
    # the other three
    assert lib.care_l2_normalize_rows(None, 128, 10, 512, None) == EINVAL and lib.care_l2_normalize_rows(64, None, 10, 512, None) == EINVAL
    assert lib.care_l2_normalize_rows(64, 128, 0, 512, None) == ESHAPE and lib.care_l2_normalize_rows(64, 128, 10, 520, None) == ESHAPE
    assert lib.care_l2_normalize_rows(64, 128, 10, 1040, None) == ESHAPE and lib.care_l2_normalize_rows(68, 128, 10, 512, None) == EALIGN
    assert lib.care_retrieval_query(None, 128, 3, 28, 512, None) == EINVAL and lib.care_retrieval_query(64, None, 3, 28, 512, None) == EINVAL
    assert lib.care_retrieval_query(64, 128, -1, 28, 512, None) == ESHAPE and lib.care_retrieval_query(64, 128, 3, 0, 512, None) == ESHAPE
    assert lib.care_retrieval_query(64, 128, 3, 28, 100, None) == ESHAPE and lib.care_retrieval_query(64, 132, 3, 28, 512, None) == EALIGN
    assert lib.care_retrieval_gather(None, 10, 768, 128, 4, 256, None) == EINVAL and lib.care_retrieval_gather(64, 10, 768, None, 4, 256, None) == EINVAL
    assert lib.care_retrieval_gather(64, 10, 768, 128, 4, None, None) == EINVAL
    assert lib.care_retrieval_gather(64, 0, 768, 128, 4, 256, None) == ESHAPE and lib.care_retrieval_gather(64, 10, 776, 128, 4, 256, None) == ESHAPE
    assert lib.care_retrieval_gather(64, 10, 768, 128, 0, 256, None) == ESHAPE and lib.care_retrieval_gather(64, 10, 768, 132, 4, 256, None) == EALIGN
    assert lib.care_retrieval_gather(64, 10, 768, 128, 4, 264, None) == EALIGN


def _fixture(path):
    z = np.load(path)
    get = lambda k: z[k] if k in z else None
    return z["image_feats"], z["text_embs"], int(z["topk"]), get("info"), get("groups"), get("sampled_indices"), z["ids"]


def test_the_fixtures_are_the_five_cases():
    assert [os.path.basename(p)[:-4] for p in FIXTURES] == ["info", "plain", "sampled", "short", "unique"]
    assert all(os.path.getsize(p) < 200 * 1024 for p in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_the_restatement_reproduces_the_reference(path):
    frames, embs, topk, info, groups, sampled, ids = _fixture(path)
    got = R.retrieve_batch(frames, embs, topk, info, groups, sampled)
    assert got == [[int(v) for v in row if v >= 0] for row in ids]
    if os.path.basename(path) == "short.npz":
        assert len(got[0]) == 23 < topk


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_the_eligibility_rule_equals_the_walk(path):
    """The scan's O(1) mask over first / prev against `run`'s set logic: ranking the eligible columns alone gives what the walk
    over all columns gives, and the mask is exactly `the lowest member of the group outside the own range`."""
    from care_amd.retrieval import eligible, group_links, translate_ranges

    frames, embs, topk, info, groups, sampled, ids = _fixture(path)
    q, unit = R.query64(frames), R.unit_rows64(embs)
    index = np.arange(embs.shape[0]) if sampled is None else sampled
    first, prev = group_links([int(groups[j]) for j in index]) if groups is not None else (None, None)
    for b in range(frames.shape[0]):
        start, end = (0, 0) if info is None else (int(info[b][0]), int(info[b][1]))
        s, e = (start, end) if sampled is None else translate_ranges(sampled, [(start, end)])[0]
        mask = np.array([eligible(p, s, e, first, prev) for p in range(len(index))])
        for p, j in enumerate(index):                       # the rule, said the long way
            outside = not start <= j < end
            lower = [k for k in index[:p] if (groups is not None and groups[k] == groups[j]) and not start <= k < end]
            assert mask[p] == (outside and not lower), (b, p)
        scores = R.scores64(q[b], unit[index])
        got = R.ranked(scores[mask], index[mask])[:topk].tolist()
        assert got == [int(v) for v in ids[b] if v >= 0]


def test_grouping_and_groups_exact():
    from care_amd.retrieval import CaptionBank, group_links

    caps = ["a", "b", "a", "c", "b", "a"]
    first, prev = group_links(caps)
    assert first.tolist() == [0, 1, 0, 3, 1, 0] and prev.tolist() == [-1, -1, 0, -1, 1, 2]
    assert first.dtype == np.int32 and prev.dtype == np.int32
    embs = torch.arange(6 * 16, dtype=torch.float32).reshape(6, 16)
    assert CaptionBank._groups_exact(embs, caps) is False
    embs[2] = embs[0]; embs[5] = embs[0]; embs[4] = embs[1]
    assert CaptionBank._groups_exact(embs, caps) is True
    embs[5, 3] = float(np.nextafter(np.float32(embs[5, 3]), np.float32(np.inf)))     # one bit
    assert CaptionBank._groups_exact(embs, caps) is False
    embs[5] = embs[0]
    embs[0, 0], embs[2, 0], embs[5, 0] = 0.0, -0.0, 0.0                          # equal as numbers, not as bits
    assert CaptionBank._groups_exact(embs, caps) is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CaptionBank(embs, caps, unique=True, device="cpu")


def test_subset_range_translation():
    from care_amd.retrieval import translate_ranges

    sampled = np.array([2, 3, 7, 10, 11, 12, 20])
    ranges = [(3, 11), (0, 2), (4, 7), (8, 10), (12, 100), (0, 50), (5, 5), (10 ** 9, 10 ** 9)]
    got = translate_ranges(sampled, ranges)
    assert got.tolist() == [[1, 4], [0, 0], [2, 2], [3, 3], [5, 7], [0, 7], [2, 2], [7, 7]]
    for (s, e), (a, b) in zip(ranges, got):                       # positions a .. b - 1 are exactly the sampled indices in [s, e)
        assert [j for j in sampled if s <= j < e] == sampled[a:b].tolist()


class _Bank:
    def __init__(self):
        self.calls = []

    def retrieve(self, image_feats, topk, own_ranges=None):
        self.calls.append((image_feats, topk, own_ranges))
        return torch.full((image_feats.shape[0], topk, 8), 5.0), None, None, None


def test_attach_retrieval_places_the_stream_and_refuses():
    from care_amd import attach_retrieval
    from care_amd.configs import make_opt

    opt = make_opt("msrvtt_care")
    assert opt["modality"] == "amir" and opt["retrieval_topk"] == 20
    a, m, i = torch.zeros(2, 28, 4), torch.ones(2, 28, 4), torch.full((2, 28, 16), 2.0)
    bank = _Bank()
    out = attach_retrieval([a, m, i], opt, bank, own_ranges=[(0, 20), (20, 40)])
    assert len(out) == 4 and out[0] is a and out[1] is m and out[2] is i and out[3].shape == (2, 20, 8)
    assert bank.calls[0][0] is i and bank.calls[0][1] == 20 and bank.calls[0][2] == [(0, 20), (20, 40)]
    out = attach_retrieval([i, a], dict(opt, modality="ira", retrieval_topk=7), bank)
    assert out[0] is i and out[1].shape == (2, 7, 8) and out[2] is a and bank.calls[1][0] is i and bank.calls[1][2] is None
    with pytest.raises(ValueError, match="no retrieval stream"):
        attach_retrieval([a, m, i], dict(opt, modality="ami"), bank)
    with pytest.raises(ValueError, match="no image stream"):
        attach_retrieval([a, m], dict(opt, modality="amr"), bank)
    with pytest.raises(ValueError, match="feature tensors"):
        attach_retrieval([a, m, i, i], opt, bank)
    assert len(bank.calls) == 2

"""No GPU: the yardstick of the concept metrics (tests/concept_reference.py) pinned to the genuine reference's recorded numbers
(tests/golden/crit: NoisyOrMIL with calculate_mAP of misc/Crit/crit_attribute.py), the order rule on rows worked by hand, the
agreement of include/care_hip.h, care_amd/_lib.py and both libraries on care_concept_metrics, and its refusals - which are all
made on the host before anything is launched, so they run here.

The bar against the recorded numbers is the error of the reference's own fp32 evaluation: (P_max + 4) 2^-24 relative - a
P-term fp32 mean plus the divisions.  Measured (attr_b3, P_max = 63 within K, bar 3.99e-6): the helper is at most 8.7e-8 off the
record; care_amd.metrics.concept_metrics (fp32, torch's sort) at most 1.0e-7 off the helper."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import concept_reference as R
from crit_reference import criterion_batches, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ESHAPE = -1, -2, -3
NAMES = ["F1-%02d" % k for k in R.TOPK_LIST] + ["mAP"]


def _bar(labels, K):
    return (float((np.asarray(labels)[:, :K] != 0).sum(1).max()) + 4) * 2.0 ** -24


def test_the_helper_reproduces_the_recorded_reference():
    from care_amd.metrics import concept_metrics

    z = load_case("attr_b3")
    assert json.loads(str(z["info_names"])) == NAMES
    preds, labels = z["preds_attr"], z["labels_attr"]
    bar = _bar(labels, preds.shape[1])
    got = R.epoch([(preds, labels)])
    mine = concept_metrics(torch.from_numpy(preds), torch.from_numpy(labels))
    worst = [0.0, 0.0]
    for name, want in zip(NAMES, z["info"]):
        worst[0] = max(worst[0], abs(got[name] / want - 1))
        worst[1] = max(worst[1], abs(mine[name] / got[name] - 1))
        assert abs(got[name] - want) <= bar * abs(want), (name, got[name], want)
        assert abs(mine[name] - got[name]) <= bar * abs(got[name]), (name, mine[name], got[name])
    print("attr_b3: bar {:.3g}, helper vs record {:.3g}, concept_metrics vs helper {:.3g}".format(bar, *worst))
    assert got["n_no_positive"] == 0


def test_the_helper_reproduces_the_recorded_two_batches():
    z = load_case("criterion_two_batches")
    want = json.loads(str(z["info_json"]))
    batches = [(p.numpy(), y.numpy()) for _, _, p, y in criterion_batches(z)]
    bar = max(_bar(y, p.shape[1]) for p, y in batches)
    got = R.epoch(batches)
    for name in NAMES:
        assert abs(got[name] - want[name]) <= bar * abs(want[name]), (name, got[name], want[name])


def test_a_clip_without_a_positive_is_nan_where_the_reference_is():
    z = load_case("attr_b3_no_positive")
    preds, labels = z["preds_attr"], z["labels_attr"]
    got = R.epoch([(preds, labels)])
    assert np.isnan(z["info"]).any()
    for name, want in zip(NAMES, z["info"]):
        assert np.isnan(got[name]) == np.isnan(want), (name, got[name], want)
        if not np.isnan(want):
            assert abs(got[name] - want) <= _bar(labels, preds.shape[1]) * abs(want)
    assert got["n_no_positive"] == int(((labels[:, : preds.shape[1]] != 0).sum(1) == 0).sum()) >= 1
    res = R.batch(preds, labels)
    empty = res["n_pos"] == 0
    assert np.isnan(res["ap"][empty]).all() and np.isnan(res["f1"][empty]).all() and np.isfinite(res["ap"][~empty]).all()


f32 = np.float32
UP, DOWN = f32(np.inf), f32(-np.inf)
HAND = [
    # (name, preds, labels, the order of the columns, {positive column: (rank, posrank)}, AP)
    ("equal values: the lower column first", [0.5, 0.5, 0.5, 0.5], [0, 1, 0, 1], [0, 1, 2, 3], {1: (1, 0), 3: (3, 1)},
     (1 / 2 + 2 / 4) / 2),
    ("both clamp ends, both labels", [0.0, 0.005, 1.0, 0.995, 0.5, 0.001], [1, 0, 0, 1, 0, 1], [2, 3, 4, 0, 1, 5],
     {0: (3, 1), 3: (1, 0), 5: (5, 2)}, (1 / 2 + 2 / 4 + 3 / 6) / 3),
    ("NaN before every number, NaNs by column", [0.3, np.nan, 0.9, np.nan], [0, 0, 1, 1], [1, 3, 2, 0], {2: (2, 1), 3: (1, 0)},
     (1 / 2 + 2 / 3) / 2),
    ("exactly 0.01 and 0.99 are inside the clamp and equal to what it makes",
     [f32(0.01), 0.0, f32(0.99), 1.0, np.nextafter(f32(0.99), UP), np.nextafter(f32(0.01), DOWN), np.nextafter(f32(0.99), DOWN),
      np.nextafter(f32(0.01), UP)], [0, 1, 0, 0, 1, 1, 1, 0], [2, 3, 4, 6, 7, 0, 1, 5],
     {1: (6, 2), 4: (2, 0), 5: (7, 3), 6: (3, 1)}, (1 / 3 + 2 / 4 + 3 / 7 + 4 / 8) / 4),
    ("labels beyond K do not count; any non-zero label is a positive", [0.2, 0.8, 0.4], [2.0, 0, -1.0, 1, 1], [1, 2, 0],
     {0: (2, 1), 2: (1, 0)}, (1 / 2 + 2 / 3) / 2),
]


@pytest.mark.parametrize("name,preds,labels,order,ranks,ap", HAND, ids=[h[0].split(":")[0] for h in HAND])
def test_the_order_rule_on_rows_worked_by_hand(name, preds, labels, order, ranks, ap):
    preds = np.array(preds, dtype=np.float32)
    assert R.order(R.clamp32(preds)).tolist() == order, name
    got = R.clip(preds, np.array(labels, dtype=np.float32), topk=(1, 2, len(preds)))
    cols = sorted(ranks)
    assert got["n_pos"] == len(cols)
    assert got["rank"].tolist() == [ranks[c][0] for c in cols] and got["posrank"].tolist() == [ranks[c][1] for c in cols], name
    assert got["hits"] == [sum(r < k for r, _ in ranks.values()) for k in (1, 2, len(preds))]
    assert abs(got["ap"] - ap) <= 1e-15
    # the reference's own arithmetic on the same integers: torch's stable descending sort gives this order for numbers
    if not np.isnan(preds).any():
        t = torch.clamp(torch.from_numpy(preds), 0.01, 0.99)
        assert torch.sort(t, descending=True, stable=True)[1].tolist() == order


def test_f1_is_the_references_formula_on_counts():
    assert R.f1(0, 5, 3) == pytest.approx(2 * (1e-3 / 5) * (1e-3 / 3) / (1e-3 / 5 + 1e-3 / 3), rel=1e-15)
    assert R.f1(2, 5, 4) == pytest.approx(2 * 0.4 * 0.5 / 0.9, rel=1e-15)
    assert np.isnan(R.f1(0, 5, 0))


# ------------------------------------------------------------------------------------------------ header, binding, libraries
def test_header_binding_and_libraries_agree_on_care_concept_metrics():
    from care_amd import _lib, build

    name = "care_concept_metrics"
    header = open(os.path.join(ROOT, "include", "care_hip.h")).read()
    assert "concept_metrics.hip" in build.SOURCES
    build.build_all()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
    assert m, "include/care_hip.h does not declare " + name
    params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert params[-1] == "void* stream"
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(params)
    for ctype, decl in zip(sig, params):
        want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_int
        assert ctype is want, (decl, ctype)
    for variant in build.VARIANTS:
        lib = ctypes.CDLL(build.lib_path(variant))
        assert hasattr(lib, name), (variant, name)
        assert lib.care_version() == _lib.ABI_VERSION == 25, "the entry point is additive"
    bound = re.search(r"#define\s+CARE_CONCEPT_MAX_K\s+(\d+)", header)
    assert bound and int(bound.group(1)) == _lib.CONCEPT_MAX_K >= 4096
    assert int(re.search(r"#define\s+CARE_CONCEPT_MAX_TOPK\s+(\d+)", header).group(1)) == _lib.CONCEPT_MAX_TOPK == 8
    from care_amd import metrics
    assert callable(metrics.concept_metrics_device) and callable(metrics.concept_metrics)


@pytest.mark.parametrize("variant", ["", "f16"])
def test_refusals_are_made_on_the_host_before_anything_is_launched(variant):
    """Every refusal of include/care_hip.h with its code - on pointers that are never dereferenced (no launch happens)."""
    from care_amd import _lib, build

    build.build(variant=variant)
    lib = ctypes.CDLL(build.lib_path(variant))
    fn = lib.care_concept_metrics
    fn.restype, fn.argtypes = ctypes.c_int, _lib.SIGNATURES["care_concept_metrics"]
    P, Y, AP, H, N, TD, TI = (0x10000 * (i + 1) for i in range(7))   # aligned, never read
    tk = (ctypes.c_int32 * 8)(5, 10, 20, 30, 40, 50, 60, 70)

    def call(preds=P, ldp=500, labels=Y, ldl=500, B=4, K=500, topk=tk, n=6, ap=AP, hits=H, n_pos=N, td=TD, ti=TI):
        return fn(preds, ldp, labels, ldl, B, K, topk, n, ap, hits, n_pos, td, ti, None)

    assert call(preds=None) == EINVAL and call(labels=None) == EINVAL
    assert call(B=-1) == EINVAL and call(K=0) == EINVAL and call(K=-3) == EINVAL
    assert call(n=-1) == EINVAL and call(n=9) == EINVAL and call(topk=None) == EINVAL
    assert call(topk=(ctypes.c_int32 * 2)(5, 0), n=2) == EINVAL and call(topk=(ctypes.c_int32 * 2)(-1, 5), n=2) == EINVAL
    assert call(ldp=499) == EINVAL and call(ldl=499) == EINVAL
    assert call(td=None) == EINVAL and call(ti=None) == EINVAL, "the two totals only together"
    assert call(ap=None) == EINVAL and call(n_pos=None) == EINVAL and call(hits=None) == EINVAL, "totals are sums of the per-clip outputs"
    assert call(K=_lib.CONCEPT_MAX_K + 1, ldp=5000, ldl=5000) == ESHAPE
    assert call(K=49, ldp=49, ldl=49) == ESHAPE and call(K=5, ldp=5, ldl=5, n=2) == ESHAPE, "a k above K: the reference's topk raises"
    assert call(td=TD + 4) == EALIGN and call(ti=TI + 4) == EALIGN and call(ap=AP + 4) == EALIGN
    assert call(hits=H + 2) == EALIGN and call(n_pos=N + 1) == EALIGN and call(preds=P + 2) == EALIGN and call(labels=Y + 1) == EALIGN
    assert call(B=0) == 0, "no clips: a no-op"
    assert call(B=0, n=0, topk=None, hits=None) == 0

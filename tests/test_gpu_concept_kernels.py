"""GPU: care_concept_metrics (csrc/concept_metrics.hip) through the raw ABI against tests/concept_reference.py.

The integers - hits, n_pos, the totals' counts - must EQUAL the helper's.  ap and the double totals must lie within 1e-12
absolute: a clip's AP is a sum of at most 4096 quotients of integers in (0, 1] over their count, in double on both sides - the
kernel's fixed grouping against the helper's exactly rounded sum differ by a few ulps of 1.1e-16 of values <= 1; a batch's
totals are sums of at most 257 values <= 1 (257 ulps of 2.8e-14 at the worst).  An AP that equals the helper's to 1e-12 has the
helper's ranks: changing one rank r of a clip with P <= 4096 positives moves its AP by at least 1 / (P (r + 1) (r + 2)) > 1.4e-11.
Every output lies in a guarded buffer between canaries.

Shapes for the edges of the lane, wave and workgroup walk: K in {1, 5, 63, 64, 65, 500, 4096 = CARE_CONCEPT_MAX_K}, B in
{1, 3, 257}, padded row strides with positives in the unused label columns, P in {0, 1, 64, 65, K} positives a clip.

Measured on one MI355X: every integer equal; ap at most 1.1e-16 off the helper, a batch's totals at most 3.6e-15 (two calls over 257
clips); the 19 tests: 2.3 s."""
import functools

import numpy as np
import pytest
import torch

import concept_reference as R
from crit_reference import criterion_batches, load_case
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

GAP = 8
BAR = 1e-12
EINVAL, EALIGN, ESHAPE = -1, -2, -3
CANARY = {torch.int32: -77, torch.int64: -77, torch.float64: -7.25}
TOPK7 = (1,) + R.TOPK_LIST


def _guarded(n, dtype):
    whole = torch.full((n + 2 * GAP,), CANARY[dtype], dtype=dtype, device=DEV)
    return whole, whole[GAP:GAP + n]


def _intact(whole, n):
    w, fill = whole.cpu(), CANARY[whole.dtype]
    return bool((w[:GAP] == fill).all()) and bool((w[GAP + n:] == fill).all())


def _topk(K, full=TOPK7):
    return tuple(k for k in full if k <= K)


class Out(object):
    """Guarded outputs of one or several calls that add into the same totals."""

    def __init__(self, n_topk):
        self.n = n_topk
        self.td_w, self.td = _guarded(n_topk + 1, torch.float64)
        self.ti_w, self.ti = _guarded(2, torch.int64)
        self.td.zero_()
        self.ti.zero_()
        self.parts = []

    def call(self, preds, labels, K, topk, variant=""):
        """preds / labels: device fp32 [B, ld]; returns the status.  The per-clip outputs are kept for `collect`."""
        from care_amd import _lib
        import ctypes

        B = preds.shape[0]
        ap_w, ap = _guarded(B, torch.float64)
        h_w, h = _guarded(B * len(topk), torch.int32)
        n_w, n = _guarded(B, torch.int32)
        lib = _lib.load(variant=variant)
        rc = lib.care_concept_metrics(preds.data_ptr(), preds.stride(0), labels.data_ptr(), labels.stride(0), B, K,
                                      (ctypes.c_int32 * max(1, len(topk)))(*topk), len(topk), ap.data_ptr(), h.data_ptr(), n.data_ptr(),
                                      self.td.data_ptr(), self.ti.data_ptr(), _lib.stream_ptr())
        self.parts.append((B, ap_w, ap, h_w, h, n_w, n))
        return rc

    def collect(self):
        torch.cuda.synchronize()
        for B, ap_w, _, h_w, _, n_w, _ in self.parts:
            assert _intact(ap_w, B) and _intact(h_w, B * self.n) and _intact(n_w, B), "a per-clip output wrote past its end"
        assert _intact(self.td_w, self.n + 1) and _intact(self.ti_w, 2), "the totals wrote past their end"
        return {"ap": torch.cat([p[2] for p in self.parts]).cpu().numpy(),
                "hits": torch.cat([p[4].view(p[0], self.n) for p in self.parts]).cpu().numpy(),
                "n_pos": torch.cat([p[6] for p in self.parts]).cpu().numpy(),
                "totals_d": self.td.cpu().numpy().copy(), "totals_i": self.ti.cpu().numpy().copy()}


def _check(got, want, what):
    assert np.array_equal(got["hits"], want["hits"]), what
    assert np.array_equal(got["n_pos"], want["n_pos"]), what
    assert np.array_equal(got["totals_i"], want["totals_i"]), what
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(want["ap"])) and np.array_equal(np.isnan(want["ap"]), want["n_pos"] == 0), what
    assert np.array_equal(np.isnan(got["totals_d"]), np.isnan(want["totals_d"])), (what, got["totals_d"], want["totals_d"])
    err_ap, err_t = (float(np.abs(np.nan_to_num(got[k]) - np.nan_to_num(want[k])).max(initial=0.0)) for k in ("ap", "totals_d"))
    print("{}: ap off by {:.3g}, totals by {:.3g} (bar {:g})".format(what, err_ap, err_t, BAR))
    assert err_ap <= BAR and err_t <= BAR, (what, err_ap, err_t)


def _make(K, B, pad_p, pad_l, counts, seed, kind="random"):
    """preds [B, K + pad_p], labels [B, K + pad_l] (host fp32): clip b has counts[b % len] positives among its first K columns and
    ones in every unused label column; the unused prediction columns hold 2.0."""
    rng = np.random.RandomState(seed)
    preds = np.full((B, K + pad_p), 2.0, dtype=np.float32)
    labels = np.zeros((B, K + pad_l), dtype=np.float32)
    labels[:, K:] = 1.0
    if kind == "random":      # a tenth beyond either clamp bound, so both ends hold groups of equal values
        preds[:, :K] = rng.uniform(-0.12, 1.12, size=(B, K)).astype(np.float32)
    elif kind == "equal":
        preds[:, :K] = 0.5
    elif kind == "coarse":    # 7 distinct values: long runs of equal probabilities in the middle too
        preds[:, :K] = (rng.randint(0, 7, size=(B, K)) / 6.0).astype(np.float32)
    for b in range(B):
        P = min(counts[b % len(counts)], K)
        labels[b, rng.permutation(K)[:P]] = 1.0
    return preds, labels


def _run(preds, labels, K, topk, split=None, variant=""):
    out = Out(len(topk))
    p, y = torch.from_numpy(preds).to(DEV), torch.from_numpy(labels).to(DEV)
    for lo, hi in (split or [(0, preds.shape[0])]):
        assert out.call(p[lo:hi], y[lo:hi], K, topk, variant) == 0
    return out.collect()


SHAPES = [   # K, B, pad of preds, pad of labels, positives a clip
    (1, 3, 0, 0, (1, 0, 1)),
    (5, 1, 3, 0, (5,)),
    (5, 3, 0, 2, (0, 1, 5)),
    (63, 3, 1, 1, (1, 63, 0)),
    (64, 257, 0, 0, (64, 1, 0, 33)),
    (65, 3, 7, 3, (65, 64, 1)),
    (500, 257, 12, 20, (25, 0, 1, 64, 65, 500)),
    (500, 1, 0, 20, (65,)),
    (4096, 3, 0, 4, (4096, 65, 0)),
]


@pytest.mark.parametrize("K,B,pad_p,pad_l,counts", SHAPES, ids=["K{}-B{}".format(s[0], s[1]) for s in SHAPES])
def test_every_shape_against_the_helper(K, B, pad_p, pad_l, counts):
    preds, labels = _make(K, B, pad_p, pad_l, counts, seed=K * 1000 + B)
    topk = _topk(K)
    want = R.batch(preds[:, :K], labels, topk)
    assert set(min(c, K) for c in counts) <= set(want["n_pos"].tolist()), "positives in the unused columns must not count"
    _check(_run(preds, labels, K, topk), want, "K {} B {}".format(K, B))


@pytest.mark.parametrize("kind", ["equal", "coarse"])
def test_equal_probabilities_rank_by_column(kind):
    K, B = 500, 3
    preds, labels = _make(K, B, 4, 20, (25, 64, 500), seed=7, kind=kind)
    want = R.batch(preds[:, :K], labels, TOPK7)
    if kind == "equal":   # rank = column: hits_k = the positives among the first k columns
        assert want["hits"][0].tolist() == [int(labels[0, :k].sum()) for k in TOPK7]
    _check(_run(preds, labels, K, TOPK7), want, kind)


def _tie_rows():
    """K = 500: the first 41 columns at or above 0.99, the last 41 at or below 0.01, both groups with both labels - the case a sort
    without a rule leaves open -, a NaN column in the second clip (a positive) and in the third (a negative), all in between
    distinct."""
    K, B = 500, 4
    rng = np.random.RandomState(41)
    preds = rng.uniform(0.02, 0.98, size=(B, K + 5)).astype(np.float32)
    preds[:, :41] = rng.uniform(0.99, 1.5, size=(B, 41)).astype(np.float32)
    preds[:, 0] = np.float32(0.99)
    preds[:, K - 41:K] = rng.uniform(-0.5, 0.01, size=(B, 41)).astype(np.float32)
    preds[:, K - 1] = np.float32(0.01)
    labels = np.zeros((B, K + 9), dtype=np.float32)
    labels[:, 0:41:2] = 1.0
    labels[:, K - 40:K:3] = 1.0
    labels[:, 100:300:17] = 1.0
    labels[:, K:] = 1.0
    preds[1, 250], labels[1, 250] = np.nan, 1.0
    preds[2, 77], labels[2, 77] = np.nan, 0.0
    preds[2, 499] = np.nan
    labels[3, :K] = 0.0
    return K, preds, labels


def test_tie_groups_at_both_clamp_ends_and_nan_columns():
    K, preds, labels = _tie_rows()
    want = R.batch(preds[:, :K], labels, TOPK7)
    assert want["clips"][1]["rank"][list(np.nonzero(labels[1, :K])[0]).index(250)] == 0, "NaN comes before every number"
    assert want["hits"][0][TOPK7.index(40)] == 20 and want["n_pos"][3] == 0, "the first 40 of 41 equal columns, by column"
    got = _run(preds, labels, K, TOPK7)
    _check(got, want, "ties")
    assert np.isnan(got["ap"][3]) and np.isnan(got["totals_d"]).all() and got["totals_i"].tolist() == [4, 1]


@pytest.mark.parametrize("variant", ["", "f16"])
def test_the_golden_inputs_in_both_libraries(variant):
    for name in ("attr_b3", "attr_b3_no_positive"):
        z = load_case(name)
        preds, labels = z["preds_attr"], z["labels_attr"]
        K = preds.shape[1]
        got = _run(preds, labels, K, R.TOPK_LIST, variant=variant)
        _check(got, R.batch(preds, labels), name)
        info = R.scores(got["totals_d"], got["totals_i"])
        bar = (float(got["n_pos"].max()) + 4) * 2.0 ** -24   # the reference's own fp32 evaluation (tests/test_concept_metrics_cpu.py)
        for key, want in zip(["F1-%02d" % k for k in R.TOPK_LIST] + ["mAP"], z["info"]):
            assert np.isnan(info[key]) == np.isnan(want) and (np.isnan(want) or abs(info[key] - want) <= bar * abs(want)), (name, key)


def test_no_positive_is_nan_and_counted():
    K, B = 65, 5
    preds, labels = _make(K, B, 0, 3, (0, 3, 0, 65, 1), seed=3)
    got = _run(preds, labels, K, _topk(K))
    assert np.isnan(got["ap"][[0, 2]]).all() and np.isfinite(got["ap"][[1, 3, 4]]).all()
    assert got["n_pos"].tolist() == [0, 3, 0, 65, 1] and got["hits"][0].tolist() == [0] * len(_topk(K))
    assert got["totals_i"].tolist() == [5, 2] and np.isnan(got["totals_d"]).all(), "0 / 0 and x / 0, as the reference computes them"
    assert got["ap"][3] == 1.0, "every column a positive: every term is 1"


def test_a_split_batch_adds_up_and_a_clip_does_not_depend_on_its_batch():
    K, B = 500, 257
    preds, labels = _make(K, B, 12, 20, (25, 1, 64, 65, 500, 7), seed=11)
    want = R.batch(preds[:, :K], labels, TOPK7)
    one = _run(preds, labels, K, TOPK7)
    two = _run(preds, labels, K, TOPK7, split=[(0, 100), (100, 257)])
    _check(one, want, "one call")
    _check(two, want, "two calls")
    assert np.array_equal(one["ap"].view(np.int64), two["ap"].view(np.int64)), "a clip's bits depend on the clip alone"
    assert np.array_equal(one["hits"], two["hits"]) and np.array_equal(one["n_pos"], two["n_pos"])
    assert np.array_equal(one["totals_i"], two["totals_i"])
    assert float(np.abs(one["totals_d"] - two["totals_d"]).max()) <= BAR


def test_the_same_call_twice_gives_the_same_bits():
    K, preds, labels = _tie_rows()
    a, b = _run(preds, labels, K, TOPK7), _run(preds, labels, K, TOPK7)
    for key in ("ap", "totals_d"):
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    for key in ("hits", "n_pos", "totals_i"):
        assert np.array_equal(a[key], b[key]), key


def test_optional_outputs_and_list_lengths():
    """No per-clip output at all (nothing is written), eight entries, none; per-clip outputs without totals."""
    from care_amd import _lib
    import ctypes

    K, B = 64, 3
    preds, labels = _make(K, B, 0, 0, (5, 64, 1), seed=5)
    p, y = torch.from_numpy(preds).to(DEV), torch.from_numpy(labels).to(DEV)
    lib = _lib.load()
    eight = (1, 2, 3, 5, 8, 13, 21, 64)
    want = R.batch(preds, labels, eight)
    _check(_run(preds, labels, K, eight), want, "eight entries")
    none = _run(preds, labels, K, ())
    assert abs(none["totals_d"][0] - want["totals_d"][-1]) <= BAR and none["totals_i"].tolist() == [3, 0]
    ap_w, ap = _guarded(B, torch.float64)
    h_w, h = _guarded(B * 8, torch.int32)
    n_w, n = _guarded(B, torch.int32)
    tk = (ctypes.c_int32 * 8)(*eight)
    for args in ((ap, None, None), (None, h, None), (None, None, n), (None, None, None)):
        a, b, c = (None if t is None else t.data_ptr() for t in args)
        assert lib.care_concept_metrics(p.data_ptr(), K, y.data_ptr(), K, B, K, tk, 8, a, b, c, None, None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _intact(ap_w, B) and _intact(h_w, B * 8) and _intact(n_w, B)
    assert np.array_equal(h.view(B, 8).cpu().numpy(), want["hits"]) and np.array_equal(n.cpu().numpy(), want["n_pos"])
    assert float(np.abs(ap.cpu().numpy() - want["ap"]).max()) <= BAR


def test_every_refusal_returns_its_code_and_leaves_the_outputs_alone():
    from care_amd import _lib
    import ctypes

    K, B = 500, 4
    preds, labels = _make(K, B, 0, 0, (25,), seed=9)
    p, y = torch.from_numpy(preds).to(DEV), torch.from_numpy(labels).to(DEV)
    big = torch.zeros(2, _lib.CONCEPT_MAX_K + 1, device=DEV)
    lib = _lib.load()
    ap_w, ap = _guarded(B, torch.float64)
    h_w, h = _guarded(B * 6, torch.int32)
    n_w, n = _guarded(B, torch.int32)
    td_w, td = _guarded(7 + 1, torch.float64)   # (room for the misaligned pointers below)
    ti_w, ti = _guarded(2 + 1, torch.int64)
    tk = (ctypes.c_int32 * 6)(*R.TOPK_LIST)
    base = dict(preds=p.data_ptr(), ldp=K, labels=y.data_ptr(), ldl=K, B=B, K=K, topk=tk, n=6, ap=ap.data_ptr(), hits=h.data_ptr(),
                n_pos=n.data_ptr(), td=td.data_ptr(), ti=ti.data_ptr())

    def call(**over):
        a = dict(base, **over)
        return lib.care_concept_metrics(a["preds"], a["ldp"], a["labels"], a["ldl"], a["B"], a["K"], a["topk"], a["n"], a["ap"],
                                        a["hits"], a["n_pos"], a["td"], a["ti"], _lib.stream_ptr())

    assert call(preds=None) == EINVAL and call(labels=None) == EINVAL and call(B=-1) == EINVAL
    assert call(K=0) == EINVAL and call(n=-1) == EINVAL and call(n=9) == EINVAL
    assert call(topk=(ctypes.c_int32 * 6)(5, 10, 0, 30, 40, 50)) == EINVAL and call(topk=(ctypes.c_int32 * 6)(5, 10, -20, 30, 40, 50)) == EINVAL
    assert call(ldp=K - 1) == EINVAL and call(ldl=K - 1) == EINVAL
    assert call(td=None) == EINVAL and call(ti=None) == EINVAL and call(ap=None) == EINVAL
    wide = _lib.CONCEPT_MAX_K + 1
    assert call(preds=big.data_ptr(), labels=big.data_ptr(), B=2, K=wide, ldp=wide, ldl=wide) == ESHAPE
    assert call(K=49) == ESHAPE, "a k above K: the reference's topk(50) raises there"
    assert call(td=td.data_ptr() + 4) == EALIGN and call(ti=ti.data_ptr() + 4) == EALIGN and call(ap=ap.data_ptr() + 4) == EALIGN
    assert call(B=0) == 0
    torch.cuda.synchronize()
    for whole in (ap_w, h_w, n_w, td_w, ti_w):
        assert bool((whole.cpu() == CANARY[whole.dtype]).all()), "a refused call wrote"
    # and the Python caller: device tensors only, the kernel's refusals as CareHipError
    from care_amd.metrics import concept_metrics_device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        concept_metrics_device(torch.from_numpy(preds), y)
    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        concept_metrics_device(p[:, :49], y)
    (d, i), per = concept_metrics_device(p, y, per_clip=True)
    want = R.batch(preds, labels)
    assert np.array_equal(per["hits"].cpu().numpy(), want["hits"]) and i.tolist() == [4, 0]
    assert float(np.abs(d.cpu().numpy() - want["totals_d"]).max()) <= BAR

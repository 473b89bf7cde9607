"""GPU, raw ABI: care_sample_logits / care_sample_accum (csrc/sample.hip) against tests/sample_reference.py, the float64
restatement with the bit-exact hash.

Shapes: V in {1, 2, 63, 64, 65, 255, 256, 257, 1025, 10547} (+ 16500: beyond the 16384 columns a workgroup keeps in
registers), rows in {1, 3, 130}, ld = V and V + 5 (padding columns hold 1e30; canaries sit around every output).
Settings: temperature in {0.25, 1, 4}, top_k in {0, 1, 2, V - 1, V, V + 3}, top_p in {1, 0.9, 0.5, 1e-6}, alone and combined.
Rows (cycled through every launch): Gaussian logits x 2; one logit 50 above the rest; all equal; -inf runs at the start, at
the end and at every 64-column boundary; exact duplicates of the maximum and of the k-th value.

Bars: the token and the size of the kept set equal the reference's; psum within 1e-5 relative, logq and -log psum within
2e-5 absolute of float64 (fp32 sums of <= 16500 terms in a tree: ~log2(V) roundings of 6e-8 on a sum of positive terms,
plus the 1-ulp exponentials and one logarithm).
Margin rule: a row whose reference Gumbel margin is under 1e-4 (8 fp32 ulps at |value| <= 64, rounded up) or whose nucleus
margin is under 1e-5 would be left out of the token check - at most 1 % of the rows.  The launches are CONSTRUCTED on the CPU
so that the reference leaves out none: such a row is drawn again with its next seed (at temperature 4 the entries around
a nucleus cut of V = 10547 weigh ~5e-5 each, so every third random row lies within 1e-5 of its cut), and a special row
whose cut falls exactly on a run of equal values (all-equal logits with top_p 0.5 over an even count: cumulative mass
exactly 0.5) gives its slot to a Gaussian row.  `build_launch` asserts this before anything touches the device.
"""
import numpy as np
import pytest
import torch

import sample_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("gauss", "peak", "equal", "ninf_start", "ninf_end", "ninf_bound", "dup_max", "dup_kth")
CANARY_F, CANARY_I, PAD = 7.25e11, -77777777, 4
VS = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 10547)


def settings(V):
    """(temperature, top_k, top_p): every value alone, then combined."""
    ks = (1, 2, V - 1, V, V + 3)
    out = [(1.0, 0, 1.0)] + [(1.0, k, 1.0) for k in ks] + [(1.0, 0, p) for p in (0.9, 0.5, 1e-6)] + [(0.25, 0, 1.0), (4.0, 0, 1.0)]
    out += [(0.25, 2, 0.9), (4.0, V - 1, 0.5), (1.0, V + 3, 1e-6), (4.0, 2, 0.5), (0.25, V - 1, 0.9), (1.0, 1, 0.5), (4.0, V, 0.9),
            (0.25, 0, 0.5), (4.0, 0, 0.9), (0.25, V, 1e-6), (4.0, max(V // 3, 1), 0.9), (0.25, max(V // 2, 1), 0.5)]
    return out


def make_row(rng, kind, V, top_k):
    x = (rng.standard_normal(V) * 2).astype(np.float32)
    if kind == "peak":
        x[rng.integers(V)] = x.max() + 50
    elif kind == "equal":
        x[:] = 0.75
    elif kind == "ninf_start":
        x[: min(V - 1, 70)] = -np.inf
    elif kind == "ninf_end":
        x[V - min(V - 1, 70):] = -np.inf
    elif kind == "ninf_bound" and V > 64:
        x[63::64] = -np.inf
        x[64::64] = -np.inf
    elif kind == "dup_max" and V >= 4:
        x[rng.choice(V, 3, replace=False)] = x.max() + 0.5
    elif kind == "dup_kth" and V >= 4:
        k = top_k if 0 < top_k < V else 2
        order = np.argsort(-x, kind="stable")
        low = order[k:]
        x[rng.choice(low, min(2, low.size), replace=False)] = x[order[k - 1]]
    return x


def build_launch(V, rows, li, setting, t=3):
    """Logits, keys, seed and the reference of one launch, with no row that the margin rule would leave out: every row is
    drawn again (its next seed) until the reference decides it with room to spare."""
    temperature, top_k, top_p = setting
    rng = np.random.default_rng([V, rows, li])
    seed = int(rng.integers(1, 2 ** 63))
    keys = rng.permutation(4 * rows + 7)[:rows].astype(np.int32)
    xs, refs = [], []
    for r in range(rows):
        kind = KINDS[(r + li) % len(KINDS)]
        for attempt in range(60):
            x = make_row(np.random.default_rng([V, rows, li, r, attempt]), kind, V, top_k)
            ref = R.sample_row(x, seed, int(keys[r]), t, temperature, top_k, top_p)
            if ref["gumbel_margin"] >= 1e-4 and ref["nucleus_margin"] >= 1e-5:
                break
            if ref["nucleus_margin"] < 1e-5 and attempt >= 3:
                kind = "gauss"   # (a run of equal values that the cut meets exactly: see the module's docstring)
        else:
            raise AssertionError("no row without a marginal decision in 60 seeds: {}".format((V, rows, li, r, setting)))
        xs.append(x)
        refs.append(ref)
    out = {k: np.array([q[k] for q in refs]) for k in refs[0] if k != "kept"}
    left_out = (out["gumbel_margin"] < 1e-4) | (out["nucleus_margin"] < 1e-5)
    assert int(left_out.sum()) * 100 <= rows and not left_out.any()   # the rule's 1 %; by construction none
    return np.stack(xs), keys, seed, out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def params_block(seed, temperature, top_k, top_p):
    blk = torch.zeros(32, dtype=torch.uint8, device=DEV)
    blk[:24] = torch.frombuffer(bytearray(R.pack_params(seed, temperature, top_k, top_p)), dtype=torch.uint8).to(DEV)
    return blk


def run_kernel(x, ld, keys, t, seed, setting, variant="", logq=True, nkept=True):
    """One launch; returns (pmax, pidx, psum, logq, nkept) as numpy arrays (None where not asked for), canaries checked."""
    from care_amd import _lib

    rows, V = x.shape
    buf = np.full((rows, ld), 1e30, dtype=np.float32)
    buf[:, :V] = x
    logits, prm = dev(buf), params_block(seed, *setting)
    fo = torch.full((3, rows + 2 * PAD), CANARY_F, dtype=torch.float32, device=DEV)
    io = torch.full((2, rows + 2 * PAD), CANARY_I, dtype=torch.int32, device=DEV)
    fp = lambda i: fo[i].data_ptr() + 4 * PAD
    ip = lambda i: io[i].data_ptr() + 4 * PAD
    kd = dev(keys) if keys is not None else None
    _lib.call("care_sample_logits", logits.data_ptr(), ld, V, rows, kd.data_ptr() if kd is not None else None, t, prm.data_ptr(),
              fp(0), ip(0), fp(1), fp(2) if logq else None, ip(1) if nkept else None, variant=variant)
    torch.cuda.synchronize()
    f, i = fo.cpu().numpy(), io.cpu().numpy()
    assert (f[:, :PAD] == np.float32(CANARY_F)).all() and (f[:, PAD + rows:] == np.float32(CANARY_F)).all()
    assert (i[:, :PAD] == CANARY_I).all() and (i[:, PAD + rows:] == CANARY_I).all()
    if not logq:
        assert (f[2] == np.float32(CANARY_F)).all()
    if not nkept:
        assert (i[1] == CANARY_I).all()
    body = slice(PAD, PAD + rows)
    return f[0, body], i[0, body], f[1, body], f[2, body] if logq else None, i[1, body] if nkept else None


def check(x, got, ref, what):
    pmax, pidx, psum, logq, nkept = got
    rows = x.shape[0]
    assert pidx.tolist() == ref["tok"].tolist(), what
    assert nkept.tolist() == ref["nkept"].tolist(), what
    assert (pmax == x[np.arange(rows), pidx]).all(), what
    rel = np.abs(psum.astype(np.float64) / ref["psum"] - 1).max()
    dq = np.abs(logq.astype(np.float64) - ref["logq"]).max()
    dp = np.abs(-np.log(psum.astype(np.float64)) - ref["logp_model"]).max()
    print(what, "psum rel %.2e  logq abs %.2e  logp abs %.2e" % (rel, dq, dp))
    assert rel <= 1e-5 and dq <= 2e-5 and dp <= 2e-5, what


@pytest.mark.parametrize("V", VS)
def test_sampler_matches_the_reference(V):
    li = 0
    for rows in (1, 3, 130):
        for ld in (V, V + 5):
            todo = settings(V)
            if rows == 130 and V > 2000:   # (the float64 reference costs 1.4 ms per row of 10547: every fifth setting, offset by ld)
                todo = todo[2 * (ld - V) // 5::5]
            for setting in todo:
                x, keys, seed, ref = build_launch(V, rows, li, setting)
                check(x, run_kernel(x, ld, keys, 3, seed, setting), ref, (V, rows, ld, setting))
                li += 1


def test_columns_beyond_the_register_file():
    """V = 16500 > 16 x 1024: the last columns are re-read from memory in every pass; the maximum, a duplicate of the k-th value
    and the drawn token are made to lie there in turn."""
    V = 16500
    for n, setting in enumerate([(1.0, 0, 1.0), (1.0, 40, 1.0), (0.25, 0, 0.9), (4.0, 16499, 0.5), (1.0, 3, 1e-6)]):
        for li in range(10 * n, 10 * n + 10):   # (the planted values move the margins: the first launch that keeps them wide)
            x, keys, seed, _ = build_launch(V, 3, li, setting)
            x[1, 16450] = x[1].max() + 3
            x[2, 16390] = np.sort(x[2])[-3]
            ref = R.sample_rows(x, seed, keys, 3, *setting)
            if not ((ref["gumbel_margin"] < 1e-4) | (ref["nucleus_margin"] < 1e-5)).any():
                break
        else:
            raise AssertionError("no launch without a marginal row")
        check(x, run_kernel(x, V + 5, keys, 3, seed, setting), ref, (V, setting))


def test_null_forms_permutation_repeat_and_the_second_library():
    V, rows, setting = 1025, 130, (0.7, 50, 0.9)
    x, keys, seed, ref = build_launch(V, rows, 5, setting)
    full = run_kernel(x, V + 5, keys, 3, seed, setting)
    check(x, full, ref, "full")
    # logq / nkept NULL: the other outputs are the same bits, the buffers untouched
    bare = run_kernel(x, V + 5, keys, 3, seed, setting, logq=False, nkept=False)
    for a, b in zip(full[:3], bare[:3]):
        assert a.tobytes() == b.tobytes()
    # row_key NULL = the row index
    ident = run_kernel(x, V, None, 3, seed, setting)
    explicit = run_kernel(x, V, np.arange(rows, dtype=np.int32), 3, seed, setting)
    for a, b in zip(ident, explicit):
        assert a.tobytes() == b.tobytes()
    assert ident[1].tolist() != full[1].tolist()   # (other keys: other draws)
    # rows permuted together with their keys: the outputs permuted, bit for bit - also in a batch of another size
    perm = np.random.default_rng(9).permutation(rows)
    moved = run_kernel(x[perm], V + 5, keys[perm], 3, seed, setting)
    for a, b in zip(full, moved):
        assert a[perm].tobytes() == b.tobytes()
    part = run_kernel(x[perm[:7]], V, keys[perm[:7]], 3, seed, setting)
    for a, b in zip(full, part):
        assert a[perm[:7]].tobytes() == b.tobytes()
    # twice: identical bits; another step or seed: another draw
    again = run_kernel(x, V + 5, keys, 3, seed, setting)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    assert run_kernel(x, V + 5, keys, 4, seed, setting)[1].tolist() != full[1].tolist()
    assert run_kernel(x, V + 5, keys, 3, seed + 1, setting)[1].tolist() != full[1].tolist()
    # the fp16 library carries the same fp32 kernel
    other = run_kernel(x, V + 5, keys, 3, seed, setting, variant="f16")
    for a, b in zip(full, other):
        assert a.tobytes() == b.tobytes()


def test_error_codes_and_the_logq_accumulator():
    from care_amd import _lib

    for variant in ("", "f16"):
        lib = _lib.load(variant=variant)
        f = torch.zeros(64, device=DEV)
        i = torch.zeros(64, dtype=torch.int32, device=DEV)
        prm = params_block(1, 1.0, 0, 1.0)
        ok = dict(logits=f.data_ptr(), ld=8, V=8, rows=2, key=None, t=1, params=prm.data_ptr(), pmax=f.data_ptr() + 128,
                  pidx=i.data_ptr(), psum=f.data_ptr() + 192)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.care_sample_logits(a["logits"], a["ld"], a["V"], a["rows"], a["key"], a["t"], a["params"], a["pmax"], a["pidx"],
                                          a["psum"], None, None, None)
        assert call() == 0 and call(rows=0) == 0
        for bad in (dict(rows=-1), dict(V=0), dict(ld=7), dict(t=0), dict(logits=None), dict(params=None), dict(pmax=None),
                    dict(pidx=None), dict(psum=None)):
            assert call(**bad) == -1, bad
        assert call(params=prm.data_ptr() + 8) == -2
        torch.cuda.synchronize()
        # care_sample_accum: score_q += logq on the rows that have not ended
        rows = 700
        rng = np.random.default_rng(4)
        lq, fin = rng.standard_normal(rows).astype(np.float32), (rng.random(rows) < 0.4).astype(np.int32)
        sq = rng.standard_normal(rows + 2).astype(np.float32)
        d, dl, df = dev(sq), dev(lq), dev(fin)
        _lib.call("care_sample_accum", dl.data_ptr(), df.data_ptr(), d.data_ptr() + 4, rows, variant=variant)
        torch.cuda.synchronize()
        want = sq.copy()
        want[1:-1] += np.where(fin == 0, lq, np.float32(0))
        assert d.cpu().numpy().tobytes() == want.tobytes()
        assert lib.care_sample_accum(None, i.data_ptr(), f.data_ptr(), 1, None) == -1 and lib.care_sample_accum(f.data_ptr(), i.data_ptr(), f.data_ptr(), 0, None) == 0

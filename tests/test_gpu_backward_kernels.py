"""GPU: the kernels of training mode, one by one, against float64 references.

csrc/backward.hip (LayerNorm backward, activation, dropout, broadcast / scatter-add helpers, concept-head backward,
care_attn_pv and care_attn_bwd in their one-wave and matrix-core forms), care_attention_probs (both forms, csrc/attention.hip)
and care_split_pieces (csrc/gemm_tile.hip) called directly through the C ABI - tests/test_gpu_training.py reaches them only
through whole models at 2 - 4 clips with every dropout probability 0.

How a comparison is judged (`_check`).  The reference is plain torch in float64 on the CPU (autograd where a gradient is
wanted).  The YARDSTICK is not the kernel: the same formula evaluated by torch in fp32 on the same inputs (torch's own fp32
autograd), its largest error against the float64 reference, per case.  A kernel passes when every element's error is at most
    4 x yardstick + 2^-22 x scale
(4 x: another summation order may lose two more bits than torch's, not more; the floor: entries that are zero in exact
arithmetic).  `scale` is the largest magnitude of the reference tensor, or - sums over many rows: dgamma, dbeta, dbias,
scatter-add - per element the float64 sum of the absolute terms (plus the magnitude of what the buffer held before: the
accumulate contracts add to it).  Statistical bounds (dropout) and representation bounds (care_split_pieces) are derived where
they stand.

Which geometry reaches which attention kernel:
    care_attn_bwd         seq <= 32 -> attn_bwd_mfma_kernel;  seq 33, 40 -> attn_bwd_kernel (one wave; 128 keys: 67 KB dynamic LDS)
    care_attn_pv          seq <= 32 and nkeys <= 128 -> attn_pv_mfma_kernel;  seq 33, 40 or nkeys 130 -> attn_pv_kernel
    care_attention_probs  fp32 keys, 8 <= seq <= 32, whole sequences, rows_per_kv = seq -> attention_probs_seq_kernel;
                          seq 1, 7, 33, bf16 keys, rows_per_kv 1 / 5 -> attention_probs_kernel
    care_ln_bwd           d <= 512 -> ln_bwd_kernel<8>;  d <= 1024 -> <16>;  d <= 2048 -> <32>

Measured on one MI355X (worst kernel error / yardstick over the cases whose yardstick is not 0, and worst error / bar):
    test                                               error / yardstick   error / bar
    care_ln_bwd, 11 d x rows 1 .. 58 (440 cases)               2.66             0.32
    care_ln_bwd, 1856 and 14851 rows                           2.60             0.23
    care_attn_pv / care_attn_bwd, real geometries              1.34             0.27
    care_attn_pv / care_attn_bwd, tile edges                   2.95             0.51   (dK at seq 1, 128 keys)
    care_attn_pv / care_attn_bwd, heads 4 / 12 / 16            1.56             0.27
    care_attn_pv / care_attn_bwd, one-wave forms               2.55             0.28
    care_attn_pv / care_attn_bwd, 512 sequences                1.04             0.19
    care_attn_pv, 130 keys                                     0.73             0.16
    care_attention_probs, matrix-core / row form               1.00 / 1.01      0.25
    care_act none, ReLU / GELU                                 exact / 1.00     0 / 0.25
    care_bcast_rows, care_add_pos_sem, care_concept_bwd        1.00             0.10 / 0.13 / 0.21
    care_scatter_add_rows                                      1.51             0.22
(two runs; the figures of the kernels that add with atomics move by a few tenths between runs.)  care_dropout: keep rates
0.899804 / 0.499703 at p 0.1 / 0.5 (0.67 / 0.61 sigma); 16 sites' masks: worst share 0.50308 (5 sigma: 0.5 +- 0.00488) - with the
stepped seeds this file's fix replaced, 20 of the 480 shares were exactly 1.0.  care_split_pieces: |(hi + lo) 2^-e - src| at
most 2^-23.2 of |max|.  The whole file: 10 s.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 2.0 ** -22
FACTOR = 4.0


def _call(name, *args):
    from care_amd import _lib

    _lib.call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _leaf(t, dt):
    """A fresh autograd leaf of dtype `dt` (never the caller's tensor itself)."""
    return t.detach().clone().to(dt).requires_grad_(True)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _padded(t, ld, extra_rows=1):
    """`t` [rows, d] (CPU) as a view into a NaN-filled device buffer [rows + extra_rows, ld]."""
    buf = _nan(t.shape[0] + extra_rows, ld)
    view = buf[:t.shape[0], :t.shape[1]]
    view.copy_(t)
    return buf, view


def _only_inside_written(buf, rows, cols):
    """Nothing left NaN inside [rows, cols] of a NaN-filled buffer, nothing written outside."""
    assert not torch.isnan(buf[:rows, :cols]).any(), "NaN left inside"
    assert torch.isnan(buf[rows:]).all() and torch.isnan(buf[:, cols:]).all(), "written outside the matrix"


class _Worst:
    """Worst kernel error / yardstick and error / bar of one test, printed at its end (pytest -s shows it)."""

    def __init__(self, name):
        self.name, self.ratio, self.of_bar, self.at = name, 0.0, 0.0, None

    def report(self):
        print("{}: worst kernel error / yardstick {:.3g}, worst error / bar {:.3g} at {}".format(self.name, self.ratio, self.of_bar, self.at))


def _check(worst, what, got, ref64, yard32, bound=None):
    """got: the kernel's fp32 result; ref64: the float64 reference; yard32: torch's fp32 evaluation of the same formula;
    bound: per-element float64 sum of absolute terms (sums over many rows) or None (the reference's largest magnitude)."""
    got = got.detach().double().cpu()
    ref64 = ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), (what, "non-finite output")
    err = (got - ref64).abs()
    yard = float((yard32.detach().double().cpu() - ref64).abs().max())
    floor = FLOOR * (float(ref64.abs().max()) if bound is None else bound.detach().double().cpu())
    bar = FACTOR * yard + floor
    e = float(err.max())
    if yard > 0.0 and e / yard > worst.ratio:
        worst.ratio = e / yard
    of_bar = float((err / torch.as_tensor(bar).clamp_min(1e-300)).max()) if e > 0.0 else 0.0
    if of_bar > worst.of_bar:
        worst.of_bar, worst.at = of_bar, what
    assert bool((err <= bar).all()), (what, "error", e, "yardstick", yard, "error / bar", of_bar)


# ====================================================================================================== 1. care_ln_bwd
LN_D = [64, 100, 256, 500, 512, 513, 768, 1024, 1025, 2047, 2048]


def _ln_case(worst, rows, d, with_res, eps, padded):
    g = _gen(rows, d, with_res, int(eps * 1e12), padded)
    x = torch.randn(rows, d, generator=g) * 1.5 + 0.3
    res = torch.randn(rows, d, generator=g) if with_res else None
    gamma = torch.randn(d, generator=g)                       # mixed sign
    dy = torch.randn(rows, d, generator=g)
    dg0, db0 = torch.randn(d, generator=g) * 3.0, torch.randn(d, generator=g) * 3.0   # earlier contents of the accumulators

    def run(dt):
        s = (x + res) if with_res else x                      # the sum is fp32 in the kernel and in the reference
        s, ga, be = _leaf(s, dt), _leaf(gamma, dt), torch.zeros(d, dtype=dt, requires_grad=True)
        y = torch.nn.functional.layer_norm(s, (d,), ga, be, eps)
        y.backward(dy.to(dt))
        return s.detach(), s.grad, dg0.to(dt) + ga.grad, db0.to(dt) + be.grad

    s64, ds64, dg64, db64 = run(torch.float64)
    _, ds32, dg32, db32 = run(torch.float32)
    with torch.no_grad():
        xh = torch.nn.functional.layer_norm(s64, (d,), None, None, eps)
        dg_bound = dg0.double().abs() + (dy.double() * xh).abs().sum(0)
        db_bound = db0.double().abs() + dy.double().abs().sum(0)

    ldx, ldres, lddy, ldds = (d + 3, d + 5, d + 1, d + 7) if padded else (d, d, d, d)
    _, xd = _padded(x, ldx)
    resd = _padded(res, ldres)[1] if with_res else None
    _, dyd = _padded(dy, lddy)
    dsb = _nan(rows + 2, ldds)
    acc = _nan(2, d + 3)
    acc[0, :d], acc[1, :d] = dg0.to(DEV), db0.to(DEV)
    gd = gamma.to(DEV)
    _call("care_ln_bwd", _p(xd), ldx, _p(resd), ldres if with_res else 0, _p(gd), _p(dyd), lddy, eps, _p(dsb), ldds,
          _p(acc[0]), _p(acc[1]), rows, d)
    torch.cuda.synchronize()
    what = "ln_bwd rows {} d {} res {} eps {} padded {}".format(rows, d, with_res, eps, padded)
    _only_inside_written(dsb, rows, d)
    assert torch.isnan(acc[:, d:]).all(), what                 # nothing added past column d
    _check(worst, what + " ds", dsb[:rows, :d], ds64, ds32)
    _check(worst, what + " dgamma", acc[0, :d], dg64, dg32, dg_bound)
    _check(worst, what + " dbeta", acc[1, :d], db64, db32, db_bound)


@pytest.mark.parametrize("d", LN_D)
def test_ln_bwd_against_float64_autograd(d):
    """ds, dgamma, dbeta of LayerNorm(x (+ res)) against float64 autograd: rows round the 16-rows-per-workgroup edge, with and
    without the residual, both eps of the configurations, dense and padded leading dimensions (each different); dgamma / dbeta
    ACCUMULATE into what the buffers held; a NaN-filled ds keeps its NaNs outside the matrix."""
    worst = _Worst("care_ln_bwd d={}".format(d))
    for rows in (1, 15, 16, 17, 58):
        for with_res in (False, True):
            for eps in (1e-12, 1e-5):
                for padded in (False, True):
                    _ln_case(worst, rows, d, with_res, eps, padded)
    worst.report()


@pytest.mark.parametrize("rows,d", [(1856, 512), (1856, 1024), (14848 + 3, 512), (14848 + 3, 1024)])
def test_ln_bwd_many_rows(rows, d):
    """64 and 512 clips x 29 positions (+ 3: a ragged last workgroup): 116 / 929 workgroups add to each dgamma / dbeta."""
    worst = _Worst("care_ln_bwd rows={} d={}".format(rows, d))
    _ln_case(worst, rows, d, True, 1e-12, False)
    _ln_case(worst, rows, d, False, 1e-5, True)
    worst.report()


def test_ln_bwd_rejects_d_above_2048():
    from care_amd import _lib

    rows, d = 4, 2049
    x, dy, ds = torch.zeros(rows, d, device=DEV), torch.zeros(rows, d, device=DEV), torch.zeros(rows, d, device=DEV)
    gam, dg, db = torch.ones(d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        _call("care_ln_bwd", _p(x), d, None, 0, _p(gam), _p(dy), d, 1e-12, _p(ds), d, _p(dg), _p(db), rows, d)


# ============================================================================ 2. care_attn_pv / care_attn_bwd, dropout included
def _dropout_mask(n, p, seed):
    """care_dropout on ones: keep / (1 - p) per flat index - by contract the mask care_attn_pv and care_attn_bwd re-create
    from (seed, flat index into P) (attn_keep / dropout_kernel share b_uniform)."""
    if p <= 0.0:
        return torch.ones(n)
    ones = torch.ones(n, device=DEV)
    out = torch.empty_like(ones)
    _call("care_dropout", _p(ones), _p(out), n, p, seed)
    torch.cuda.synchronize()
    return out.cpu()


# (nseq, seq, nkeys, heads, causal, p_drop, with_dbias)
ATTN_REAL = [(3, 29, 29, 8, True, p, False) for p in (0.0, 0.1, 0.5)] + [(3, 29, 114, 8, False, p, True) for p in (0.0, 0.1, 0.5)] + \
            [(2, 28, 28, 8, False, p, False) for p in (0.0, 0.1, 0.5)]
# tile edges of the matrix-core forms: seq 1, 15, 16, 17, 32 x nkeys 1, 15, 16, 17, 64, 65, 127, 128, crossed sparingly (a fixed sample)
ATTN_EDGES = [
    (2, 1, 1, 8, False, 0.0, True), (2, 1, 15, 8, False, 0.0, False), (2, 1, 17, 8, False, 0.5, False), (2, 1, 64, 8, False, 0.1, True),
    (1, 1, 128, 8, False, 0.1, True), (2, 15, 15, 8, True, 0.1, False), (2, 15, 16, 8, False, 0.5, True), (2, 15, 64, 8, False, 0.5, True),
    (2, 15, 65, 8, False, 0.1, False), (2, 15, 127, 8, False, 0.0, False), (2, 15, 128, 8, False, 0.1, True), (2, 16, 1, 8, False, 0.1, True),
    (2, 16, 16, 8, True, 0.5, False), (2, 16, 17, 8, False, 0.5, False), (2, 16, 65, 8, False, 0.0, True), (2, 16, 127, 8, False, 0.1, False),
    (2, 16, 128, 8, False, 0.5, False), (2, 17, 1, 8, False, 0.0, True), (2, 17, 15, 8, False, 0.1, True), (2, 17, 17, 8, True, 0.0, False),
    (2, 17, 64, 8, False, 0.5, False), (2, 17, 65, 8, False, 0.1, False), (2, 17, 127, 8, False, 0.1, True), (3, 32, 1, 8, False, 0.5, False),
    (2, 32, 15, 8, False, 0.0, True), (2, 32, 16, 8, False, 0.5, True), (2, 32, 32, 8, True, 0.1, False), (2, 32, 65, 8, False, 0.1, False),
    (2, 32, 127, 8, False, 0.5, True), (2, 32, 128, 8, False, 0.0, True),
]
ATTN_HEADS = [(2, 29, 114, 4, False, 0.1, True), (2, 29, 29, 12, True, 0.5, False), (1, 20, 84, 16, False, 0.1, True)]
# seq > 32: the one-wave forms of both entry points; 128 keys: (384 + 2 x 128 x 64) x 4 = 67 KB of dynamic LDS
ATTN_ONE_WAVE = [(2, 33, 33, 8, True, 0.1, False), (2, 40, 128, 8, False, 0.5, True), (2, 33, 114, 8, False, 0.0, True),
                 (1, 40, 17, 4, False, 0.1, False)]
ATTN_MANY = [(512, 29, 114, 8, False, 0.1, True)]   # 4096 workgroups, 512 atomics per dbias entry


def _attn_inputs(nseq, seq, nkeys, heads, causal, p_drop):
    g = _gen(nseq, seq, nkeys, heads, causal, int(p_drop * 10))
    d = heads * 64
    q, k, v = (torch.randn(n, d, generator=g) for n in (nseq * seq, nseq * nkeys, nseq * nkeys))
    bias = torch.randn(heads, nkeys, generator=g)
    dctx = torch.randn(nseq * seq, d, generator=g)
    pad = torch.rand(nseq, nkeys, generator=g) < 0.25           # padded keys: exact zeros in P
    pad[:, 0] = False
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
    return q, k, v, bias, dctx, pad, seed


def _attn_reference(dt, q, k, v, bias, dctx, pad, mask, nseq, seq, nkeys, heads, causal):
    """softmax(S) -> * mask -> @ V per (sequence, head) in dtype `dt`, differentiated by autograd: (P [nseq * seq, heads, nkeys],
    ctx, dq, dk, dv, dbias, per-term dS [nseq, heads, seq, nkeys])."""
    q_, k_, v_, b_ = (_leaf(t, dt) for t in (q, k, v, bias))
    qh = q_.view(nseq, seq, heads, 64).permute(0, 2, 1, 3)
    kh = k_.view(nseq, nkeys, heads, 64).permute(0, 2, 1, 3)
    vh = v_.view(nseq, nkeys, heads, 64).permute(0, 2, 1, 3)
    m = pad.view(nseq, 1, 1, nkeys).expand(nseq, heads, seq, nkeys).clone()
    if causal:
        m |= torch.triu(torch.ones(seq, nkeys, dtype=torch.bool), 1).view(1, 1, seq, nkeys)
    S = (qh @ kh.transpose(-1, -2) / 8.0).masked_fill(m, -1e9) + b_.view(1, heads, 1, nkeys)
    S.retain_grad()
    P = torch.softmax(S, -1)
    mk = mask.view(nseq, seq, heads, nkeys).permute(0, 2, 1, 3).to(dt)
    ctx = ((P * mk) @ vh).permute(0, 2, 1, 3).reshape(nseq * seq, heads * 64)
    ctx.backward(dctx.to(dt))
    return (P.detach().permute(0, 2, 1, 3).reshape(nseq * seq, heads, nkeys), ctx.detach(), q_.grad, k_.grad, v_.grad, b_.grad,
            S.grad)


def _attn_case(worst, geo, padded, with_bwd=True):
    nseq, seq, nkeys, heads, causal, p_drop, with_dbias = geo
    d = heads * 64
    what = "attn {} padded {}".format(geo, padded)
    q, k, v, bias, dctx, pad, seed = _attn_inputs(nseq, seq, nkeys, heads, causal, p_drop)
    mask = _dropout_mask(nseq * seq * heads * nkeys, p_drop, seed)
    P64, ctx64, dq64, dk64, dv64, db64, dS64 = _attn_reference(torch.float64, q, k, v, bias, dctx, pad, mask, nseq, seq, nkeys, heads, causal)
    _, ctx32, dq32, dk32, dv32, db32, _ = _attn_reference(torch.float32, q, k, v, bias, dctx, pad, mask, nseq, seq, nkeys, heads, causal)
    if causal or bool(pad.any()):
        assert bool((P64 == 0).any()), what                    # masked keys: exact zeros in P, as training's probabilities have
    Pd = P64.float().contiguous().to(DEV)                      # the kernels are handed the fp32 rounding of the reference's P

    ldq, ldkv, ldd, ldc, lddq, lddkv = (d + 2, 2 * d + 4, d + 6, d + 7, d + 5, d + 3) if padded else (d, d, d, d, d, d)
    _, qd = _padded(q, ldq)
    if padded:   # K | V side by side in one buffer: one row stride for both, as the ABI has it
        kvb = _nan(nseq * nkeys + 1, ldkv)
        kd, vd = kvb[:nseq * nkeys, :d], kvb[:nseq * nkeys, d:2 * d]
        kd.copy_(k)
        vd.copy_(v)
    else:
        kd, vd = k.to(DEV), v.to(DEV)
    _, dcd = _padded(dctx, ldd)
    rows, krows = nseq * seq, nseq * nkeys
    bias_ld = nkeys + 5
    db0 = torch.randn(heads, bias_ld, generator=_gen(7, nkeys, heads)) * 2.0   # earlier contents of dbias

    def run():
        ctxb = _nan(rows + 1, ldc)
        _call("care_attn_pv", _p(Pd), _p(vd), nkeys * ldkv, ldkv, _p(ctxb), ldc, nseq, seq, nkeys, heads, p_drop, seed)
        if not with_bwd:
            torch.cuda.synchronize()
            return ctxb, None, None, None, None
        dqb, dkb, dvb = _nan(rows + 1, lddq), _nan(krows + 1, lddkv), _nan(krows + 1, lddkv)
        dbb = db0.to(DEV) if with_dbias else None
        _call("care_attn_bwd", _p(qd), ldq, _p(kd), _p(vd), nkeys * ldkv, ldkv, _p(Pd), _p(dcd), ldd, _p(dqb), lddq, _p(dkb), _p(dvb),
              nkeys * lddkv, lddkv, _p(dbb), bias_ld if with_dbias else 0, nseq, seq, nkeys, heads, p_drop, seed)
        torch.cuda.synchronize()
        return ctxb, dqb, dkb, dvb, dbb

    first, second = run(), run()
    ctxb, dqb, dkb, dvb, dbb = first
    _only_inside_written(ctxb, rows, d)
    _check(worst, what + " ctx", ctxb[:rows, :d], ctx64, ctx32)
    assert torch.equal(ctxb[:rows, :d], second[0][:rows, :d]), what + ": ctx differs between two runs"
    if not with_bwd:
        return
    for name, buf, n, r64, r32, again in (("dQ", dqb, rows, dq64, dq32, second[1]), ("dK", dkb, krows, dk64, dk32, second[2]),
                                          ("dV", dvb, krows, dv64, dv32, second[3])):
        _only_inside_written(buf, n, d)
        _check(worst, what + " " + name, buf[:n, :d], r64, r32)
        assert torch.equal(buf[:n, :d], again[:n, :d]), what + ": " + name + " differs between two runs"   # no atomics: bit-identical
    if with_dbias:
        # dbias is summed with atomics across sequences (and, one-wave form, across queries): two runs agree to tolerance only,
        # so each is held to the same bar and they are not compared bit for bit
        c0 = db0[:, :nkeys]
        bound = c0.double().abs() + dS64.abs().sum((0, 2))
        for got in (dbb, second[4]):
            assert torch.equal(got[:, nkeys:].cpu(), db0[:, nkeys:]), what + ": dbias written past nkeys"
            _check(worst, what + " dbias", got[:, :nkeys], c0.double() + db64, c0 + db32, bound)


@pytest.mark.parametrize("group", ["real", "edges", "heads", "one_wave", "many"])
def test_attn_pv_and_bwd_against_float64_autograd(group):
    """ctx = (P o mask) V and dQ, dK, dV, dbias of softmax(S) -> o mask -> . V against float64 autograd, the dropout mask taken
    from care_dropout (same generator, same flat index).  The three real geometries as training lays them out (dense), every
    other one with padded leading dimensions and NaN sentinels round every output."""
    geos = dict(real=ATTN_REAL, edges=ATTN_EDGES, heads=ATTN_HEADS, one_wave=ATTN_ONE_WAVE, many=ATTN_MANY)[group]
    worst = _Worst("care_attn_pv / care_attn_bwd [{}]".format(group))
    for geo in geos:
        _attn_case(worst, geo, padded=group not in ("real", "many"))
    worst.report()


def test_attn_pv_alone_above_128_keys():
    """130 keys: care_attn_pv's one-wave form (also at seq <= 32); care_attn_bwd has no form for it and must say so."""
    from care_amd import _lib

    worst = _Worst("care_attn_pv nkeys=130")
    for geo in ((2, 29, 130, 8, False, 0.1, False), (2, 33, 130, 8, False, 0.5, False), (1, 1, 130, 4, False, 0.0, False)):
        _attn_case(worst, geo, padded=True, with_bwd=False)
    worst.report()
    nseq, seq, nkeys, heads, d = 1, 4, 130, 1, 64
    z = lambda n: torch.zeros(n, d, device=DEV)
    q, k, v, dc, dq, dk, dv = z(seq), z(nkeys), z(nkeys), z(seq), z(seq), z(nkeys), z(nkeys)
    P = torch.zeros(seq, heads, nkeys, device=DEV)
    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        _call("care_attn_bwd", _p(q), d, _p(k), _p(v), nkeys * d, d, _p(P), _p(dc), d, _p(dq), d, _p(dk), _p(dv), nkeys * d, d, None, 0,
              nseq, seq, nkeys, heads, 0.0, 1)


# ================================================================================================= 3. care_attention_probs
# (nseq, seq, nkeys, heads, causal, with_bias, with_pad, kv dtype, rows_per_kv (0: seq), all_pad_sequence)
PROBS_SEQ_FORM = [   # fp32 keys, whole sequences of 8 .. 32 positions, rows_per_kv = seq: attention_probs_seq_kernel
    (3, 29, 29, 8, True, False, True, torch.float32, 0, False), (3, 29, 114, 8, False, True, False, torch.float32, 0, False),
    (2, 28, 28, 8, False, False, False, torch.float32, 0, False), (2, 8, 1, 8, False, True, True, torch.float32, 0, False),
    (2, 16, 16, 8, True, True, True, torch.float32, 0, False), (2, 17, 17, 4, True, False, False, torch.float32, 0, False),
    (2, 32, 128, 8, False, True, True, torch.float32, 0, False), (2, 15, 17, 12, False, True, True, torch.float32, 0, False),
    (3, 29, 114, 8, False, True, True, torch.float32, 0, True), (2, 32, 16, 16, False, False, True, torch.float32, 0, False),
]
PROBS_ROW_FORM = [   # everything else: attention_probs_kernel (a wave per (row, head))
    (3, 1, 114, 8, False, True, True, torch.float32, 0, False), (3, 1, 1, 8, True, False, False, torch.float32, 0, False),
    (2, 7, 7, 8, True, False, True, torch.float32, 0, False), (2, 7, 128, 8, False, True, True, torch.float32, 0, False),
    (2, 33, 33, 8, True, False, True, torch.float32, 0, False), (2, 33, 17, 4, False, True, False, torch.float32, 0, False),
    (3, 29, 29, 8, True, False, True, torch.bfloat16, 0, False), (3, 29, 114, 8, False, True, True, torch.bfloat16, 0, False),
    (2, 16, 16, 8, False, True, False, torch.bfloat16, 0, False), (6, 1, 16, 8, False, True, True, torch.float32, 1, False),
    (2, 5, 114, 8, False, True, True, torch.float32, 5, False), (2, 5, 17, 8, False, False, True, torch.bfloat16, 5, True),
    (3, 1, 128, 12, False, True, True, torch.bfloat16, 1, True),
]


def _probs_case(worst, case):
    nseq, seq, nkeys, heads, causal, with_bias, with_pad, kdt, per_kv, all_pad = case
    what = "attention_probs {}".format(case)
    g = _gen(nseq, seq, nkeys, heads, causal, with_bias, with_pad, per_kv)
    d = heads * 64
    rows = nseq * seq
    per_kv = per_kv or seq
    nkv = rows // per_kv
    assert rows % per_kv == 0
    q = torch.randn(rows, d, generator=g)
    k = torch.randn(nkv * nkeys, d, generator=g).to(kdt)
    bias_ld = nkeys + 3
    bias_buf = torch.randn(heads, bias_ld, generator=g)
    tok = torch.randint(1, 5, (nkv, nkeys + 2), generator=g).to(torch.int32)      # pad table with its own row stride
    tok[:, :nkeys][torch.rand(nkv, nkeys, generator=g) < 0.3] = 0
    tok[:, 0] = 2
    if all_pad:
        tok[nkv - 1, :] = 0                                       # a block whose keys are ALL padding
    pad = tok[:, :nkeys].eq(0) if with_pad else torch.zeros(nkv, nkeys, dtype=torch.bool)

    def ref(dt):
        qh = q.to(dt).view(nkv, per_kv, heads, 64).permute(0, 2, 1, 3)
        kh = k.to(dt).view(nkv, nkeys, heads, 64).permute(0, 2, 1, 3)   # (bf16 keys: the rounded operand, exactly representable)
        s = qh @ kh.transpose(-1, -2) / 8.0
        m = pad.view(nkv, 1, 1, nkeys).expand(nkv, heads, per_kv, nkeys).clone()
        if causal:
            m |= torch.triu(torch.ones(seq, nkeys, dtype=torch.bool), 1).view(1, 1, seq, nkeys)
        s = s.masked_fill(m, -1e9)
        if with_bias:
            s = s + bias_buf[:, :nkeys].to(dt).view(1, heads, 1, nkeys)
        return torch.softmax(s, -1).permute(0, 2, 1, 3).reshape(rows, heads, nkeys)

    p64, p32 = ref(torch.float64), ref(torch.float32)
    n = rows * heads * nkeys
    out = _nan(n + 64)
    qd, kd, bd, td = q.to(DEV), k.to(DEV), bias_buf.to(DEV), tok.to(DEV)
    _call("care_attention_probs", _p(qd), d, _p(kd), 1 if kdt == torch.bfloat16 else 0, nkeys * d, d, per_kv, nkeys, 1 if causal else 0,
          seq, _p(td) if with_pad else None, tok.stride(0) if with_pad else 0, 0, _p(bd) if with_bias else None,
          bias_ld if with_bias else 0, _p(out), rows, heads)
    torch.cuda.synchronize()
    assert torch.isnan(out[n:]).all(), what + ": written past the probabilities"
    got = out[:n].view(rows, heads, nkeys)
    _check(worst, what, got, p64, p32)
    assert float((got.double().sum(-1) - 1.0).abs().max()) < 1e-6, what
    if causal:
        past = torch.triu(torch.ones(seq, nkeys, dtype=torch.bool), 1).view(1, seq, 1, nkeys).expand(nseq, seq, heads, nkeys)
        assert not bool(got.view(nseq, seq, heads, nkeys).cpu()[past].ne(0).any()), what        # exact zeros past the causal bound


@pytest.mark.parametrize("form", ["seq", "row"])
def test_attention_probs_against_float64(form):
    """softmax((q_h . k_h) / 8 masked_fill(pad, -1e9) (+ causal) + bias) in float64 (tests/test_gpu_kernels.py test_attention's
    formula): nkeys 1 .. 128, a bias with bias_ld > nkeys, none, no pad table, a key block that is ALL padding (float64: the
    softmax of the bias alone; fp32 - torch's and the kernel's - rounds -1e9 + bias to -1e9: the yardstick carries that)."""
    worst = _Worst("care_attention_probs [{}]".format(form))
    for case in (PROBS_SEQ_FORM if form == "seq" else PROBS_ROW_FORM):
        _probs_case(worst, case)
    worst.report()


def test_attention_probs_rejects_129_keys():
    from care_amd import _lib

    q, k = torch.zeros(8, 64, device=DEV), torch.zeros(129, 64, device=DEV)
    out = torch.zeros(8 * 129, device=DEV)
    with pytest.raises(_lib.CareHipError):
        _call("care_attention_probs", _p(q), 64, _p(k), 0, 129 * 64, 64, 8, 129, 0, 8, None, 0, 0, None, 0, _p(out), 8, 1)


# ======================================================================================= 4. element-wise and index kernels
@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_forward_and_gradient(act):
    """care_act: out = act(z) and out = dy * act'(z) for none / ReLU / GELU; the inputs include 0, -0, +-1e-8, +-6, +-30 (the GELU
    gradient's tails against float64 erf)."""
    worst = _Worst("care_act act={}".format(act))
    special = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 6.0, -6.0, 30.0, -30.0, 1.0, -1.0, 0.5, -3.0])
    for n in (1, 255, 257, (1 << 20) + 3):
        g = _gen(n, act)
        z = torch.randn(n, generator=g) * 2.5
        m = min(n, special.numel())
        z[:m] = special[:m] if n > 1 else special[5:6]
        dy = torch.randn(n, generator=g)

        def ref(dt):
            z_ = _leaf(z, dt)
            y = z_ if act == 0 else (torch.relu(z_) if act == 1 else torch.nn.functional.gelu(z_))
            y = y * 1.0
            y.backward(dy.to(dt))
            return y.detach(), z_.grad

        (y64, dz64), (y32, dz32) = ref(torch.float64), ref(torch.float32)
        zd, dyd = z.to(DEV), dy.to(DEV)
        out = _nan(n + 5)
        _call("care_act", _p(zd), None, _p(out), n, act)
        torch.cuda.synchronize()
        assert torch.isnan(out[n:]).all()
        _check(worst, "act {} forward n {}".format(act, n), out[:n], y64, y32)
        out = _nan(n + 5)
        _call("care_act", _p(zd), _p(dyd), _p(out), n, act)
        torch.cuda.synchronize()
        assert torch.isnan(out[n:]).all()
        _check(worst, "act {} backward n {}".format(act, n), out[:n], dz64, dz32)
    worst.report()


def test_bcast_rows():
    """dst[i] = scale * src[i / grp]: groups that do not divide the row count, strides on both sides."""
    worst = _Worst("care_bcast_rows")
    for rows, d, grp, scale in ((29, 512, 29, 1.0 / 29), (100, 70, 7, 1.0 / 3), (1, 1, 5, 2.5), (58, 513, 28, 1.0 / 28), (1000, 64, 1, -1.0)):
        g = _gen(rows, d, grp)
        ngrp = (rows + grp - 1) // grp
        src = torch.randn(ngrp, d, generator=g)
        sc = float(np.float32(scale))                                # the scale travels as an fp32 argument
        idx = torch.arange(rows) // grp
        r64, r32 = sc * src.double()[idx], torch.tensor(sc, dtype=torch.float32) * src[idx]
        _, sd = _padded(src, d + 3)
        dst = _nan(rows + 1, d + 6)
        _call("care_bcast_rows", _p(sd), d + 3, _p(dst), d + 6, rows, d, grp, scale)
        torch.cuda.synchronize()
        _only_inside_written(dst, rows, d)
        _check(worst, "bcast_rows {}".format((rows, d, grp)), dst[:rows, :d], r64, r32)
    worst.report()


def test_add_pos_sem():
    """out[r] = x[r] + pos[r % seq] + sem[r / sem_div]: each of pos / sem absent in turn, sem_div != seq."""
    worst = _Worst("care_add_pos_sem")
    for rows, d, seq, sem_div, has_pos, has_sem in ((87, 512, 29, 29, True, True), (87, 512, 29, 29, True, False), (90, 100, 30, 30, False, True),
                                                    (60, 65, 12, 20, True, True), (60, 65, 12, 5, False, True), (7, 1, 7, 1, True, True),
                                                    (33, 513, 33, 11, False, False)):
        g = _gen(rows, d, seq, sem_div)
        x, pos = torch.randn(rows, d, generator=g), torch.randn(seq, d, generator=g)
        sem = torch.randn((rows + sem_div - 1) // sem_div, d, generator=g)
        r = torch.arange(rows)

        def ref(dt):
            o = x.to(dt)
            if has_pos:
                o = o + pos.to(dt)[r % seq]
            if has_sem:
                o = o + sem.to(dt)[r // sem_div]
            return o

        out = _nan(rows * d + 9)
        xd, pd, sd = x.to(DEV), pos.to(DEV), sem.to(DEV)
        _call("care_add_pos_sem", _p(xd), _p(pd) if has_pos else None, _p(sd) if has_sem else None, _p(out), rows, d, seq, sem_div)
        torch.cuda.synchronize()
        assert torch.isnan(out[rows * d:]).all()
        _check(worst, "add_pos_sem {}".format((rows, d, seq, sem_div, has_pos, has_sem)), out[:rows * d].view(rows, d), ref(torch.float64),
               ref(torch.float32))
    worst.report()


def test_scatter_add_rows():
    """table[idx[i]] += src[i] against float64 index_add_: every row onto ONE index, random indices with repeats, skip_idx and
    negative indices left out, ldt > d, a table with earlier contents (the bound per element: |contents| + sum of |terms|)."""
    worst = _Worst("care_scatter_add_rows")
    for rows, d, ntab, mode, skip in ((5000, 64, 3, "one", -1), (300, 512, 50, "random", 0), (1856, 100, 2000, "random", 7),
                                      (64, 513, 5, "negative", 2), (1, 1, 1, "one", -1), (257, 65, 4, "all_skipped", 1)):
        g = _gen(rows, d, ntab)
        src = torch.randn(rows, d, generator=g)
        if mode == "one":
            idx = torch.full((rows,), ntab - 1, dtype=torch.int32)
        elif mode == "all_skipped":
            idx = torch.full((rows,), skip, dtype=torch.int32)
        else:
            idx = torch.randint(0, ntab, (rows,), generator=g).to(torch.int32)
            if mode == "negative":
                idx[::3] = -1
                idx[1::7] = -5
        t0 = torch.randn(ntab, d, generator=g) * 2.0
        use = (idx >= 0) & (idx != skip)
        ui = idx[use].long()

        def ref(dt):
            return t0.to(dt).index_add_(0, ui, src.to(dt)[use])

        bound = t0.double().abs().index_add_(0, ui, src.double().abs()[use])
        _, sd = _padded(src, d + 2)
        tb, tv = _padded(t0, d + 4, extra_rows=2)
        idd = idx.to(DEV)
        _call("care_scatter_add_rows", _p(sd), d + 2, _p(idd), _p(tv), d + 4, rows, d, skip)
        torch.cuda.synchronize()
        _only_inside_written(tb, ntab, d)
        _check(worst, "scatter_add_rows {}".format((rows, d, ntab, mode, skip)), tv, ref(torch.float64), ref(torch.float32), bound)
        if mode == "all_skipped":
            assert torch.equal(tv.cpu(), t0)
    worst.report()


def test_concept_bwd():
    """ds = (dpreds [1 - p >= 1e-12] + davg / k) p (1 - p) against float64 autograd of preds = 1 - exp(log(clamp(1 - p, 1e-12, 1))),
    avg = mean_k p; scores in [-90, 90]: both sides of the gate and both saturated ends.  Compared in ABSOLUTE terms (the
    floor is 2^-22 of the largest gradient): near saturation fp32's 1 - p is quantised, float64's is not."""
    worst = _Worst("care_concept_bwd")
    for B, k, has_dp, has_da in ((5, 500, True, True), (5, 500, True, False), (5, 500, False, True), (1, 1, True, True), (33, 65, True, True)):
        g = _gen(B, k, has_dp, has_da)
        scores = (torch.rand(B, k, generator=g) * 2 - 1) * 90.0
        scores[0, :min(k, 12)] = torch.tensor([0.0, 27.0, 27.6, 27.7, 28.0, 16.0, 17.0, 18.0, -88.0, 89.0, -30.0, 1e-3])[:min(k, 12)]
        if B > 1:
            scores[1] = torch.randn(k, generator=g) * 3.0
        dp, da = torch.randn(B, k, generator=g), torch.randn(B, generator=g) * 3.0

        def ref(dt):
            s = _leaf(scores, dt)
            p = torch.sigmoid(s)
            preds = 1.0 - torch.exp(torch.log(torch.clamp(1.0 - p, 1e-12, 1)))
            avg = p.mean(1)
            loss = s.sum() * 0.0
            if has_dp:
                loss = loss + (preds * dp.to(dt)).sum()
            if has_da:
                loss = loss + (avg * da.to(dt)).sum()
            loss.backward()
            return s.grad

        r64, r32 = ref(torch.float64), ref(torch.float32)
        open_, shut = (1.0 - torch.sigmoid(scores.double())) >= 1e-12, (1.0 - torch.sigmoid(scores.double())) < 1e-12
        assert bool(open_.any()) and (bool(shut.any()) or k == 1)        # both sides of the gate occur
        _, sd = _padded(scores, k + 3)
        _, dpd = _padded(dp, k + 1)
        dad = da.to(DEV)
        out = _nan(B + 1, k + 5)
        _call("care_concept_bwd", _p(sd), k + 3, _p(dpd) if has_dp else None, k + 1, _p(dad) if has_da else None, _p(out), k + 5, B, k)
        torch.cuda.synchronize()
        _only_inside_written(out, B, k)
        _check(worst, "concept_bwd {}".format((B, k, has_dp, has_da)), out[:B, :k], r64, r32)
    worst.report()


# ============================================================================================ 5. care_dropout and the seeds
def _mask(n, p, seed):
    x = torch.ones(n, device=DEV)
    y = torch.empty_like(x)
    _call("care_dropout", _p(x), _p(y), n, p, seed)
    torch.cuda.synchronize()
    return y


def test_dropout_kernel_contract():
    """Same seed: the same bits; p = 0: the identity; p = 1 and p < 0: rejected; the keep rate within 5 sigma of 1 - p
    (sigma = sqrt(p (1 - p) / n), n = 2^20 - derived, not tuned); survivors scaled by 1 / (1 - p); _Dropout's backward zeroes exactly
    the forward's positions."""
    from care_amd import _lib, training

    n = 1 << 20
    g = _gen(5)
    x = torch.randn(n, generator=g).to(DEV)
    x[x == 0] = 1.0
    for p in (0.1, 0.5):
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        a, b = torch.empty_like(x), torch.empty_like(x)
        _call("care_dropout", _p(x), _p(a), n, p, seed)
        _call("care_dropout", _p(x), _p(b), n, p, seed)
        c = torch.empty_like(x)
        _call("care_dropout", _p(x), _p(c), n, p, seed + 1)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and not torch.equal(a, c)
        keep = a != 0
        rate, sigma = float(keep.double().mean()), math.sqrt(p * (1 - p) / n)
        print("care_dropout p {}: keep rate {:.6f}, |rate - (1 - p)| = {:.2f} sigma".format(p, rate, abs(rate - (1 - p)) / sigma))
        assert abs(rate - (1 - p)) <= 5 * sigma, (p, rate)
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert torch.equal(a[keep], (x * float(scale))[keep])
        # the autograd Function: the gradient is zero exactly where the forward was, 1 / (1 - p) elsewhere
        xin = x.clone().requires_grad_(True)
        y = training._Dropout.apply(xin, p, seed)
        assert torch.equal(y.detach(), a)
        y.sum().backward()
        assert torch.equal(xin.grad != 0, keep) and torch.equal(xin.grad[keep], torch.full_like(xin.grad[keep], float(scale)))
    out = torch.empty_like(x)
    _call("care_dropout", _p(x), _p(out), n, 0.0, 99)
    torch.cuda.synchronize()
    assert torch.equal(out, x)
    for p in (1.0, -0.1):
        with pytest.raises(_lib.CareHipError):
            _call("care_dropout", _p(x), _p(out), n, p, 99)


def site_mask_shares(seeds, n=1 << 18, p=0.5):
    """For every pair of sites a before b and every shift s in 0 .. 3: the share of positions where mask_a[s:] == mask_b[:n - s]."""
    masks = [_mask(n, p, s) != 0 for s in seeds]
    shares = {}
    for a in range(len(seeds)):
        for b in range(a + 1, len(seeds)):
            for s in range(4):
                shares[(a, b, s)] = float((masks[a][s:] == masks[b][:n - s]).double().mean())
    return shares


def test_dropout_masks_of_different_sites_are_independent():
    """16 consecutive seeds of one training._Seeds(), masks of 2^18 elements at p = 0.5: for every pair of sites and every shift
    0 .. 3 the share of agreeing positions lies within 5 sigma of 0.5 (sigma = 0.5 / sqrt(n - s), about 1e-3; 480 comparisons:
    a false alarm has probability below 1e-3).  With seeds stepped by the generator's own increment (base + G n) the masks of
    neighbouring sites were shifted copies of one another: shares of exactly 1.0."""
    from care_amd import training

    torch.manual_seed(20)
    seeds = training._Seeds()
    got = [seeds.next() for _ in range(16)]
    assert len(set(got)) == 16 and all(0 <= s < 2 ** 64 for s in got)
    n = 1 << 18
    shares = site_mask_shares(got, n)
    assert len(shares) == 480
    worst = max(shares.items(), key=lambda kv: abs(kv[1] - 0.5))
    print("dropout sites: worst share {} at (site a, site b, shift) {}; 5 sigma = {:.5f}".format(worst[1], worst[0], 2.5 / math.sqrt(n - 3)))
    for (a, b, s), share in shares.items():
        assert abs(share - 0.5) <= 5 * 0.5 / math.sqrt(n - s), (a, b, s, share)


# ================================================================================================== 6. care_split_pieces
def _scale_exp(bits):
    E = (bits >> 23) & 255
    return 0 if E in (0, 255) else min(max(141 - E, -100), 100)


def _split(src, rows, K, transposed, slabs, ks, pieces, slot, ld=None):
    """care_split_pieces into a buffer with a sentinel tail -> [slabs, rows, pieces * ks] fp16."""
    n = slabs * rows * pieces * ks
    out = torch.full((n + 64,), 7.0, device=DEV, dtype=torch.float16)
    _call("care_split_pieces", _p(src), ld if ld is not None else src.stride(0), rows, K, transposed, slabs, ks, _p(out), pieces, slot.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[n:] == 7.0).all()), "written past the pieces"
    return out[:n].view(slabs, rows, pieces * ks)


@pytest.mark.parametrize("rows,K,mag", [(70, 100, 1.0), (129, 1000, 1e-6), (64, 64, 3e4), (1, 1, 1e-20), (300, 517, 1e3)])
def test_split_pieces_contract(rows, K, mag):
    """include/care_hip.h: with e from care_absmax's slot, (hi + lo) 2^-e == src to 2^-21 of the tensor's |max| (two fp16 pieces
    hold 22 bits of the largest element), the largest scaled magnitude in [2^14, 2^15), pieces 2 (hi | lo) and 3 (hi | lo | hi),
    the transposed layout gives the same bits, slabs of ks columns with zeros past K.  (The kernel clamps e to +-100: a tensor
    whose |max| lies below 2^-86 or above 2^115 is outside this contract and outside this test.)"""
    from care_amd import training

    g = _gen(rows, K)
    src = (torch.randn(rows, K, generator=g) * mag)
    src[rows // 2, K // 3] *= 1e-4                                   # an element whose low piece is an fp16 denormal
    buf, sd = _padded(src, K + 3)
    st = src.t().contiguous().to(DEV)                                # the same operand as it lies transposed: [K, rows]
    slot = training._absmax_slot(src.to(DEV))
    bits = int(slot.item())
    amax = float(src.abs().max())
    assert float(slot.view(torch.float32).item()) == amax
    e = _scale_exp(bits)
    assert abs(e) < 100 and 2.0 ** 14 <= amax * 2.0 ** e < 2.0 ** 15
    for slabs in (1, 3, 32):
        ks = ((K + slabs - 1) // slabs + 63) // 64 * 64
        p2 = _split(sd, rows, K, 0, slabs, ks, 2, slot, ld=K + 3)
        p3 = _split(sd, rows, K, 0, slabs, ks, 3, slot, ld=K + 3)
        assert torch.equal(p3[:, :, :2 * ks], p2) and torch.equal(p3[:, :, 2 * ks:], p2[:, :, :ks])     # hi | lo | hi
        assert torch.equal(_split(st, rows, K, 1, slabs, ks, 2, slot), p2)                               # transposed: the same bits
        assert torch.equal(_split(st, rows, K, 1, slabs, ks, 3, slot), p3)
        assert torch.isfinite(p2.float()).all()
        hi = p2[:, :, :ks].permute(1, 0, 2).reshape(rows, slabs * ks).double().cpu()                    # column s ks + kk of the operand
        lo = p2[:, :, ks:].permute(1, 0, 2).reshape(rows, slabs * ks).double().cpu()
        assert float(hi[:, K:].abs().max() if slabs * ks > K else 0.0) == 0.0 and float(lo[:, K:].abs().max() if slabs * ks > K else 0.0) == 0.0
        back = (hi[:, :K] + lo[:, :K]) * 2.0 ** -e
        err = float((back - src.double()).abs().max())
        print("care_split_pieces {} slabs {}: |(hi + lo) 2^-e - src| / |max| = 2^{:.1f}".format((rows, K, mag), slabs, math.log2(max(err / amax, 1e-300))))
        assert err <= 2.0 ** -21 * amax, (slabs, err / amax)
        assert 2.0 ** 14 <= float((hi + lo).abs().max()) < 2.0 ** 15


def test_split_pieces_degenerate_maxima_and_rejections():
    """All-zero and infinite maxima: e = 0 (finite pieces for the zero tensor, the plain fp16 split for the finite elements of the
    other); ks % 64 != 0 is refused."""
    from care_amd import _lib, training

    rows, K, ks = 5, 70, 128
    zero = torch.zeros(rows, K, device=DEV)
    slot = training._absmax_slot(zero)
    assert int(slot.item()) == 0 and _scale_exp(0) == 0
    pz = _split(zero, rows, K, 0, 1, ks, 3, slot)
    assert torch.isfinite(pz.float()).all() and float(pz.float().abs().max()) == 0.0
    x = torch.randn(rows, K, generator=_gen(6))
    x[2, 3] = float("inf")
    xd = x.to(DEV)
    slot = training._absmax_slot(xd)
    assert int(slot.item()) == 0x7F800000 and _scale_exp(0x7F800000) == 0
    pi = _split(xd, rows, K, 0, 1, ks, 2, slot)
    fin = torch.isfinite(x)
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    assert torch.equal(pi[0, :, :K].cpu()[fin], hi[fin]) and torch.equal(pi[0, :, ks:ks + K].cpu()[fin], lo[fin])   # e = 0
    out = torch.zeros(rows * 3 * 96, device=DEV, dtype=torch.float16)
    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        _call("care_split_pieces", _p(xd), K, rows, K, 0, 1, 96, _p(out), 3, slot.data_ptr())


# ============================================================ 7. one training step where "auto" mixes both GEMM forms
def test_training_step_where_auto_mixes_split_and_exact_products():
    """msrvtt_care at 64 clips under the default TRAIN_GEMM = "auto": the vocabulary products (2 M N K = 20 GFLOP) take the split
    form, the d x d ones (1 GFLOP) the exact form - the mix bench.py's training legs time, which 2 - 4 clips never reach.
    Forward and every parameter's gradient against the oracle's autograd, tests/test_gpu_training.py's bars unchanged."""
    from care_amd import get_framework, training
    from care_amd.configs import feat_shapes, make_opt
    from care_amd.synth import synth_feats, synth_input_ids, synth_state_dict
    from test_gpu_training import NO_DROP, _compare_with_oracle_autograd

    clips = 64
    opt = make_opt("msrvtt_care", **{**NO_DROP, "hidden_act": "gelu"})
    d, t, V = int(opt["dim_hidden"]), int(opt["max_len"]) - 1, int(opt["vocab_size"])
    training.set_train_gemm("auto")
    assert training.TRAIN_GEMM == "auto"
    assert training._use_x3(clips * t, V, d), "the vocabulary product does not take the split form: the test does not test"
    assert not training._use_x3(clips * t, d, d), "a d x d product takes the split form: the test does not test"
    model = get_framework(opt)
    P = synth_state_dict(7, [(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(P, strict=True)
    feats = synth_feats(7, feat_shapes(opt, clips))
    ids = synth_input_ids(7, clips, opt["max_len"] - 1, opt["vocab_size"])
    _compare_with_oracle_autograd(opt, P, feats, ids, model.to("cuda:0"))

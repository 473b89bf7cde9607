"""GPU: the kernels that use the library's 16-bit type, in BOTH libraries side by side on the same inputs.

csrc/ compiles twice from one source: libcare_hip.so (variant "", 16-bit type bfloat16) and libcare_hip_f16.so (variant
"f16", IEEE half - the default 16-bit mode).  tests/test_gpu_kernels.py runs on the first; every test here is parametrised
over both and calls through `_lib.call(..., variant=variant)`.

The reference is always float64 arithmetic on operands rounded to the variant's 16-bit type (what the MFMA sees).  Bars:
  * fp32 outputs: BAR32 = 3e-3 absolute on O(1..30) outputs - the order of the fp32 sums, the same in both libraries;
  * 16-bit outputs: elementwise half an ulp of the 16-bit type at the reference + BAR32.  For 2^e <= |ref| < 2^(e+1) and
    p significand bits (implicit one included: 8 bf16, 11 half) the spacing is 2^(e+1-p) and half an ulp is H = 2^(e-p),
    the largest error of a correct round-to-nearest.  How H relates to a bound proportional to |ref|:
      - 2^-(p+1) |ref| lies in [H / 2, H): BELOW half an ulp in the whole binade (by 2 x at its bottom), so a correctly
        rounding kernel cannot meet it; asserting H is up to 2 x wider than that form - deliberately;
      - 2^-p |ref| lies in [H, 2 H): equal to H at the bottom of the binade, up to 2 x wider at its top; H is never
        wider than that form.
    H is the tightest bound a correct conversion always meets, so H (`_half_ulp`) + BAR32 is what `_assert_h16` asserts.
  * kernels that round intermediates to 16 bits (the absorbed cross-attention, attention_seq, the head projections): bf16
    keeps the bar of the matching test in test_gpu_kernels.py, which half may never exceed either; half's own bar is
    2 x the worst error measured against the float64 reference (the figure stands next to each constant).

Second half of the file: what half's format changes for a kernel - the exponent range in the lazy softmax of the
absorbed cross-attention, the conversion (round to nearest even, subnormals, overflow) and subnormal MFMA operands.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VARIANTS = ["", "f16"]
BAR32 = 3e-3


def _h16(variant):
    return torch.float16 if variant else torch.bfloat16


def _caller(variant):
    from care_amd import _lib

    return lambda name, *a: _lib.call(name, *a, variant=variant)


def _lib_of(variant):
    from care_amd import _lib

    return _lib.load(variant=variant)


def _p(t):
    return None if t is None else t.data_ptr()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _half_ulp(ref, h16):
    """Half the spacing of h16 at every element of `ref` (float64); 0 where ref is 0."""
    p, emin = (8, -126) if h16 == torch.bfloat16 else (11, -14)
    e = (torch.frexp(ref)[1] - 1).clamp_min(emin).double()      # ref = m 2^(e + 1), m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.exp2(e - p))


def _assert_f32(got, ref, what="", bar=BAR32):
    err = (got.double() - ref).abs().max().item()
    print("%s: max error %.3g / %.3g" % (what, err, bar))
    assert err < bar, (what, err)


def _assert_h16(got, ref, h16, what="", bar32=BAR32):
    """|got - ref| <= half an ulp of h16 at ref + the fp32 accumulation bar, elementwise."""
    assert got.dtype == h16
    err = (got.double() - ref).abs()
    over = (err - _half_ulp(ref, h16) - bar32).max().item()
    print("%s: max error %.3g, worst excess over half-ulp + %.3g: %.3g" % (what, err.max().item(), bar32, over))
    assert torch.isfinite(got.float()).all() and over <= 0, (what, over)


def _act(ref, act):
    return torch.relu(ref) if act == 1 else (torch.nn.functional.gelu(ref) if act == 2 else ref)


# ------------------------------------------------------------------------------------------------ GEMM families
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("a16", [False, True])
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 512, 512), (129, 1040, 256), (257, 2048, 512)])
def test_gemm_a_stationary(M, N, K, out16, a16, variant):
    """care_gemm_bf16 (csrc/gemm_as.hip): A fp32 (rounded in the kernel) or 16-bit, C fp32 or 16-bit, one row, ragged
    row and column tiles; nothing written outside the destination."""
    h16, call = _h16(variant), _caller(variant)
    A = _rand(M, K, seed=1)
    W = _rand(N, K, seed=2, scale=1 / math.sqrt(K)).to(h16).contiguous()
    bias = _rand(N, seed=3)
    Ain = A.to(h16).contiguous() if a16 else A
    act = 1 if M == 129 else 0
    out = torch.full((M + 2, N + 8), 7.0, device=DEV, dtype=h16 if out16 else torch.float32)
    dst = out[:M, :N]
    call("care_gemm_bf16", _p(Ain), K, int(a16), _p(W), _p(bias), _p(dst), dst.stride(0), int(out16), None, 0, 0, N, M, N, K, act)
    ref = _act(A.to(h16).double() @ W.double().t() + bias.double(), act)
    torch.cuda.synchronize()
    (_assert_h16(dst, ref, h16, "gemm_as") if out16 else _assert_f32(dst, ref, "gemm_as"))
    assert float(out[M:].float().min()) == 7.0 and float(out[:, N:].float().min()) == 7.0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel", ["care_gemm_bf16", "care_gemm_tile"])
def test_gemm_split_destination(kernel, variant):
    """q fp32 | K, V 16-bit straight into position 7 of a [M, 29, 1024] cache (columns >= n_split, own leading dimension)."""
    h16, call = _h16(variant), _caller(variant)
    M, K, d = 77, 512, 512
    A = _rand(M, K, seed=4).to(h16).contiguous()
    W, bias = _rand(3 * d, K, seed=5, scale=0.05).to(h16).contiguous(), _rand(3 * d, seed=6)
    q = torch.zeros(M, d, device=DEV)
    cache = torch.zeros(M, 29, 2 * d, device=DEV, dtype=h16)
    dst = cache[:, 7, :]
    tail = (_p(W), _p(bias), _p(q), d, 0, _p(dst), dst.stride(0), 1, d, M, 3 * d, K, 0)
    if kernel == "care_gemm_bf16":
        call(kernel, _p(A), K, 1, *tail)
    else:
        call(kernel, _p(A), K, *tail)
    ref = A.double() @ W.double().t() + bias.double()
    torch.cuda.synchronize()
    _assert_f32(q, ref[:, :d], kernel + " q")
    _assert_h16(cache[:, 7, :], ref[:, d:], h16, kernel + " k|v")
    assert cache[:, 6, :].float().abs().max().item() == 0 and cache[:, 8, :].float().abs().max().item() == 0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M", [5, 300])
def test_gemm_splitk_slabs(M, variant):
    """care_gemm_bf16_splitk: K = 2048 as four slabs of 512, summed (with residual and LayerNorm) by care_add_ln."""
    h16, call = _h16(variant), _caller(variant)
    N, K = 512, 2048
    A = _rand(M, K, seed=30).to(h16)
    W = _rand(N, K, seed=31, scale=0.03).to(h16).contiguous()
    bias, res = _rand(N, seed=32), _rand(M, N, seed=33)
    g, b = _rand(N, seed=34), _rand(N, seed=35)
    slabs = torch.full((K // 512, M, N), float("nan"), device=DEV)
    call("care_gemm_bf16_splitk", _p(A), K, 1, _p(W), _p(bias), _p(slabs), N, slabs.stride(0), M, N, K)
    out = torch.zeros(M, N, device=DEV)
    call("care_add_ln", _p(slabs), N, _p(res), N, None, _p(g), _p(b), 1e-12, _p(out), None, N, M, N, M, M, 0, K // 512, slabs.stride(0))
    y = A.double() @ W.double().t() + bias.double()
    ref = torch.nn.functional.layer_norm(y + res.double(), (N,), g.double(), b.double(), 1e-12)
    torch.cuda.synchronize()
    _assert_f32(slabs.double().sum(0), y, "splitk slabs")
    _assert_f32(out, ref, "splitk + add_ln")


def _tied_vocab(M, N, K, h16, seeds, a_row):
    """A [M, K], W [N, K] in h16 with exact ties (duplicated W rows: far apart, and inside the ragged last tile) that ARE the
    maximum of rows `a_row` and M - 1."""
    A = _rand(M, K, seed=seeds[0]).to(h16).contiguous()
    W = _rand(N, K, seed=seeds[1], scale=0.05)
    W[N // 2 + 5] = W[11]
    W[N - 1] = W[N - 2]
    A[a_row] = (W[11] * 40).to(h16)
    A[M - 1] = (W[N - 2] * 40).to(h16)
    return A, W.to(h16).contiguous()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M", [3, 129])
def test_gemm_argmax_with_labels(M, variant):
    """care_gemm_argmax_bf16 (arg-max and sum-exp epilogue of gemm_as.hip) with the label logit, reduced by
    care_score_partials: prediction, log-probability of the label; exact ties go to the lowest column."""
    h16, call, lib = _h16(variant), _caller(variant), _lib_of(variant)
    N, K = 10547, 512
    A, W = _tied_vocab(M, N, K, h16, (40, 41), 1)
    labels = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(M), dtype=torch.int32).to(DEV)
    labels[0] = N - 1
    parts = lib.care_argmax_parts_bf16(M, N)
    pm, ps, pl = (torch.full((M, parts), float("nan"), device=DEV) for _ in range(3))
    pi = torch.full((M, parts), -7, device=DEV, dtype=torch.int32)
    call("care_gemm_argmax_bf16", _p(A), K, 1, _p(W), _p(pm), _p(pi), _p(ps), _p(labels), _p(pl), M, N, K)
    logp, pred = torch.empty(M, device=DEV), torch.empty(M, device=DEV, dtype=torch.int32)
    call("care_score_partials", _p(pm), _p(pi), _p(ps), _p(pl), parts, _p(logp), _p(pred), M)
    ref = A.double() @ W.double().t()
    want = torch.log_softmax(ref, dim=1).gather(1, labels.long().unsqueeze(1)).squeeze(1)
    torch.cuda.synchronize()
    top2 = ref.topk(2, dim=1)
    safe = (top2[0][:, 0] - top2[0][:, 1]) > 1e-3
    assert torch.equal(pred[safe].long(), top2[1][:, 0][safe])
    assert int(pred[1]) == 11 and int(pred[M - 1]) == N - 2          # ties: the lower column
    _assert_f32(logp, want, "label log-probability")
    _assert_f32(pm.max(1).values, ref.max(1).values, "row maximum")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("out16", [False, True])
def test_gemm_store_256_row_panels(out16, variant):
    """csrc/gemm_store32.hip (16-bit A, K = 512, M >= 8192): a ragged last panel, nothing written outside."""
    h16, call = _h16(variant), _caller(variant)
    M, N, K = 8192 + 100, 512, 512
    A = _rand(M, K, seed=61).to(h16).contiguous()
    W = _rand(N, K, seed=62, scale=0.05).to(h16).contiguous()
    bias = _rand(N, seed=63)
    out = torch.full((M + 3, N + 8), 7.0, device=DEV, dtype=h16 if out16 else torch.float32)
    dst = out[:M, :N]
    call("care_gemm_bf16", _p(A), K, 1, _p(W), _p(bias), _p(dst), dst.stride(0), int(out16), None, 0, 0, N, M, N, K, 0)
    ref = A.double() @ W.double().t() + bias.double()
    torch.cuda.synchronize()
    (_assert_h16(dst, ref, h16, "store panels") if out16 else _assert_f32(dst, ref, "store panels"))
    assert float(out[M:].float().min()) == 7.0 and float(out[:, N:].float().min()) == 7.0


_vocab_ref = {}


def _vocab_case(variant):
    """Operands and float64 logits of the vocabulary panel case, made once per library."""
    if variant not in _vocab_ref:
        M, N, K = 8192 + 77, 10547, 512
        A, W = _tied_vocab(M, N, K, _h16(variant), (17, 18), 5)
        ref = A.double() @ W.double().t()
        top2 = ref.topk(2, dim=1)
        _vocab_ref[variant] = (A, W, torch.logsumexp(ref, 1), ref.max(1).values, top2[1][:, 0],
                               (top2[0][:, 0] - top2[0][:, 1]) > 1e-3)
        del ref
    return _vocab_ref[variant]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("min_parts", [1, 8])
def test_vocab_argmax_256_row_panels(min_parts, variant):
    """csrc/gemm_vocab.hip (16-bit A, K = 512, M >= 8192): per column range (max, lowest arg-max, sum-exp), merged like
    care_greedy_update merges them; ragged last panel and last tile; ties to the lower column."""
    call, lib = _caller(variant), _lib_of(variant)
    M, N, K = 8192 + 77, 10547, 512
    A, W, lse_ref, max_ref, arg_ref, safe = _vocab_case(variant)
    parts = lib.care_argmax_parts_bf16_min(M, N, K, 1, min_parts) if min_parts > 1 else lib.care_argmax_parts_bf16(M, N)
    assert parts >= min_parts
    pm, ps = torch.full((M, parts), float("nan"), device=DEV), torch.full((M, parts), float("nan"), device=DEV)
    pi = torch.full((M, parts), -7, device=DEV, dtype=torch.int32)
    if min_parts > 1:
        call("care_gemm_argmax_bf16_min", _p(A), K, 1, _p(W), _p(pm), _p(pi), _p(ps), M, N, K, min_parts)
    else:
        call("care_gemm_argmax_bf16", _p(A), K, 1, _p(W), _p(pm), _p(pi), _p(ps), None, None, M, N, K)
    torch.cuda.synchronize()
    best = pm.max(1).values
    lse = torch.log((ps.double() * torch.exp(pm.double() - best.double().unsqueeze(1))).sum(1)) + best.double()
    cand = torch.where(pm == best.unsqueeze(1), pi, torch.full_like(pi, 0x7fffffff)).min(1).values
    _assert_f32(lse, lse_ref, "log-sum-exp")
    _assert_f32(best, max_ref, "row maximum")
    assert torch.equal(cand[safe].long(), arg_ref[safe])
    assert int(cand[5]) == 11 and int(cand[M - 1]) == N - 2


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_generic_16bit_weight(variant):
    """care_gemm with wdtype = 1 (fp32 A rounded in the kernel, 16-bit W), K = 640: not a multiple of 128."""
    h16, call = _h16(variant), _caller(variant)
    M, N, K = 130, 640, 640
    A, W, bias = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=1 / math.sqrt(K)).to(h16).contiguous(), _rand(N, seed=3)
    out = torch.full((M, N), float("nan"), device=DEV)
    call("care_gemm", _p(A), K, _p(W), 1, _p(bias), _p(out), N, 0, None, 0, 0, N, M, N, K, 0)
    ref = A.to(h16).double() @ W.double().t() + bias.double()
    torch.cuda.synchronize()
    _assert_f32(out, ref, "generic gemm")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cfg", ["", "2422"])
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("M,N,K", [(129, 1024, 1024), (300, 768, 512), (4096 + 7, 1024, 1024)])
def test_gemm_tile(M, N, K, out16, cfg, variant, monkeypatch):
    """csrc/gemm_tile.hip (MFMA 32x32x16), default tile shape and one other; ragged edges in M and N."""
    h16, call = _h16(variant), _caller(variant)
    if cfg:
        monkeypatch.setenv("CARE_TILE_CFG", cfg)
    A = _rand(M, K, seed=71).to(h16).contiguous()
    W = _rand(N, K, seed=72, scale=1 / math.sqrt(K)).to(h16).contiguous()
    bias = _rand(N, seed=73)
    act = 1 if out16 else 0
    ld = (N + 15) // 8 * 8
    out = torch.full((M + 2, ld), 7.0, device=DEV, dtype=h16 if out16 else torch.float32)
    dst = out[:M, :N]
    call("care_gemm_tile", _p(A), K, _p(W), _p(bias), _p(dst), dst.stride(0), int(out16), None, 0, 0, N, M, N, K, act)
    ref = _act(A.double() @ W.double().t() + bias.double(), act)
    torch.cuda.synchronize()
    (_assert_h16(dst, ref, h16, "gemm_tile") if out16 else _assert_f32(dst, ref, "gemm_tile"))
    assert float(out[M:].float().min()) == 7.0 and float(out[:, N:].float().min()) == 7.0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cfg", ["", "2422"])
@pytest.mark.parametrize("M,K", [(129, 1024), (300, 512)])
def test_gemm_tile_argmax(M, K, cfg, variant, monkeypatch):
    """care_gemm_tile_argmax: per 64-column group (max, lowest arg-max, sum-exp) and the label logit."""
    h16, call, lib = _h16(variant), _caller(variant), _lib_of(variant)
    if cfg:
        monkeypatch.setenv("CARE_TILE_CFG", cfg)
    N = 10547
    A, W = _tied_vocab(M, N, K, h16, (81, 82), 0)
    parts = lib.care_argmax_parts_tile(N)
    labels = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(M), dtype=torch.int32).to(DEV)
    pm, ps, pl = (torch.full((M, parts), float("nan"), device=DEV) for _ in range(3))
    pi = torch.full((M, parts), -7, device=DEV, dtype=torch.int32)
    call("care_gemm_tile_argmax", _p(A), K, _p(W), _p(pm), _p(pi), _p(ps), _p(labels), _p(pl), M, N, K)
    logp, pred = torch.empty(M, device=DEV), torch.empty(M, device=DEV, dtype=torch.int32)
    call("care_score_partials", _p(pm), _p(pi), _p(ps), _p(pl), parts, _p(logp), _p(pred), M)
    ref = A.double() @ W.double().t()
    want = torch.log_softmax(ref, dim=1).gather(1, labels.long().unsqueeze(1)).squeeze(1)
    torch.cuda.synchronize()
    top2 = ref.topk(2, dim=1)
    safe = (top2[0][:, 0] - top2[0][:, 1]) > 1e-3
    assert torch.equal(pred[safe].long(), top2[1][:, 0][safe])
    assert int(pred[0]) == 11 and int(pred[M - 1]) == N - 2
    _assert_f32(logp, want, "tile label log-probability")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_tile_batched_head_projections(variant):
    """care_gemm_tile_batched in its two uses at d_model = 1024, 16 heads (16-bit in, 16-bit out)."""
    h16, call = _h16(variant), _caller(variant)
    H, d, rows = 16, 1024, 130
    q = _rand(rows, d, seed=21).to(h16)
    wkt = _rand(H, d, 64, seed=22, scale=0.05).to(h16)
    qt = torch.full((rows, H, d), float("nan"), device=DEV, dtype=h16)
    call("care_gemm_tile_batched", _p(q), d, 64, _p(wkt), 64, d * 64, None, 0, _p(qt), H * d, d, 1, H, rows, d, 64)
    ref = torch.einsum("rhe,hce->rhc", q.double().view(rows, H, 64), wkt.double())
    ct = _rand(rows, H, d, seed=23, scale=0.5).to(h16)
    wv = _rand(d, d, seed=24, scale=0.03).to(h16)
    bv = _rand(d, seed=25)
    ctx = torch.full((rows, d), float("nan"), device=DEV, dtype=h16)
    call("care_gemm_tile_batched", _p(ct), H * d, d, _p(wv), d, 64 * d, _p(bv), 64, _p(ctx), d, 64, 1, H, rows, 64, d)
    ref2 = torch.einsum("rhc,hec->rhe", ct.double(), wv.double().view(H, 64, d)).reshape(rows, d) + bv.double()
    torch.cuda.synchronize()
    _assert_h16(qt, ref, h16, "batched expand")
    _assert_h16(ctx, ref2, h16, "batched reduce")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,N,split", [(1280, 512, False), (640, 1536, True)])
def test_tile_and_a_stationary_gemm_agree_bit_for_bit(M, N, split, variant):
    """Both kernels add K = 512 in ascending order into one accumulator per output: the same bits, fp32 or 16-bit."""
    h16, call = _h16(variant), _caller(variant)
    K = 512
    A = _rand(M, K, seed=81).to(h16).contiguous()
    W = _rand(N, K, seed=82, scale=1 / math.sqrt(K)).to(h16).contiguous()
    bias = _rand(N, seed=83)
    outs = []
    for fn in ("care_gemm_bf16", "care_gemm_tile"):
        if split:
            o0, o1 = torch.zeros(M, 512, device=DEV), torch.zeros(M, N - 512, device=DEV, dtype=h16)
            tail = (_p(bias), _p(o0), 512, 0, _p(o1), N - 512, 1, 512, M, N, K, 0)
        else:
            o0, o1 = torch.zeros(M, N, device=DEV, dtype=h16), None
            tail = (_p(bias), _p(o0), N, 1, None, 0, 0, N, M, N, K, 0)
        call(fn, _p(A), K, *((1,) if fn == "care_gemm_bf16" else ()), _p(W), *tail)
        outs.append((o0, o1))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and float(outs[0][0].float().abs().max()) > 0.1
    if split:
        assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("a_f32", [True, False])
@pytest.mark.parametrize("M,K", [(7, 128), (200, 2048), (28 * 300, 512)])
def test_gemm_ln(M, K, a_f32, packed, variant):
    """care_gemm_ln / care_gemm_ln_packed: dense + residual (+ positions) + LayerNorm, fp32 rows and their 16-bit mirror
    in one call; with out = NULL only the mirror is written, with the same bits."""
    h16, call = _h16(variant), _caller(variant)
    d, grp = 512, 28 if M % 28 == 0 else M
    A = _rand(M, K, seed=50)
    W = _rand(d, K, seed=51, scale=1 / math.sqrt(K)).to(h16).contiguous()
    bias, g, b = _rand(d, seed=52), _rand(d, seed=53), _rand(d, seed=54)
    res = _rand(M, d, seed=55)
    pos = _rand(grp, d, seed=56) if (grp == 28 and not packed) else None
    Ain = A if a_f32 else A.to(h16).contiguous()
    ngrp = M // grp
    out = torch.zeros(ngrp, grp + 9, d, device=DEV)
    outb = torch.zeros(ngrp, grp + 9, d, device=DEV, dtype=h16)
    only = torch.zeros(ngrp, grp + 9, d, device=DEV, dtype=h16)
    if packed:
        Wp = torch.empty_like(W)
        call("care_pack_ln_weight", _p(W), _p(Wp), d, K)
        for o, ob in ((out, outb), (None, only)):
            call("care_gemm_ln_packed", _p(Ain), K, int(not a_f32), _p(Wp), _p(bias), _p(res), d, _p(g), _p(b), 1e-12,
                 _p(o), _p(ob), d, M, d, K, grp, grp + 9, 4)
    else:
        for o, ob in ((out, outb), (None, only)):
            call("care_gemm_ln", _p(Ain), K, int(not a_f32), _p(W), _p(bias), _p(res), d, _p(pos), _p(g), _p(b), 1e-12,
                 _p(o), _p(ob), d, M, d, K, grp, grp + 9, 4)
    y = A.to(h16).double() @ W.double().t() + bias.double() + res.double()
    if pos is not None:
        y = (y.view(ngrp, grp, d) + pos.double().unsqueeze(0)).view(M, d)
    ref = torch.nn.functional.layer_norm(y, (d,), g.double(), b.double(), 1e-12).view(ngrp, grp, d)
    torch.cuda.synchronize()
    _assert_f32(out[:, 4:4 + grp], ref, "gemm_ln")
    assert out[:, :4].abs().max().item() == 0 and out[:, 4 + grp:].abs().max().item() == 0
    assert torch.equal(outb.view(torch.int16), out.to(h16).view(torch.int16))
    assert torch.equal(only.view(torch.int16), outb.view(torch.int16))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,V", [(130, 3000), (8192 + 40, 700)])
def test_gemm_collect_with_a_full_staging_area(M, V, variant):
    """care_gemm_collect_bf16 with a threshold every logit reaches: all V columns of every row, once each, with their
    logits.  A work item stages at most 1023 candidates in LDS; the rest go straight to the global lists.  130 x 3000:
    the 128-row panels of csrc/gemm_as.hip; 8232 x 700: the 256-row panels of csrc/gemm_vocab.hip, ragged last tile."""
    K = 512
    h16, call = _h16(variant), _caller(variant)
    A = _rand(M, K, seed=71).to(h16)
    W = _rand(V, K, seed=72, scale=1 / math.sqrt(K)).to(h16)
    thr = torch.full((M,), -1e30, device=DEV)
    cnt = torch.zeros(M, device=DEV, dtype=torch.int32)
    cval = torch.full((M, V), float("nan"), device=DEV)
    cidx = torch.full((M, V), -1, device=DEV, dtype=torch.int32)
    call("care_gemm_collect_bf16", _p(A), K, 1, _p(W), _p(thr), _p(cnt), _p(cval), _p(cidx), V, M, V, K)
    torch.cuda.synchronize()
    assert torch.equal(cnt, torch.full_like(cnt, V))
    cols, order = cidx.long().sort(1)
    assert torch.equal(cols, torch.arange(V, device=DEV).expand(M, V))
    _assert_f32(cval.gather(1, order), A.double() @ W.double().t(), "gemm_collect, full staging area")


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("d", [512, 1024])
def test_add_ln_mirror(d, variant):
    h16, call = _h16(variant), _caller(variant)
    rows, grp = 37 * 4 + 3, 7
    x, res = _rand(rows, d, seed=11, scale=3.0), _rand(rows, d, seed=12)
    g, b = _rand(d, seed=13) + 1.0, _rand(d, seed=14)
    out = torch.full((rows + grp, d), float("nan"), device=DEV)
    outb = torch.zeros(rows + grp, d, device=DEV, dtype=h16)
    call("care_add_ln", _p(x), d, _p(res), d, None, _p(g), _p(b), 1e-12, _p(out), _p(outb), d, rows, d, grp, grp, 0, 1, 0)
    ref = torch.nn.functional.layer_norm(x.double() + res.double(), (d,), g.double(), b.double(), 1e-12)
    torch.cuda.synchronize()
    _assert_f32(out[:rows], ref, "add_ln", bar=2e-5)
    assert torch.equal(outb[:rows].view(torch.int16), out[:rows].to(h16).view(torch.int16))
    assert bool(torch.isnan(out[rows:]).all()) and outb[rows:].float().abs().max().item() == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_embed_ln_mirror(variant):
    """care_embed_ln: word + position + semantic vector, LayerNorm; the 16-bit mirror is the fp32 row rounded once."""
    h16, call = _h16(variant), _caller(variant)
    d, V, T, B = 512, 1000, 29, 3
    word, pos, sem = _rand(V, d, seed=13), _rand(30, d, seed=14), _rand(B, d, seed=15)
    g, b = _rand(d, seed=11), _rand(d, seed=12)
    tok = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(DEV)
    o2 = torch.zeros(B * T, d, device=DEV)
    o2b = torch.zeros(B * T, d, device=DEV, dtype=h16)
    call("care_embed_ln", _p(tok), T, 0, None, 0, _p(word), _p(pos), 0, _p(sem), T, _p(g), _p(b), 1e-12, _p(o2), _p(o2b), d, B * T, T, d)
    x = word[tok.long()].double() + pos[:T].double().unsqueeze(0) + sem.double().unsqueeze(1)
    ref = torch.nn.functional.layer_norm(x, (d,), g.double(), b.double(), 1e-12).view(B * T, d)
    torch.cuda.synchronize()
    _assert_f32(o2, ref, "embed_ln", bar=2e-5)
    assert torch.equal(o2b.view(torch.int16), o2.to(h16).view(torch.int16))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows,parts,d", [(5, 7, 512), (33, 512, 1024)])
def test_greedy_update_embed_equals_the_two_kernels(rows, parts, d, variant):
    """care_greedy_update_embed == care_greedy_update followed by the next step's care_embed_ln, 16-bit mirror included."""
    h16, call = _h16(variant), _caller(variant)
    V, T, t = 300, 29, 4
    pmax = _rand(rows, parts, seed=41)
    psum = _rand(rows, parts, seed=42).abs() + 0.1
    pidx = torch.randint(0, V, (rows, parts), generator=torch.Generator().manual_seed(rows), dtype=torch.int32).to(DEV)
    word, pos = _rand(V, d, seed=43), _rand(T + 1, d, seed=44)
    sem = _rand(rows, d, seed=45)
    g, b = _rand(d, seed=46), _rand(d, seed=47)

    def state():
        fed = torch.zeros(rows, T + 1, device=DEV, dtype=torch.int32)
        score = _rand(rows, seed=48).clone()
        length = torch.zeros(rows, device=DEV, dtype=torch.int32)
        fin = (torch.arange(rows, device=DEV) % 3 == 0).to(torch.int32)
        return fed, score, length, fin

    f1, s1, l1, n1 = state()
    x1 = torch.empty(rows, d, device=DEV); x1b = torch.empty(rows, d, device=DEV, dtype=h16)
    call("care_greedy_update", _p(pmax), _p(pidx), _p(psum), parts, _p(f1), T + 1, _p(s1), _p(l1), _p(n1), t, T, 3, rows)
    call("care_embed_ln", _p(f1), T + 1, t, None, 0, _p(word), _p(pos), t, _p(sem), 1, _p(g), _p(b), 1e-12, _p(x1), _p(x1b), d, rows, 1, d)
    f2, s2, l2, n2 = state()
    x2 = torch.empty(rows, d, device=DEV); x2b = torch.empty(rows, d, device=DEV, dtype=h16)
    call("care_greedy_update_embed", _p(pmax), _p(pidx), _p(psum), parts, _p(f2), T + 1, _p(s2), _p(l2), _p(n2), t, T,
         3, rows, _p(word), _p(pos), _p(sem), 1, _p(g), _p(b), 1e-12, _p(x2), _p(x2b), d, d)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2) and torch.equal(s1, s2) and torch.equal(l1, l2) and torch.equal(n1, n2)
    assert torch.equal(x1, x2) and torch.equal(x1b.view(torch.int16), x2b.view(torch.int16))
    assert torch.equal(x2b.view(torch.int16), x2.to(h16).view(torch.int16))


# ------------------------------------------------------------------------------------------------ head projections
# bf16: the bars of test_head_expand_and_reduce in test_gpu_kernels.py (relative to max(1, max |ref|)); half may never
# exceed them, and its own bars are 2 x the worst error measured on an MI355X.
HEAD_EXPAND_BAR = {"": 4e-3, "f16": 6.4e-4}   # measured: bf16 2.58e-3, half 3.21e-4
HEAD_REDUCE_BAR = {"": 8e-3, "f16": 7.4e-4}   # measured: bf16 3.22e-3, half 3.72e-4


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows,heads", [(1, 8), (16, 8), (250, 8), (33, 4)])
def test_head_expand_and_reduce(rows, heads, variant):
    """care_head_expand qt[r][h] = wkt[h] q[r, 64 h :], care_head_reduce ctx[r, 64 h :] = W_v[64 h :] ct[r][h] + b_v
    (csrc/heads.hip), 16-bit in and out."""
    h16, call = _h16(variant), _caller(variant)
    q = _rand(rows, 512, seed=1).to(h16)
    wkt = _rand(heads, 512, 64, seed=2, scale=0.05).to(h16)
    qt = torch.full((rows, heads, 512), float("nan"), device=DEV, dtype=h16)
    call("care_head_expand", _p(q), 512, _p(wkt), _p(qt), heads * 512, rows, heads)
    ref = torch.einsum("rhe,hce->rhc", q.double()[:, : heads * 64].reshape(rows, heads, 64), wkt.double())
    torch.cuda.synchronize()
    assert torch.isfinite(qt.float()).all()
    err = (qt.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("head_expand [%s] rows %d heads %d: relative error %.3g / %.3g" % (variant, rows, heads, err, HEAD_EXPAND_BAR[variant]))
    assert err < HEAD_EXPAND_BAR[variant] <= HEAD_EXPAND_BAR[""]

    ct = _rand(rows, heads, 512, seed=3).to(h16)
    wv = _rand(512, 512, seed=4, scale=0.05).to(h16)
    bv = _rand(512, seed=5)
    for bias in (bv, None):
        ctx = torch.full((rows, 512), float("nan"), device=DEV, dtype=h16)
        call("care_head_reduce", _p(ct), heads * 512, _p(wv), _p(bias), _p(ctx), 512, rows, heads)
        ref = torch.einsum("rhc,hec->rhe", ct.double(), wv.double()[: heads * 64].reshape(heads, 64, 512)).reshape(rows, -1)
        if bias is not None:
            ref = ref + bias.double()[: heads * 64]
        torch.cuda.synchronize()
        got = ctx.double()[:, : heads * 64]
        assert torch.isfinite(got).all()
        err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        print("head_reduce [%s] rows %d heads %d: relative error %.3g / %.3g" % (variant, rows, heads, err, HEAD_REDUCE_BAR[variant]))
        assert err < HEAD_REDUCE_BAR[variant] <= HEAD_REDUCE_BAR[""]


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ctx16", [False, True])
@pytest.mark.parametrize("nkeys,causal", [(7, False), (84, False), (114, False), (29, True)])
def test_attention_16bit_cache(nkeys, causal, ctx16, variant):
    """care_attention (csrc/attention.hip) on a 16-bit K/V cache: fp32 arithmetic on the rounded cache; padded keys."""
    h16, call = _h16(variant), _caller(variant)
    B, H, d, per = 3, 8, 512, (29 if causal else 5)
    rows = B * per
    q = _rand(rows, d, seed=16)
    kv = _rand(B * nkeys, 2 * d, seed=17).to(h16).contiguous()
    bias = _rand(H, nkeys, seed=18)
    tok = torch.randint(0, 4, (B, nkeys), generator=torch.Generator().manual_seed(nkeys), dtype=torch.int32).to(DEV)
    tok[:, 0] = 2
    tok[1, nkeys - 1] = 0
    ctx = torch.zeros(rows, d, device=DEV, dtype=h16 if ctx16 else torch.float32)
    call("care_attention", _p(q), d, _p(kv), _p(kv[:, d:]), 1, nkeys * 2 * d, 2 * d, per, None, 0, nkeys, int(causal), per, 0,
         _p(tok), nkeys, 0, _p(bias), nkeys, _p(ctx), d, int(ctx16), rows, H)
    kvf = kv.double().view(B, nkeys, 2, H, 64)
    k, v = kvf[:, :, 0].permute(0, 2, 1, 3), kvf[:, :, 1].permute(0, 2, 1, 3)
    qh = q.double().view(B, per, H, 64).permute(0, 2, 1, 3)
    s = qh @ k.transpose(-1, -2) / 8.0
    mask = tok.eq(0).view(B, 1, 1, nkeys).expand(B, H, per, nkeys).clone()
    if causal:
        mask |= torch.triu(torch.ones(per, nkeys, dtype=torch.bool, device=DEV), 1).view(1, 1, per, nkeys)
    s = s.masked_fill(mask, -1e9) + bias.double().view(1, H, 1, nkeys)
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(rows, d)
    torch.cuda.synchronize()
    # (fp32 arithmetic on the rounded cache, no MFMA: the 2e-5 of test_attention in test_gpu_kernels.py)
    (_assert_h16(ctx, ref, h16, "attention", bar32=2e-5) if ctx16 else _assert_f32(ctx, ref, "attention", bar=2e-5))


# attention_seq rounds the probabilities and the output to 16 bits.  bf16: the bars of test_attention_seq in
# test_gpu_kernels.py; half: 2 x the worst error measured on an MI355X, never above bf16's.
SEQ_MAX_BAR = {"": 4e-2, "f16": 3.9e-3}     # measured: bf16 1.54e-2, half 1.94e-3
SEQ_MEAN_BAR = {"": 3e-3, "f16": 2.9e-4}    # measured: bf16 1.15e-3, half 1.43e-4


def _seq_case(nseq, seq, nkeys, per_kv, kind, h16, q_scale=1.5, kv_scale=None):
    H, d = 8, 512
    kv_scale = kv_scale or (1.5 if kind == "self" else 1.0)
    rows = nseq * seq
    g = torch.Generator().manual_seed(nseq * 131 + nkeys)
    if kind == "self":
        qkv = torch.randn(rows, 3 * d, generator=g)
        qkv[:, :d] *= q_scale
        qkv[:, d:] *= kv_scale
        qkv = qkv.to(DEV).to(h16)
        Q, K, V = qkv, qkv[:, d:], qkv[:, 2 * d:]
        ldq, kbs, krs = 3 * d, seq * 3 * d, 3 * d
        tok = torch.randint(1, 50, (nseq, seq), generator=g).to(DEV).to(torch.int32)
        tok[:, 0] = 1
        tok[0, 3] = 0
        tok[nseq - 1, seq - 2:] = 0       # PAD keys (id 0), also at a row's own position
        bias = None
        Kf = qkv[:, d:2 * d].double().view(nseq, seq, H, 64)
        Vf = qkv[:, 2 * d:].double().view(nseq, seq, H, 64)
        Qf = qkv[:, :d].double().view(nseq, seq, H, 64)
    else:
        nkv = nseq // per_kv
        q = (torch.randn(rows, d, generator=g) * q_scale).to(DEV).to(h16)
        kv = (torch.randn(nkv * nkeys, 2 * d, generator=g) * kv_scale).to(DEV).to(h16)
        Q, K, V = q, kv, kv[:, d:]
        ldq, kbs, krs = d, nkeys * 2 * d, 2 * d
        tok = None
        bias = (torch.randn(H, nkeys, generator=g) * 0.5).to(DEV)
        idx = torch.arange(nseq, device=DEV) // per_kv
        Kf = kv[:, :d].double().view(nkv, nkeys, H, 64)[idx]
        Vf = kv[:, d:].double().view(nkv, nkeys, H, 64)[idx]
        Qf = q.double().view(nseq, seq, H, 64)
    args = (_p(Q), ldq, _p(K), _p(V), kbs, krs, per_kv, nkeys, 1 if kind == "self" else 0, seq, _p(tok),
            seq if tok is not None else 0, 0, _p(bias), nkeys if bias is not None else 0)
    keep = (Q, K, V, tok, bias)

    def reference(Kx=Kf, Vx=Vf):
        sc = torch.einsum("sqhe,skhe->shqk", Qf, Kx) / 8.0
        if kind == "self":
            mask = (tok == 0)[:, None, None, :] | torch.triu(torch.ones(seq, seq, device=DEV, dtype=torch.bool), 1)[None, None]
            sc = sc.masked_fill(mask, -1e9)
        if bias is not None:
            sc = sc + bias.double()[None, :, None, :]
        return torch.einsum("shqk,skhe->sqhe", torch.softmax(sc, dim=-1), Vx).reshape(rows, d)

    return args, keep, reference, (Kf, Vf)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nseq,seq,nkeys,per_kv,kind", [(7, 29, 29, 1, "self"), (9, 29, 84, 3, "cross")])
def test_attention_seq(nseq, seq, nkeys, per_kv, kind, variant):
    """csrc/attention_seq.hip: one wave per (sequence, head); causal + key-padding mask for self-attention, per-(head, key)
    bias and key/value blocks shared by `per_kv` sequences for cross-attention."""
    h16, call = _h16(variant), _caller(variant)
    args, keep, reference, _ = _seq_case(nseq, seq, nkeys, per_kv, kind, h16)
    ctx = torch.full((nseq * seq, 512), float("nan"), device=DEV, dtype=h16)
    call("care_attention_seq", *args, _p(ctx), 512, nseq, 8)
    ref = reference()
    torch.cuda.synchronize()
    got = ctx.double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    print("attention_seq [%s] %s: max error %.3g / %.3g, mean %.3g / %.3g" % (
        variant, kind, err.max().item(), SEQ_MAX_BAR[variant], err.mean().item(), SEQ_MEAN_BAR[variant]))
    assert err.max().item() < SEQ_MAX_BAR[variant] <= SEQ_MAX_BAR[""]
    assert err.mean().item() < SEQ_MEAN_BAR[variant] <= SEQ_MEAN_BAR[""]


# The absorbed cross-attention rounds the probabilities and the output to 16 bits.  bf16: the bars of test_attention_latent*
# in test_gpu_kernels.py (maximum relative to max(1, max |ref|), and the mean); half: 2 x the worst error measured on an
# MI355X, never above bf16's.
LAT_MAX_BAR = {"": 1.2e-2, "f16": 1.3e-3}   # measured: bf16 5.20e-3, half 6.39e-4
LAT_MEAN_BAR = {"": 2e-3, "f16": 2.5e-4}    # measured: bf16 8.90e-4, half 1.23e-4


def _latent_check(ct, ref, variant, what):
    assert torch.isfinite(ct.float()).all(), what
    err = (ct.double() - ref).abs()
    rel = err.max().item() / max(1.0, ref.abs().max().item())
    print("attention_latent [%s] %s: max error %.3g / %.3g, mean %.3g / %.3g" % (
        variant, what, rel, LAT_MAX_BAR[variant], err.mean().item(), LAT_MEAN_BAR[variant]))
    assert rel < LAT_MAX_BAR[variant] <= LAT_MAX_BAR[""], what
    assert err.mean().item() < LAT_MEAN_BAR[variant] <= LAT_MEAN_BAR[""], what


def _latent_case(rows, nkeys, rows_per_kv, H, d, h16, q_scale):
    clips = (rows + rows_per_kv - 1) // rows_per_kv
    mem = _rand(clips, nkeys, d, seed=11).to(h16)
    qt = _rand(rows, H, d, seed=12, scale=q_scale).to(h16)
    bias = _rand(H, nkeys, seed=13, scale=0.7)
    m = mem.double()[torch.arange(rows, device=DEV) // rows_per_kv]
    s = torch.einsum("rhc,rjc->rhj", qt.double(), m) + bias.double()[None]
    return mem, qt, bias, torch.einsum("rhj,rjc->rhc", torch.softmax(s, -1), m)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows,nkeys,rows_per_kv,H,d", [(1, 84, 1, 8, 512), (35, 57, 5, 8, 512), (130, 114, 1, 8, 512),
                                                        (12, 40, 3, 4, 512), (77, 84, 1, 16, 1024), (77, 84, 1, 12, 768)])
def test_attention_latent(rows, nkeys, rows_per_kv, H, d, variant):
    """ct[r][h] = softmax_j(qt[r][h] . mem[clip][j] + bias[h][j]) . mem[clip] (csrc/attention_latent.hip): one row, pairs of
    rows that share a clip and the odd row out, four heads, and the several-waves-per-row forms of d_model 1024 / 768."""
    h16, call = _h16(variant), _caller(variant)
    mem, qt, bias, ref = _latent_case(rows, nkeys, rows_per_kv, H, d, h16, 0.12 if d == 512 else 0.09)
    ct = torch.full((rows, H, d), float("nan"), device=DEV, dtype=h16)
    call("care_attention_latent", _p(qt), H * d, _p(mem), nkeys * d, d, rows_per_kv, nkeys, _p(bias), nkeys, _p(ct), H * d, rows, H, d)
    torch.cuda.synchronize()
    _latent_check(ct, ref, variant, "rows %d keys %d per clip %d heads %d d %d" % (rows, nkeys, rows_per_kv, H, d))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows,nkeys", [(128, 114), (256, 128)])
def test_attention_latent_few_rows_is_bit_identical_to_the_streaming_kernel(rows, nkeys, variant):
    """Up to 256 rows: one wave per row with the head of its stream in flight - the same bits as those rows' slice of a
    300-row launch, which takes the streaming kernel."""
    h16, call = _h16(variant), _caller(variant)
    H, d, big = 8, 512, 300
    mem, qt, bias, ref = _latent_case(big, nkeys, 1, H, d, h16, 0.12)
    out_big = torch.full((big, H, d), float("nan"), device=DEV, dtype=h16)
    out_few = torch.full((rows, H, d), float("nan"), device=DEV, dtype=h16)
    for o, n in ((out_big, big), (out_few, rows)):
        call("care_attention_latent", _p(qt), H * d, _p(mem), nkeys * d, d, 1, nkeys, _p(bias), nkeys, _p(o), H * d, n, H, d)
    torch.cuda.synchronize()
    assert torch.equal(out_few.view(torch.int16), out_big[:rows].view(torch.int16))
    _latent_check(out_big, ref, variant, "streaming, keys %d" % nkeys)


# ------------------------------------------------------------------------------------------------ beam and scoring
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,V", [(5, 700), (300, 700), (5, 10547), (300, 10547), (8192 + 40, 10547)])
def test_fused_beam_selection_equals_logits_plus_beam_select(M, V, variant):
    """statistics GEMM -> threshold -> candidate GEMM (care_gemm_collect_bf16) -> pick  ==  the stored logits +
    care_beam_select of the same library: the same ids in the same order, with tied columns and (large V) a plateau at the
    top of row 1 that overflows the candidate list.  The sparse second pass (csrc/beam_sparse.hip:
    care_gemm_argmax_bf16_tiles + care_beam_sparse_collect) and the collect mode of the 256-row panels (csrc/gemm_vocab.hip)
    exist only from 8192 rows: the last shape is there for them, with a ragged last panel, and the test asserts that
    the library takes the sparse pass for that shape and for no other."""
    h16, call, lib = _h16(variant), _caller(variant), _lib_of(variant)
    assert bool(lib.care_beam_sparse_applies(M, V, 512, 1)) == (M >= 8192)
    K, bm, cap = 512, 5, 64
    A = _rand(M, K, seed=51).to(h16)
    W = _rand(V, K, seed=52, scale=0.05).to(h16)
    W[17] = W[400]
    if V > 5000:
        W[3000:3100] = W[2999]
        A[1] = (W[2999].float() * 40).to(h16)
    ld = (V + 63) // 64 * 64
    logits = torch.empty(M, ld, device=DEV)
    call("care_gemm_bf16", _p(A), K, 1, _p(W), None, _p(logits), ld, 0, None, 0, 0, V, M, V, K, 0)
    ref_v = torch.zeros(M, bm, device=DEV); ref_i = torch.zeros(M, bm, device=DEV, dtype=torch.int32)
    call("care_beam_select", _p(logits), ld, V, bm, _p(ref_v), _p(ref_i), M, 1)
    parts = lib.care_argmax_parts_bf16_min(M, V, K, 1, 8)
    pmax = torch.empty(M, parts, device=DEV); psum = torch.empty(M, parts, device=DEV)
    pidx = torch.empty(M, parts, device=DEV, dtype=torch.int32)
    thr = torch.empty(M, device=DEV); cnt = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    cval = torch.empty(M, cap, device=DEV); cidx = torch.empty(M, cap, device=DEV, dtype=torch.int32)
    got_v = torch.zeros(M, bm, device=DEV); got_i = torch.zeros(M, bm, device=DEV, dtype=torch.int32)
    call("care_gemm_argmax_bf16_min", _p(A), K, 1, _p(W), _p(pmax), _p(pidx), _p(psum), M, V, K, 8)
    call("care_beam_threshold", _p(pmax), parts, bm, _p(thr), _p(cnt), M)
    call("care_gemm_collect_bf16", _p(A), K, 1, _p(W), _p(thr), _p(cnt), _p(cval), _p(cidx), cap, M, V, K)
    call("care_beam_pick", _p(pmax), _p(psum), parts, _p(cnt), _p(cval), _p(cidx), cap, bm, _p(A), K, 1, _p(W), V, K,
         _p(got_v), _p(got_i), M)
    torch.cuda.synchronize()
    if lib.care_beam_sparse_applies(M, V, K, 1):
        tiles = (V + 31) // 32
        tmx = torch.full((tiles, M), float("nan"), device=DEV)
        pm2, ps2, pi2 = torch.empty_like(pmax), torch.empty_like(psum), torch.empty_like(pidx)
        thr2 = torch.empty_like(thr); cnt2 = torch.full_like(cnt, -1)
        cval2, cidx2 = torch.empty_like(cval), torch.empty_like(cidx)
        tcount = torch.full((2 * tiles + 1,), -3, device=DEV, dtype=torch.int32)
        tlist = torch.empty(tiles, M, device=DEV, dtype=torch.int32)
        sp_v, sp_i = torch.zeros_like(got_v), torch.zeros_like(got_i)
        call("care_gemm_argmax_bf16_tiles", _p(A), K, 1, _p(W), _p(pm2), _p(pi2), _p(ps2), _p(tmx), M, V, K, 8)
        call("care_beam_threshold", _p(pm2), parts, bm, _p(thr2), _p(cnt2), M)
        call("care_beam_sparse_collect", _p(A), K, _p(W), _p(tmx), _p(thr2), _p(cnt2), _p(cval2), _p(cidx2), cap,
             _p(tcount), _p(tlist), M, V, K)
        call("care_beam_pick", _p(pm2), _p(ps2), parts, _p(cnt2), _p(cval2), _p(cidx2), cap, bm, _p(A), K, 1, _p(W), V, K,
             _p(sp_v), _p(sp_i), M)
        torch.cuda.synchronize()
        assert torch.equal(pm2, pmax) and torch.equal(pi2, pidx) and torch.equal(ps2, psum)
        assert torch.equal(tmx.max(0).values, pmax.max(1).values)      # the map's row maxima are the rows' maxima
        assert torch.equal(cnt2, cnt)                                   # the same number of candidates per row ...
        assert torch.equal(sp_i, got_i) and torch.equal(sp_v, got_v)    # ... and the same picks, bit for bit
        assert int(tcount[:tiles].sum()) >= M and int(tcount[:tiles].max()) <= M   # the sparse pass did run
        assert int(tcount[2 * tiles]) == int(((tcount[:tiles] + 127) // 128).sum())
    assert int(cnt.min()) >= bm
    if V > 5000:
        assert int(cnt[1]) > cap
    assert torch.equal(got_i, ref_i)
    over = cnt > cap
    assert (got_v[~over] - ref_v[~over]).abs().max().item() < 2e-5
    if bool(over.any()):
        assert (got_v[over] - ref_v[over]).abs().max().item() < 1e-3
    # and the ids are the float64 product's wherever that one is decided by more than the fp32 bar
    order = (A.double() @ W.double().t()).topk(bm + 1, dim=1)
    safe = ((order[0][:, :-1] - order[0][:, 1:]) > BAR32).all(1)
    assert torch.equal(got_i[safe].long(), order[1][:, :bm][safe])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,V", [(5, 700), (300, 700), (5, 10547), (300, 10547)])
def test_beam_selection_from_group_maxima_equals_logits_plus_beam_select(M, V, variant):
    """care_gemm_tile_beam -> care_beam_pick_groups  ==  the logits of the same tile kernel + care_beam_select."""
    h16, call, lib = _h16(variant), _caller(variant), _lib_of(variant)
    K, bm = 512, 5
    A = _rand(M, K, seed=61).to(h16)
    W = _rand(V, K, seed=62, scale=0.05).to(h16)
    W[17] = W[40]
    if V > 5000:
        W[3000:3100] = W[2999]
        A[1] = (W[2999].float() * 40).to(h16)
    ld = (V + 63) // 64 * 64
    logits = torch.empty(M, ld, device=DEV)
    call("care_gemm_tile", _p(A), K, _p(W), None, _p(logits), ld, 0, None, 0, 0, V, M, V, K, 0)
    ref_v = torch.zeros(M, bm, device=DEV); ref_i = torch.zeros(M, bm, device=DEV, dtype=torch.int32)
    call("care_beam_select", _p(logits), ld, V, bm, _p(ref_v), _p(ref_i), M, 1)
    parts = lib.care_argmax_parts_tile(V)
    pmax = torch.full((M, parts), float("nan"), device=DEV); psum = torch.full((M, parts), float("nan"), device=DEV)
    gmax = torch.full((M, parts, 16), float("nan"), device=DEV)
    got_v = torch.zeros(M, bm, device=DEV); got_i = torch.zeros(M, bm, device=DEV, dtype=torch.int32)
    call("care_gemm_tile_beam", _p(A), K, _p(W), _p(pmax), _p(psum), _p(gmax), M, V, K)
    call("care_beam_pick_groups", _p(pmax), _p(psum), _p(gmax), parts, bm, _p(A), K, _p(W), V, K, _p(got_v), _p(got_i), M)
    torch.cuda.synchronize()
    pad = torch.full((M, parts * 64 - V), float("-inf"), device=DEV)
    blocks = torch.cat([logits[:, :V], pad], 1).view(M, parts, 16, 4)
    assert torch.equal(gmax, blocks.max(-1).values)
    assert torch.equal(got_i, ref_i)
    assert (got_v - ref_v).abs().max().item() < 2e-5
    if V > 5000:
        assert got_i[1].tolist() == [2999, 3000, 3001, 3002, 3003]
    _assert_f32(logits[:, :V], A.double() @ W.double().t(), "tile logits")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows,K", [(5, 512), (300, 520)])
def test_label_logits(rows, K, variant):
    """care_label_logits: out[r] = A[r] . W[col[r]] on 16-bit operands, a full pass and a pass plus one lane."""
    h16, call = _h16(variant), _caller(variant)
    N = 10547
    A = _rand(rows, K, seed=130).to(h16)
    W = _rand(N, K, seed=131, scale=0.05).to(h16).contiguous()
    col = torch.randint(1, N - 1, (rows,), generator=torch.Generator().manual_seed(rows + K), dtype=torch.int32).to(DEV)
    col[0], col[rows - 1] = 0, N - 1
    out = torch.full((rows + 4,), float("nan"), device=DEV)
    call("care_label_logits", _p(A), K, _p(W), _p(col), _p(out), rows, N, K)
    ref = (A.double() * W[col.long()].double()).sum(1)
    torch.cuda.synchronize()
    _assert_f32(out[:rows], ref, "label logits", bar=1e-4)
    assert torch.isnan(out[rows:]).all()


# ================================================================================================ half's own edges
# (a) the lazy online softmax of the absorbed cross-attention.  The exponentials of a 16-key chunk are taken against a
# reference maximum that moves only when a chunk's maximum exceeds it by more than a threshold; they are cast to the
# 16-bit type for the P . mem MFMA, so exp(threshold) must be finite in it: half ends at 65504 = e^11.09.
#
# Scores are made EXACT: key j is a * e_j (one-hot, a a power of two) and qt[h][j] = s_hj / a with every s a multiple of
# 0.5 below 128 (exact in bf16), so the score of key j is s_hj to the bit and ct[h][j] = a * p_hj reads the probabilities
# out.  112 keys = 7 chunks of 16; the heads of a row carry different patterns, so the wave-uniform decision to rescale
# (taken when ANY head asks) meets heads that did not ask.
WIN_A, WIN_KEYS, WIN_D = 4.0, 112, 512
WIN_JUMPS = [4.0, 10.5, 11.5, 12.0, 15.5, 16.5, 24.0, 40.0]
# Against the float64 softmax, in units of probability.  bf16: DELIBERATELY the bars of test_attention_latent in
# test_gpu_kernels.py, inherited unchanged although these exact-score cases sit far below them (the mean by 100 x): they
# are the ceiling half may never exceed, not what would catch a moderately wrong rescale on bf16 - WIN_L1_BAR below is.
# half: 2 x the worst error measured on an MI355X (with the threshold at 8), never above bf16's.
WIN_MAX_BAR = {"": 1.2e-2, "f16": 4.9e-4}    # measured: bf16 3.90e-3, half 2.44e-4 (half an ulp of a probability near 1)
WIN_MEAN_BAR = {"": 2e-3, "f16": 4.2e-6}     # measured: bf16 2.00e-5, half 2.09e-6
# Derived from the formats, for both libraries: with exact scores the only roundings are the probability's (to p
# significand bits: 2^-p relative) and the output's (2^-p relative again), so key j is off by at most
# (2^-(p-1) + 2^-2p) p_j and a (row, head), whose probabilities sum to 1, by that in total; + 1e-5 for what is not
# proportional to p_j (the fp32 sum and __expf at arguments down to -126, half's subnormal probabilities: 2^-25 a key).
WIN_L1_BAR = {"": 2.0 ** -7 + 2.0 ** -16 + 1e-5, "f16": 2.0 ** -10 + 2.0 ** -22 + 1e-5}


def window_scores(case, heads=8):
    """[3 rows, heads, 112 keys] float64 scores, multiples of 0.5 with |s| < 128.  A head's pattern is the list of its
    chunks' maxima; the other keys of a chunk lie 0.5 .. 6 below the chunk's maximum.  `case` is a jump J - chunk 0 at 0,
    chunk 1 at J and its variants - or one of the two staircases, whose steps do not depend on J.  Row 0 mixes patterns
    over its heads, in row 1 every head carries the case's main pattern, in row 2 head 3 alone (the others stay flat)."""
    flat = [0.0] * 7
    if case == "staircase":
        main = [12.0 * c for c in range(7)]                     # +12 per chunk
        row0 = [main, flat, [12.0 * (c // 2) for c in range(7)], flat, main, [12.0 * max(c - 3, 0) for c in range(7)], flat, main]
    elif case == "descending":
        main = [-20.0 * c for c in range(7)]                    # 0, -20, -40, ...
        row0 = [main, flat, [-20.0 * (c // 2) for c in range(7)], flat, main, [-20.0 * max(c - 3, 0) for c in range(7)], flat, main]
    else:
        J = float(case)
        main = [0.0, J] + [0.0] * 5                             # chunk 0 at 0, chunk 1 at J, back to 0
        row0 = [main,
                [0.0] * 6 + [J],                                # the jump at the last chunk
                [J] + [0.0] * 6,                                # a high first chunk, then J lower
                "last",                                         # the maximum J at the last key of the last chunk
                [0.0, 0.0, 0.0, J, 0.0, 0.0, 0.0],              # the jump in the middle of the row
                flat,
                [0.0, J, 2 * J, 2 * J, 0.0, 0.0, 0.0],          # two jumps in a row
                [-J, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]             # a low first chunk
    rows = [row0, [main] * 8, [flat] * 3 + [main] + [flat] * 4]
    rng = np.random.RandomState(len(str(case)) + int(sum(map(abs, main))))
    s = np.zeros((3, heads, WIN_KEYS))
    for r in range(3):
        for h in range(heads):
            pat = rows[r][h % 8]
            for c in range(7):
                below = rng.randint(1, 13, size=16) * 0.5
                if pat == "last":
                    top, at = (J if c == 6 else 0.0), (15 if c == 6 else int(rng.randint(16)))
                    if c == 6:
                        below = below + J            # the rest of the last chunk stays below 0
                else:
                    top, at = pat[c], int(rng.randint(16))
                s[r, h, c * 16:(c + 1) * 16] = top - below
                s[r, h, c * 16 + at] = top
    assert np.all(s * 2 == np.round(s * 2)) and np.abs(s).max() < 128
    return torch.from_numpy(s)


def window_reference(case, heads=8):
    """(scores, float64 softmax) - checked to hold no inf / NaN; the probabilities of a row sum to 1."""
    s = window_scores(case, heads)
    p = torch.softmax(s, -1)
    assert torch.isfinite(s).all() and torch.isfinite(p).all() and (p.sum(-1) - 1).abs().max().item() < 1e-12
    return s, p


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("form", ["few rows", "paired rows", "streaming", "four waves per row"])
@pytest.mark.parametrize("case", WIN_JUMPS + ["staircase", "descending"])
def test_attention_latent_lazy_softmax_windows(case, form, variant):
    """Jumps of the running maximum below, inside and above the rescale threshold of either library, in every kernel that
    carries the lazy softmax: few rows (3 rows), paired rows (rows_per_kv = 2: rows 0 1 | 2 0), streaming (the 3 rows 100
    times) and the several-waves-per-row kernel of d_model 1024 (16 heads).  The output must be finite and equal the
    float64 softmax within the library's bar."""
    h16, call = _h16(variant), _caller(variant)
    H, d = (16, 1024) if form == "four waves per row" else (8, WIN_D)
    s, p = window_reference(case, H)
    pick = {"few rows": [0, 1, 2], "paired rows": [0, 1, 2, 0], "streaming": [0, 1, 2] * 100, "four waves per row": [0, 1, 2]}[form]
    rows, rows_per_kv = len(pick), 2 if form == "paired rows" else 1
    mem = torch.zeros(WIN_KEYS, d, device=DEV, dtype=h16)
    mem[torch.arange(WIN_KEYS), torch.arange(WIN_KEYS)] = WIN_A
    qt = torch.zeros(rows, H, d, device=DEV, dtype=h16)
    qt[:, :, :WIN_KEYS] = (s[pick] / WIN_A).to(DEV).to(h16)
    assert torch.equal(qt[:, :, :WIN_KEYS].double().cpu() * WIN_A, s[pick])       # the scores are exact in h16
    ct = torch.full((rows, H, d), float("nan"), device=DEV, dtype=h16)
    # one memory block for every clip (batch stride 0)
    call("care_attention_latent", _p(qt), H * d, _p(mem), 0, d, rows_per_kv, WIN_KEYS, None, 0, _p(ct), H * d, rows, H, d)
    torch.cuda.synchronize()
    got = ct.double().cpu()
    bad = ~torch.isfinite(got).all(-1)
    assert not bool(bad.any()), "inf / NaN in (row, head) %s" % bad.nonzero().tolist()[:8]
    assert got[:, :, WIN_KEYS:].abs().max().item() == 0
    err = (got[:, :, :WIN_KEYS] / WIN_A - p[pick]).abs()
    print("lazy softmax [%s] %s %s: max error %.3g / %.3g, mean %.3g / %.3g" % (
        variant, form, case, err.max().item(), WIN_MAX_BAR[variant], err.mean().item(), WIN_MEAN_BAR[variant]))
    l1 = err.sum(-1).max().item()
    print("lazy softmax [%s] %s %s: worst summed error of a (row, head) %.3g / %.3g" % (variant, form, case, l1, WIN_L1_BAR[variant]))
    assert err.max().item() < WIN_MAX_BAR[variant] <= WIN_MAX_BAR[""]
    assert err.mean().item() < WIN_MEAN_BAR[variant] <= WIN_MEAN_BAR[""]
    assert l1 <= WIN_L1_BAR[variant]


# (b) conversion semantics: fp32 -> 16 bits is round to nearest even, keeps subnormals, overflows to +-inf, makes no NaN.
def _wide_gamma(d):
    """Per-column LayerNorm gain from 1e-7 to 1e5 with alternating sign: the mirror of a normalised row spans half's
    subnormals (below 6.1e-5), its normals and values beyond 65504."""
    g = torch.pow(10.0, torch.linspace(-7, 5, d, dtype=torch.float64)).float()
    g[1::2] *= -1
    return g.to(DEV)


def _assert_mirror(outb, out, h16, what):
    want = out.to(h16)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(outb.float()).any()), what
    assert torch.equal(outb.view(torch.int16), want.view(torch.int16)), what
    if h16 == torch.float16:     # the case does reach the three regimes
        a = outb.float().abs()
        assert bool(torch.isinf(a).any()) and bool(((a > 0) & (a < 2.0 ** -14)).any()), what
        assert bool(torch.isfinite(out).all()), what


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel", ["care_gemm_ln", "care_gemm_ln_packed", "care_add_ln"])
def test_mirror_is_the_fp32_result_rounded_once(kernel, variant):
    """The entry points that write an fp32 result and its 16-bit mirror in one call: mirror == out32.to(h16), bit for bit,
    over subnormals, normals and overflow."""
    h16, call = _h16(variant), _caller(variant)
    M, K, d = 200, 512, 512
    g, b = _wide_gamma(d), torch.zeros(d, device=DEV)
    out = torch.zeros(M, d, device=DEV)
    outb = torch.zeros(M, d, device=DEV, dtype=h16)
    if kernel == "care_add_ln":
        x, res = _rand(M, d, seed=11, scale=3.0), _rand(M, d, seed=12)
        call("care_add_ln", _p(x), d, _p(res), d, None, _p(g), _p(b), 1e-12, _p(out), _p(outb), d, M, d, M, M, 0, 1, 0)
    else:
        A = _rand(M, K, seed=50)
        W = _rand(d, K, seed=51, scale=1 / math.sqrt(K)).to(h16).contiguous()
        bias, res = _rand(d, seed=52), _rand(M, d, seed=55)
        if kernel == "care_gemm_ln_packed":
            Wp = torch.empty_like(W)
            call("care_pack_ln_weight", _p(W), _p(Wp), d, K)
            call(kernel, _p(A), K, 0, _p(Wp), _p(bias), _p(res), d, _p(g), _p(b), 1e-12, _p(out), _p(outb), d, M, d, K, M, M, 0)
        else:
            call(kernel, _p(A), K, 0, _p(W), _p(bias), _p(res), d, None, _p(g), _p(b), 1e-12, _p(out), _p(outb), d, M, d, K, M, M, 0)
    torch.cuda.synchronize()
    _assert_mirror(outb, out, h16, kernel)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel", ["care_gemm_bf16", "care_gemm_tile"])
@pytest.mark.parametrize("regime,sa,sw", [("normal", 0, 0), ("overflow", 3, 2), ("subnormal", -10, -12)])
def test_16bit_only_output_is_the_exact_product_rounded_once(regime, sa, sw, kernel, variant):
    """16-bit C without an fp32 copy.  The operands are small integers times a power of two (A in -8 .. 8 times 2^sa, W in -32 .. 32
    times 2^sw, the bias in units of 2^(sa + sw)), so every product and every partial sum (below 2^24 units) is exact in fp32 in ANY order:
    the accumulator IS the float64 reference and the output must be that reference rounded to the 16-bit type - to nearest
    EVEN (sums beyond 2^8 / 2^11 units hit exact ties), to +-inf beyond the largest value (half, scaled by 2^5), with
    subnormals kept (half, scaled by 2^-22).  No element is excluded: none is near a rounding boundary it is not on."""
    h16, call = _h16(variant), _caller(variant)
    M, N, K = 130, 512, 512
    gen = torch.Generator().manual_seed(7)
    A = (torch.randint(-8, 9, (M, K), generator=gen).double() * 2.0 ** sa).to(DEV).to(h16)
    W = (torch.randint(-32, 33, (N, K), generator=gen).double() * 2.0 ** sw).to(DEV).to(h16)
    bias = (torch.randint(-64, 65, (N,), generator=gen).double() * 2.0 ** (sa + sw)).to(DEV).float()
    out = torch.full((M, N), float("nan"), device=DEV, dtype=h16)
    if kernel == "care_gemm_bf16":
        call(kernel, _p(A), K, 1, _p(W), _p(bias), _p(out), N, 1, None, 0, 0, N, M, N, K, 0)
    else:
        call(kernel, _p(A), K, _p(W), _p(bias), _p(out), N, 1, None, 0, 0, N, M, N, K, 0)
    ref = A.double() @ W.double().t() + bias.double()
    assert torch.equal(ref.float().double(), ref)            # the reference is an fp32 number: no double rounding below
    want = ref.to(h16)
    torch.cuda.synchronize()
    units = (ref / 2.0 ** (sa + sw)).abs()
    p = 8 if h16 == torch.bfloat16 else 11
    ties = ((units >= 2 ** p) & (units < 2 ** (p + 1)) & (units % 2 == 1)).sum().item()
    print("%s [%s] %s: %d exact ties, %d inf, %d subnormal" % (kernel, variant, regime, ties, int(torch.isinf(want.float()).sum()),
                                                               int(((want.float().abs() < 2.0 ** -14) & (want.float() != 0)).sum())))
    assert ties > 100                                          # round-to-nearest-EVEN is decided, not assumed
    if h16 == torch.float16 and regime == "overflow":
        assert int(torch.isinf(want.float()).sum()) > 100
    if h16 == torch.float16 and regime == "subnormal":
        assert int(((want.float().abs() < 2.0 ** -14) & (want.float() != 0)).sum()) > 1000
    assert not bool(torch.isnan(out.float()).any())
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


# (c) subnormal MFMA operands.  W = randn * 2e-5 is mostly SUBNORMAL in half (below 2^-14 = 6.1e-5; a normal number in
# bf16).  Two float64 references: subnormal operands kept, and flushed to zero.  Expected: kept (the MFMAs of gfx950 take
# 16-bit subnormals as they are); the references differ by far more than 10 x the bar, so the test decides between them.
def _flush(x16):
    """h16 tensor -> float64 with half's subnormals flushed to zero."""
    x = x16.double()
    return torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x) if x16.dtype == torch.float16 else x


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel", ["care_gemm_bf16", "care_gemm_tile"])
def test_subnormal_weights_gemm(kernel, variant):
    """MFMA 16x16x32 (care_gemm_bf16) and 32x32x16 (care_gemm_tile): A = randn * 1024, W = randn * 2e-5, fp32 C."""
    h16, call = _h16(variant), _caller(variant)
    M, N, K = 130, 512, 512
    A = _rand(M, K, seed=1, scale=1024.0).to(h16).contiguous()
    W = _rand(N, K, seed=2, scale=2e-5).to(h16).contiguous()
    out = torch.full((M, N), float("nan"), device=DEV)
    if kernel == "care_gemm_bf16":
        call(kernel, _p(A), K, 1, _p(W), None, _p(out), N, 0, None, 0, 0, N, M, N, K, 0)
    else:
        call(kernel, _p(A), K, _p(W), None, _p(out), N, 0, None, 0, 0, N, M, N, K, 0)
    kept, flushed = A.double() @ W.double().t(), A.double() @ _flush(W).t()
    torch.cuda.synchronize()
    if h16 == torch.float16:
        assert (W.float().abs() < 2.0 ** -14).float().mean().item() > 0.99
        assert (kept - flushed).abs().max().item() > 10 * BAR32 and (kept - flushed).abs().mean().item() > 10 * BAR32
    print("%s [%s]: |out - kept| %.3g, |out - flushed| %.3g" % (kernel, variant, (out.double() - kept).abs().max().item(),
                                                                 (out.double() - flushed).abs().max().item()))
    _assert_f32(out, kept, kernel + " subnormal W")


@pytest.mark.parametrize("variant", VARIANTS)
def test_subnormal_keys_and_values_attention_seq(variant):
    """MFMA 16x16x16 (the P . V product of attention_seq; its Q . K^T is a 16x16x32): Q = randn * 1024, K and V = randn * 2e-5,
    the (7, 29, 29) self form.  The scores are O(0.02), the context an average of subnormal values, itself subnormal in half.
    Bar, from the formats: every probability is rounded to p significand bits (2^-p relative, so 2^-p max |V| on their
    average), the output to half an ulp of at most max |V| (2^-p max |V|) or half the subnormal spacing (2^-25), and the
    fp32 sums add 1e-6 max |V|."""
    h16, call = _h16(variant), _caller(variant)
    nseq, seq = 7, 29
    args, keep, reference, (Kf, Vf) = _seq_case(nseq, seq, seq, 1, "self", h16, q_scale=1024.0, kv_scale=2e-5)
    ctx = torch.full((nseq * seq, 512), float("nan"), device=DEV, dtype=h16)
    call("care_attention_seq", *args, _p(ctx), 512, nseq, 8)
    kept = reference()
    fl = lambda x: torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x) if h16 == torch.float16 else x
    flushed = reference(fl(Kf), fl(Vf))
    torch.cuda.synchronize()
    p = 8 if h16 == torch.bfloat16 else 11
    vmax = Vf.abs().max().item()
    bar = 2.0 ** -p * vmax + max(2.0 ** -p * vmax, 2.0 ** -25) + 1e-6 * vmax
    if h16 == torch.float16:
        assert (Vf.abs() < 2.0 ** -14).double().mean().item() > 0.99
        assert (kept - flushed).abs().max().item() > 10 * bar and (kept - flushed).abs().mean().item() > 10 * bar
    got = ctx.double()
    print("attention_seq [%s] subnormal K, V: |out - kept| %.3g, |out - flushed| %.3g, bar %.3g" % (
        variant, (got - kept).abs().max().item(), (got - flushed).abs().max().item(), bar))
    assert torch.isfinite(got).all()
    assert (got - kept).abs().max().item() <= bar

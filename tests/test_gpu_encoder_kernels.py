"""GPU: the small kernels at the encoder's tail and under the training step's reductions, called directly at their limits and
edges - care_concept_finish, care_concept_topk_embed, care_group_mean (csrc/rowops.hip) and both forms of care_strided_sum
(csrc/backward.hip: strided_sum_kernel and, from 64 terms on, strided_sum_tile_kernel) - against the float64 restatements of
tests/step_reference.py (pinned to torch by tests/test_step_reference_cpu.py).  Pad columns of the inputs hold NaN, outputs
carry canaries around what a call may write.  The 16-bit mirror of care_concept_topk_embed runs on both libraries.
"""
import pytest
import torch

import step_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VARIANTS = ["", "f16"]
CANARY = 7.0


def _h16(variant):
    return torch.float16 if variant else torch.bfloat16


def _caller(variant=""):
    from care_amd import _lib

    return lambda name, *a: _lib.call(name, *a, variant=variant)


def _p(t):
    return None if t is None else t.data_ptr()


def _assert_f32(got, ref, what, bar):
    err = (got.double().cpu() - ref).abs().max().item()
    print("%s: max error %.3g / %.3g" % (what, err, bar))
    assert err < bar, (what, err)


def _untouched(t):
    return float(t.float().min()) == CANARY == float(t.float().max())


# ------------------------------------------------------------------------------------------------ care_concept_finish
@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("k,lds,ldp", sr.CF_SHAPES)
def test_concept_finish(B, k, lds, ldp):
    """One wave per clip, 4 clips per workgroup (B = 1, 5, 9: a lone wave, a ragged second and third workgroup); k = 1, the
    documented limit 1024, row strides that differ from k and from one another; scores saturated on both sides."""
    scores = sr.concept_finish_case(B, k, lds)
    ref, ref_avg = sr.concept_finish(scores, k)
    preds = torch.full((B + 1, ldp), CANARY, device=DEV)
    avg = torch.full((B + 1,), CANARY, device=DEV)
    sd = scores.to(DEV)
    _caller()("care_concept_finish", _p(sd), lds, _p(preds), ldp, _p(avg), B, k)
    torch.cuda.synchronize()
    _assert_f32(preds[:B, :k], ref, "concept_finish preds B %d k %d" % (B, k), 1e-6)
    _assert_f32(avg[:B], ref_avg, "concept_finish avg B %d k %d" % (B, k), 1e-6)
    assert bool(torch.isfinite(preds).all()) and float(preds[:B].min()) >= 0.0 and float(preds[:B].max()) <= 1.0
    assert ldp == k or float(preds[:B, k:].abs().max()) == 0.0            # the columns k .. ldp - 1: exactly 0
    assert _untouched(preds[B]) and _untouched(avg[B:])


def test_concept_finish_rejects_a_short_output_row():
    from care_amd import _lib

    scores = torch.zeros(2, 16, device=DEV)
    preds = torch.full((2, 16), CANARY, device=DEV)
    avg = torch.full((2,), CANARY, device=DEV)
    with pytest.raises(_lib.CareHipError, match="EINVAL"):
        _caller()("care_concept_finish", _p(scores), 16, _p(preds), 8, _p(avg), 2, 9)
    torch.cuda.synchronize()
    assert _untouched(preds) and _untouched(avg)


# ------------------------------------------------------------------------------------------------ care_concept_topk_embed
EMB_BAR = 1e-5                       # test_concept_kernels' bar for the embedded rows


def _topk_embed(call, p, k, topk, d, h16, word=None, pos=None, gamma=None, beta=None, mirror=True):
    ldo, grp_rows, row_off = d + 4, topk + 5, 3
    labels = torch.full((sr.TOPK_B + 1, topk), -7, device=DEV, dtype=torch.int64)
    out = torch.full((sr.TOPK_B, grp_rows, ldo), CANARY, device=DEV)
    outb = torch.full((sr.TOPK_B, grp_rows, ldo), CANARY, device=DEV, dtype=h16) if mirror else None
    pd = p.to(DEV)
    call("care_concept_topk_embed", _p(pd), pd.stride(0), k, topk, _p(word), _p(pos), _p(gamma), _p(beta), 1e-12, _p(labels), _p(out),
         _p(outb), ldo, grp_rows, row_off, sr.TOPK_B, d)
    torch.cuda.synchronize()
    return labels, out, outb


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("d", [512, 2048])
@pytest.mark.parametrize("k,topk", sr.TOPK_SHAPES)
def test_concept_topk_embed(k, topk, d, variant):
    """Rank by counting over k <= 1024 values with exact ties - on a grid, straddling rank topk - 1 / topk, a row of equal
    values (labels 0 .. topk - 1) - at the documented limits k = 1024 and topk = 64 and at topk = k; the embedded rows at
    out_row_off inside groups of out_grp_rows rows, a row stride of d + 4, with the 16-bit mirror."""
    h16, call = _h16(variant), _caller(variant)
    p = sr.concept_topk_case(k, topk, k + 4)
    g = sr.gen(k + d)
    word, pos = torch.randn(k, d, generator=g), torch.randn(topk, d, generator=g)
    gamma, beta = torch.randn(d, generator=g) + 1.0, torch.randn(d, generator=g)
    ref_lab = sr.concept_topk(p, k, topk)
    ref = sr.concept_embed(ref_lab, word, pos, gamma, beta, 1e-12)
    labels, out, outb = _topk_embed(call, p, k, topk, d, h16, word.to(DEV), pos.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert torch.equal(labels[: sr.TOPK_B].cpu(), ref_lab) and int(labels[sr.TOPK_B].max()) == -7
    assert labels[2].tolist() == list(range(topk))
    _assert_f32(out[:, 3:3 + topk, :d], ref, "concept_topk_embed k %d topk %d d %d [%s]" % (k, topk, d, variant), EMB_BAR)
    for o in (out, outb):
        assert _untouched(o[:, :3]) and _untouched(o[:, 3 + topk:]) and _untouched(o[:, :, d:])
    # the mirror is the fp32 row rounded once
    assert torch.equal(outb[:, 3:3 + topk, :d].contiguous().view(torch.int16), out[:, 3:3 + topk, :d].to(h16).view(torch.int16))
    # labels only (word == NULL): the same labels, nothing else written
    lab2, out2, _ = _topk_embed(call, p, k, topk, d, h16, mirror=False)
    assert torch.equal(lab2, labels) and _untouched(out2)


def test_concept_topk_embed_rejected_arguments():
    from care_amd import _lib

    p = torch.rand(sr.TOPK_B, 1100)
    w = torch.zeros(1100, 512, device=DEV)
    for what, match, k, topk, word, pos in (("k 1025", "ESHAPE", 1025, 30, w, w), ("topk 65", "ESHAPE", 1024, 65, w, w),
                                            ("topk > k", "ESHAPE", 20, 30, w, w), ("word without pos", "EINVAL", 500, 30, w, None)):
        ldo, labels = 516, None
        with pytest.raises(_lib.CareHipError, match=match):
            pd = p.to(DEV)
            labels = torch.full((sr.TOPK_B, topk), -7, device=DEV, dtype=torch.int64)
            out = torch.full((sr.TOPK_B, topk, ldo), CANARY, device=DEV)
            _caller()("care_concept_topk_embed", _p(pd), 1100, k, topk, _p(word), _p(pos), _p(w), _p(w), 1e-12, _p(labels), _p(out), None,
                      ldo, topk, 0, sr.TOPK_B, 512)
        torch.cuda.synchronize()
        assert int(labels.max()) == -7 and _untouched(out), what
        print("rejected: concept_topk_embed,", what)


# ------------------------------------------------------------------------------------------------ care_group_mean
@pytest.mark.parametrize("d", [4, 516])
@pytest.mark.parametrize("grp", [1, 28])
@pytest.mark.parametrize("groups", [1, 3])
def test_group_mean(groups, grp, d):
    """A thread per (group, float4 column): 1 .. 387 threads (no multiple of 256); the group's rows start in_row_off = 3 rows
    into a block of grp + 5 (the rows around them NaN), the means land in columns d .. 2 d - 1 of a 3 d wide output."""
    in_grp_rows, off, ldx = grp + 5, 3, d + 4
    g = sr.gen(groups + 10 * grp + d)
    x = torch.full((groups * in_grp_rows, ldx), float("nan"))
    for gi in range(groups):
        x[gi * in_grp_rows + off: gi * in_grp_rows + off + grp, :d] = torch.randn(grp, d, generator=g)
    out = torch.full((groups + 1, 3 * d), CANARY, device=DEV)
    xd = x.to(DEV)
    _caller()("care_group_mean", _p(xd), ldx, in_grp_rows, off, grp, _p(out), 3 * d, d, groups, d)
    torch.cuda.synchronize()
    _assert_f32(out[:groups, d:2 * d], sr.group_mean(x, in_grp_rows, off, grp, groups, d), "group_mean %d x %d x %d" % (groups, grp, d), 1e-6)
    assert _untouched(out[:, :d]) and _untouched(out[:, 2 * d:]) and _untouched(out[groups])


# ------------------------------------------------------------------------------------------------ care_strided_sum
@pytest.mark.parametrize("mode", sr.SS_MODES)
@pytest.mark.parametrize("terms", sr.SS_TERMS, ids=lambda t: "terms%d-%s" % (t, "strided_sum_tile_kernel" if t >= 64 else "strided_sum_kernel"))
def test_strided_sum(terms, mode):
    """out[r] = scale * sum_k x[r * row_stride + k * term_stride] in both forms: the thread-per-element kernel (terms < 64) and
    strided_sum_tile_kernel (16 waves take the terms 16 apart, two chains each, a tail: terms around 64, 80 and 96; a ragged
    last tile of 64 columns: d = 1, 63, 65, 500).  Inputs +-U[0.5, 1.5]: a dropped or doubled term is at least 0.5 (x scale)."""
    call = _caller()
    worst = 0.0
    for d in sr.SS_D:
        ldx, ldo = d + 4, d + 3
        x = sr.strided_sum_case(3 * terms, ldx, d)
        xd = x.to(DEV)
        for rows in sr.SS_ROWS:
            rs, ts, n = sr.strided_sum_strides(mode, rows, terms)
            for scale in sr.SS_SCALES:
                ref, mag = sr.strided_sum(x[:n], rows, d, terms, rs, ts, scale)
                outs = []
                for _ in range(2):
                    out = torch.full((rows + 1, ldo), CANARY, device=DEV)
                    call("care_strided_sum", _p(xd), ldx, _p(out), ldo, rows, d, terms, rs, ts, scale)
                    outs.append(out)
                torch.cuda.synchronize()
                out = outs[0]
                assert torch.equal(out.view(torch.int32), outs[1].view(torch.int32))          # the same bits every run
                assert _untouched(out[:, d:]) and _untouched(out[rows])
                err = (out[:rows, :d].double().cpu() - ref).abs()
                bar = sr.strided_sum_bar(terms, scale, mag)
                share = (err / bar).max().item()
                worst = max(worst, share)
                assert bool((err <= bar).all()), (d, rows, scale, err.max().item(), share)
    print("strided_sum terms %d %s: worst error / (terms 2^-24 scale sum|x|) = %.3g" % (terms, mode, worst))

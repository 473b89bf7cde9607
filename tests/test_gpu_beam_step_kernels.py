"""GPU: the kernels a beam step of the multi-launch search goes through, called directly - care_attention and care_embed_ln
through an ancestor table, care_ensemble_select - against the float64 restatements of tests/step_reference.py (pinned to torch
by tests/test_step_reference_cpu.py), and against the second route the code offers to the same arithmetic, bit for bit.

Instantiations of csrc/attention.hip that no other test launches, each named in a test id below:
  attention_row_kernel<NK4 = 1..8, ANC>  and  <NK4 = 3, 5, noANC>;
  attention_kernel<f32 | h16, NKB in {1, 2, 3, 4, 13, 16}, ANC | noANC, EXTRA | plain>.
csrc/beam.hip: ensemble_select_kernel (and beam_select_kernel, the two-pass form it shares its arithmetic with).

Every shape is tiny.  Poison (NaN) lives in valid memory - a cache row of its own, the cache positions past nkeys, pad columns -
so a kernel that took a wrong row or one key too many shows NaN instead of faulting.  Where a 16-bit type is involved the
test runs on both libraries ("" = bfloat16, "f16" = IEEE half).
"""
import ctypes

import pytest
import torch

import step_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VARIANTS = ["", "f16"]
CANARY = 7.0


def _h16(variant):
    return torch.float16 if variant else torch.bfloat16


def _caller(variant):
    from care_amd import _lib

    return lambda name, *a: _lib.call(name, *a, variant=variant)


def _p(t):
    return None if t is None else t.data_ptr()


def _assert_f32(got, ref, what, bar):
    err = (got.double().cpu() - ref).abs().max().item()
    print("%s: max error %.3g / %.3g" % (what, err, bar))
    assert err < bar, (what, err)


def _assert_h16(got, ref, h16, what, bar32):
    """|got - ref| <= half an ulp of h16 at ref + the fp32 bar, elementwise."""
    assert got.dtype == h16
    err = (got.double().cpu() - ref).abs()
    over = (err - sr.half_ulp(ref, h16) - bar32).max().item()
    print("%s: max error %.3g, worst excess over half-ulp + %.3g: %.3g" % (what, err.max().item(), bar32, over))
    assert over <= 0, (what, over)


# ------------------------------------------------------------------------------------------------ care_attention
ATT_BAR = 2e-5                       # test_attention's bar for this kernel (fp32 arithmetic on the rounded cache)
EXTRAS = {"mask": (True, False), "mask+bias": (True, True), "plain": (False, False)}
_att = {}


def _att_case(form, nkeys, h16):
    """The case, its device copies and the materialised (anc == NULL) layout - built once per (form, nkeys, 16-bit type)."""
    key = (form, nkeys, h16 if sr.ATT_FORMS[form][0] else None)
    if key not in _att:
        c = sr.attention_case(form, nkeys, h16)
        dense, dtok = sr.materialise(c["cache"], c["tok"], c["anc"], nkeys)
        c["dev"] = {k: c[k].to(DEV) for k in ("q", "cache", "anc", "tok", "bias")}
        c["dev"].update(dense=dense.to(DEV), dtok=dtok.to(DEV))
        c["ref"] = {}
        _att[key] = c
    return _att[key]


def _att_ref(c, extra):
    if extra not in c["ref"]:
        c["ref"][extra] = sr.attention_case_ref(c, *EXTRAS[extra])
    return c["ref"][extra]


def _attention(call, c, extra, ctx_dtype, anc=True, nkeys=None, causal=0, causal_off=0):
    """One care_attention call on the case's ancestor layout (anc) or on its materialised dense layout; ctx [16, d + 8] comes
    back whole, canaries and all."""
    dv, d, T = c["dev"], c["d"], c["T"]
    mask, with_bias = EXTRAS[extra]
    cache, tok = (dv["cache"], dv["tok"]) if anc else (dv["dense"], dv["dtok"])
    ctx = torch.full((sr.ATT_ROWS + 1, d + 8), CANARY, device=DEV, dtype=ctx_dtype)
    call("care_attention", _p(dv["q"]), dv["q"].stride(0), _p(cache), _p(cache[:, :, d:]), int(cache.dtype != torch.float32),
         T * 2 * d, 2 * d, 1, _p(dv["anc"]) if anc else None, dv["anc"].stride(0) if anc else 0,
         c["nkeys"] if nkeys is None else nkeys, causal, 1, causal_off, _p(tok) if mask else None, tok.stride(0), sr.PAD,
         _p(dv["bias"]) if with_bias else None, dv["bias"].stride(0), _p(ctx), ctx.stride(0), int(ctx_dtype != torch.float32),
         sr.ATT_ROWS, c["heads"])
    torch.cuda.synchronize()
    return ctx


def _check_ctx(ctx, ref, d, what):
    out = ctx[: sr.ATT_ROWS, :d]
    assert bool(torch.isfinite(out.float()).all()), what + ": poison leaked"
    assert float(ctx[:, d:].float().min()) == CANARY == float(ctx[:, d:].float().max()), what + ": wrote past column d"
    assert float(ctx[sr.ATT_ROWS].float().min()) == CANARY == float(ctx[sr.ATT_ROWS].float().max()), what + ": wrote past the rows"
    if ctx.dtype == torch.float32:
        _assert_f32(out, ref, what, ATT_BAR)
    else:
        _assert_h16(out, ref, ctx.dtype, what, ATT_BAR)


def _ctx_types(form, variant):
    """fp32 and the library's 16-bit type; the fp32 cache with an fp32 context involves no 16-bit type: bf16 library only."""
    return [t for t in (torch.float32, _h16(variant)) if not (form == "a" and variant and t == torch.float32)]


def _att_id(anc):
    return lambda v: "%s-nkeys%d-%s" % (v[0], v[1], sr.attention_kernel_name(v[0], v[1], anc))


ATT_ANC_CASES = ([(f, n) for f in sr.ATT_FORMS for n in sr.ATT_NKEYS] + [(f, n) for f in ("a", "b") for n in sr.ATT_NKEYS_LONG])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("extra", list(EXTRAS))
@pytest.mark.parametrize("case", ATT_ANC_CASES, ids=_att_id(True))
def test_attention_ancestors(case, extra, variant):
    """care_attention through an ancestor table (the self-attention of a beam step, engine_decode._decode_step): key j of row r
    and its pad token come from cache row anc[r, j].  Forms: a fp32 cache; b 16-bit cache, 8 heads (row kernel up to 32 keys);
    c 16-bit, 16 heads and d Q's row stride d + 4 (generic 16-bit kernel).  `plain` = neither mask nor bias (EXTRA = false).
    Against float64 on the rounded cache; bit-identical to the anc == NULL call on the materialised cache and token table."""
    form, nkeys = case
    call = _caller(variant)
    c = _att_case(form, nkeys, _h16(variant))
    ref = _att_ref(c, extra)
    for ctx_dtype in _ctx_types(form, variant):
        what = "attention %s [%s] %s ctx %s" % (_att_id(True)(case), variant, extra, str(ctx_dtype)[6:])
        ctx = _attention(call, c, extra, ctx_dtype)
        _check_ctx(ctx, ref, c["d"], what)
        dense = _attention(call, c, extra, ctx_dtype, anc=False)
        assert torch.equal(ctx.view(torch.int32 if ctx_dtype == torch.float32 else torch.int16),
                           dense.view(torch.int32 if ctx_dtype == torch.float32 else torch.int16)), what + ": anc != dense"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("extra", ["mask+bias", "plain"])
@pytest.mark.parametrize("case", [(f, n) for f in ("a", "b", "c") for n in sr.ATT_NKEYS_PLAIN], ids=_att_id(False))
def test_attention_without_ancestors(case, extra, variant):
    """The anc == NULL instantiations no other test launches (key counts 12, 20, 100, 128), on the materialised layout."""
    form, nkeys = case
    c = _att_case(form, nkeys, _h16(variant))
    for ctx_dtype in _ctx_types(form, variant):
        ctx = _attention(_caller(variant), c, extra, ctx_dtype, anc=False)
        _check_ctx(ctx, _att_ref(c, extra), c["d"], "attention %s [%s] %s ctx %s" % (_att_id(False)(case), variant, extra, str(ctx_dtype)[6:]))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("form", ["a", "b", "d"])
@pytest.mark.parametrize("t", [1, 6, 13, 32])
def test_attention_causal_off_of_a_decode_step(t, form, variant):
    """seq = 1, causal = 1, causal_off = t - 1 over a 32-key cache sees min(32, 0 + 1 + t - 1) = t keys: the bits of the
    non-causal call at nkeys = t (the keys past t are the cache's NaN positions and ancestors of the poison row)."""
    call = _caller(variant)
    c = _att_case(form, t, _h16(variant))
    for ctx_dtype in _ctx_types(form, variant):
        a = _attention(call, c, "mask+bias", ctx_dtype, nkeys=32, causal=1, causal_off=t - 1)
        b = _attention(call, c, "mask+bias", ctx_dtype)
        _check_ctx(a, _att_ref(c, "mask+bias"), c["d"], "attention causal_off %d form %s [%s]" % (t - 1, form, variant))
        assert torch.equal(a.float(), b.float())


# ------------------------------------------------------------------------------------------------ care_embed_ln
EMB_BAR = 1e-5                       # test_add_ln_group_mean_embed's bar, the same O(1) inputs
_emb = {}


def _emb_case(d, seq):
    if (d, seq) not in _emb:
        c = sr.embed_case(d, seq)
        c["dev"] = {k: c[k].to(DEV) for k in ("tok", "anc", "word", "pos", "sem", "gamma", "beta")}
        c["dev"]["gathered"] = sr.gather_tokens(c["tok"], c["anc"]).to(DEV)
        _emb[(d, seq)] = c
    return _emb[(d, seq)]


def _embed(call, c, tok_off, seq, with_sem, anc, h16, mirror=True):
    dv, d = c["dev"], c["d"]
    out = torch.full((sr.EMB_ROWS + 1, d + 4), CANARY, device=DEV)
    outb = torch.full((sr.EMB_ROWS + 1, d + 4), CANARY, device=DEV, dtype=h16) if mirror else None
    tok = dv["tok"] if anc else dv["gathered"]
    call("care_embed_ln", _p(tok), tok.stride(0), tok_off, _p(dv["anc"]) if anc else None, dv["anc"].stride(0) if anc else 0,
         _p(dv["word"]), _p(dv["pos"]), tok_off, _p(dv["sem"]) if with_sem else None, 5, _p(dv["gamma"]), _p(dv["beta"]), 1e-12,
         _p(out), _p(outb), out.stride(0), sr.EMB_ROWS, seq, d)
    torch.cuda.synchronize()
    return out, outb


def _check_embed(call, c, tok_off, seq, with_sem, h16, what):
    d = c["d"]
    ref = sr.embed_ln_anc(c["tok"], tok_off, c["anc"], c["word"], c["pos"], tok_off, c["sem"] if with_sem else None, 5, c["gamma"],
                          c["beta"], 1e-12, sr.EMB_ROWS, seq)
    out, outb = _embed(call, c, tok_off, seq, with_sem, True, h16)
    _assert_f32(out[: sr.EMB_ROWS, :d], ref, what, EMB_BAR)
    for o in (out, outb):
        assert float(o[:, d:].float().min()) == CANARY == float(o[:, d:].float().max())
        assert float(o[sr.EMB_ROWS].float().min()) == CANARY == float(o[sr.EMB_ROWS].float().max())
    # the mirror is the fp32 row rounded once
    assert torch.equal(outb[: sr.EMB_ROWS, :d].view(torch.int16), out[: sr.EMB_ROWS, :d].to(h16).view(torch.int16))
    plain, plainb = _embed(call, c, tok_off, seq, with_sem, False, h16)
    assert torch.equal(out, plain) and torch.equal(outb.view(torch.int16), plainb.view(torch.int16)), what + ": anc != gathered"
    alone, _ = _embed(call, c, tok_off, seq, with_sem, True, h16, mirror=False)
    assert torch.equal(out, alone)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("with_sem", [True, False], ids=["sem", "nosem"])
@pytest.mark.parametrize("t", [1, 7, 30])
@pytest.mark.parametrize("d", [512, 768, 1024, 2048])
def test_embed_ln_ancestors(d, t, with_sem, variant):
    """care_embed_ln of a beam step: 15 rows, seq = 1, tok_off = pos0 = t - 1, the token of row r from row anc[r, t - 1] of a
    [15, 31] table (ancestor stride 33), a semantic row per clip of 5 beams or none; output rows d + 4 apart."""
    _check_embed(_caller(variant), _emb_case(d, 1), t - 1, 1, with_sem, _h16(variant), "embed_ln d %d t %d [%s]" % (d, t, variant))


@pytest.mark.parametrize("variant", VARIANTS)
def test_embed_ln_ancestors_teacher_forced(variant):
    """seq = 5: row r is position 2 + r % 5 of sequence r / 5, its token from row anc[r / 5, 2 + r % 5]."""
    _check_embed(_caller(variant), _emb_case(512, 5), 2, 5, True, _h16(variant), "embed_ln seq 5 [%s]" % variant)


# ------------------------------------------------------------------------------------------------ care_ensemble_select
def _ensemble(members, ld, V, bm, rows=sr.ENS_ROWS, n_models=None, null_member=None):
    """ensemble_select_kernel on device copies of `members`; cand_val / cand_idx [rows + 1, bm] come back whole."""
    from care_amd import _lib

    dev = [m.to(DEV) for m in members]
    ptrs = [m.data_ptr() for m in dev]
    if null_member is not None:
        ptrs[null_member] = None
    arr = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    cv = torch.full((rows + 1, bm), CANARY, device=DEV)
    ci = torch.full((rows + 1, bm), -7, device=DEV, dtype=torch.int32)
    _lib.call("care_ensemble_select", arr, len(dev) if n_models is None else n_models, ld, V, bm, _p(cv), _p(ci), rows)
    torch.cuda.synchronize()
    return cv, ci


def _check_ensemble(members, ld, V, bm, what):
    val, idx, mag = sr.ensemble_select(members, V, bm)
    cv, ci = _ensemble(members, ld, V, bm)
    assert float(cv[sr.ENS_ROWS].min()) == CANARY and int(ci[sr.ENS_ROWS].max()) == -7
    cv, ci = cv[: sr.ENS_ROWS].cpu(), ci[: sr.ENS_ROWS].cpu()
    assert torch.equal(ci, idx), (what, ci, idx)
    fin = torch.isfinite(val)
    assert torch.equal(torch.isfinite(cv), fin) and bool((cv[~fin] == float("-inf")).all())
    over = ((cv.double() - val).abs() - sr.ensemble_value_bar(mag))[fin]
    err = (cv.double() - val).abs()[fin].max().item()
    print("%s: max error %.3g, worst share of the bar %.3g" % (what, err, (1 + over / sr.ensemble_value_bar(mag)[fin]).max().item()))
    assert over.max().item() <= 0, (what, over.max().item())


@pytest.mark.parametrize("V,ld,n_models,bm", sr.ensemble_cases())
def test_ensemble_select(V, ld, n_models, bm):
    """ensemble_select_kernel: the bm best columns of the members' log_softmax rows averaged, NaN in the pad columns; the top
    bm + 1 averages are 0.25 apart (tests/test_step_reference_cpu.py, every case), so the indices must be the reference's."""
    members, _ = sr.ensemble_case(V, ld, n_models, bm)
    _check_ensemble(members, ld, V, bm, "ensemble V %d members %d bm %d" % (V, n_models, bm))


@pytest.mark.parametrize("n_models", [1, 3])
@pytest.mark.parametrize("V,ld", [(1029, 1032), (10547, 10560)])
def test_ensemble_select_exact_ties_come_out_column_ascending(V, ld, n_models):
    """Columns equal in every member have bit-equal averages: inside one thread's stride of 256 (rows 0, 3), in neighbouring
    threads (1, 4), in different waves (2, 5) - on top of the order, and across its end (the bm-th and bm + 1-th best)."""
    bm = 5
    members, planted = sr.ensemble_case(V, ld, n_models, bm)
    pairs = [(10, 10 + 256), (700, 701), (5, 5 + 64)]
    for r in range(sr.ENS_ROWS):
        a, b = pairs[r % 3]
        for m in members:
            if r < 3:
                m[r, a] = m[r, b] = 13.0                      # the two best
            else:
                m[r, planted[r]] = -20.0                      # take the planted ladder away ...
                m[r, a] = m[r, b] = 10.5                      # ... the pair ties for ranks bm - 1 and bm
                m[r, [20, 300, 600, 900][: bm - 1]] = torch.tensor([14.0, 13.5, 13.0, 12.5])
    val, idx, _ = sr.ensemble_select(members, V, bm)
    for r in range(sr.ENS_ROWS):
        a, b = pairs[r % 3]
        assert idx[r, :2].tolist() == [a, b] if r < 3 else (idx[r, bm - 1] == a and b not in idx[r].tolist())
    _check_ensemble(members, ld, V, bm, "ensemble ties V %d members %d" % (V, n_models))


def test_ensemble_select_minus_infinity():
    """A column that is -inf in one member averages to -inf and is never selected; fewer than bm finite averages: the tail is
    (-inf, 0), as care_beam_select documents."""
    members, planted = sr.ensemble_case(300, 301, 3, 5)
    for r in range(sr.ENS_ROWS):
        members[r % 3][r, planted[r, 0]] = float("-inf")       # the best column of the row
        members[1][r, [c for c in range(7, 40) if c not in planted[r].tolist()]] = float("-inf")
    _check_ensemble(members, 301, 300, 5, "ensemble -inf V 300")
    members, _ = sr.ensemble_case(5, 8, 2, 5)
    members[1][:, 1] = members[0][:, 4] = float("-inf")
    _check_ensemble(members, 8, 5, 5, "ensemble -inf tail V 5")


@pytest.mark.parametrize("V,ld,bm", [(300, 301, 5), (17, 19, 8), (1029, 1030, 1)])
def test_ensemble_of_one_is_beam_select(V, ld, bm):
    """n_models = 1 on a row stride that is no multiple of 4 - care_beam_select takes beam_select_kernel there, the two-pass
    kernel ensemble_select_kernel shares its arithmetic with: identical bits."""
    from care_amd import _lib

    members, _ = sr.ensemble_case(V, ld, 1, bm)
    members[0][2, 3] = float("-inf")
    cv, ci = _ensemble(members, ld, V, bm)
    x = members[0].to(DEV)
    bv = torch.full_like(cv, CANARY)
    bi = torch.full_like(ci, -7)
    _lib.call("care_beam_select", _p(x), ld, V, bm, _p(bv), _p(bi), sr.ENS_ROWS, 1)
    torch.cuda.synchronize()
    assert torch.equal(cv.view(torch.int32), bv.view(torch.int32)) and torch.equal(ci, bi)


# ------------------------------------------------------------------------------------------------ rejected arguments
def test_rejected_arguments_leave_the_outputs_alone():
    from care_amd import _lib

    members, _ = sr.ensemble_case(17, 20, 8, 5)

    def ens(what, match, m=members[:2], ld=20, V=17, bm=5, **kw):
        with pytest.raises(_lib.CareHipError, match=match):
            _ensemble(m, ld, V, bm, **kw)
        print("rejected: ensemble,", what)

    ens("no member", "EINVAL", m=[], n_models=0)
    ens("9 members", "ESHAPE", m=members + members[:1])
    ens("a NULL member", "EINVAL", null_member=1)
    ens("bm 9", "ESHAPE", bm=9)
    ens("bm > V", "ESHAPE", m=[x[:, :8].contiguous() for x in members[:2]], ld=8, V=4, bm=5)
    ens("ldl < V", "EINVAL", ld=16)
    # (the outputs of a rejected call: _ensemble raised before returning them - one more call that keeps them)
    dev = [m.to(DEV) for m in members[:2]]
    arr = (ctypes.c_void_p * 2)(*[m.data_ptr() for m in dev])
    cv = torch.full((6, 5), CANARY, device=DEV)
    ci = torch.full((6, 5), -7, device=DEV, dtype=torch.int32)
    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        _lib.call("care_ensemble_select", arr, 2, 20, 17, 9, _p(cv), _p(ci), 6)
    torch.cuda.synchronize()
    assert float(cv.min()) == CANARY == float(cv.max()) and int(ci.max()) == -7 == int(ci.min())

    d, rows = 512, 4
    q = torch.zeros(rows, d + 8, device=DEV)
    kv = torch.zeros(rows, 130, 2 * d, device=DEV)
    ctx = torch.full((rows, d), CANARY, device=DEV)

    def att(nkeys, ldq):
        _lib.call("care_attention", _p(q), ldq, _p(kv), _p(kv[:, :, d:]), 0, 130 * 2 * d, 2 * d, 1, None, 0, nkeys, 0, 1, 0, None, 0, 0,
                  None, 0, _p(ctx), d, 0, rows, 8)

    with pytest.raises(_lib.CareHipError, match="ESHAPE"):
        att(129, d)
    with pytest.raises(_lib.CareHipError, match="EALIGN"):
        att(16, d + 2)
    torch.cuda.synchronize()
    assert float(ctx.min()) == CANARY == float(ctx.max())
    att(128, d + 4)                                            # the limits themselves are accepted
    torch.cuda.synchronize()
    assert float(ctx.abs().max()) == 0.0

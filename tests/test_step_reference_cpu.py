"""tests/step_reference.py (the yardstick of tests/test_gpu_beam_step_kernels.py and tests/test_gpu_encoder_kernels.py) against
torch, and every input builder of those tests against the condition it states - on every parametrised case, all on the CPU."""
import pytest
import torch

import step_reference as sr

H16 = [torch.bfloat16, torch.float16]


# ---------------------------------------------------------------------------------------------- restatements == torch
def _torch_attention(q, K, V, tok, bias, heads, dtype=torch.float64):
    """softmax(masked_fill(Q K^T / 8, -1e9) + bias) V for rows that own one cache block each (identity ancestors)."""
    rows, nk = q.shape[0], K.shape[1]
    qh = q.to(dtype).view(rows, heads, 1, 64)
    k = K.to(dtype).view(rows, nk, heads, 64).permute(0, 2, 1, 3)
    v = V.to(dtype).view(rows, nk, heads, 64).permute(0, 2, 1, 3)
    s = qh @ k.transpose(-1, -2) / 8.0
    if tok is not None:
        s = s.masked_fill(tok[:, :nk].eq(sr.PAD).view(rows, 1, 1, nk), -1e9)
    if bias is not None:
        s = s + bias[:, :nk].to(dtype).view(1, heads, 1, nk)
    return (torch.softmax(s.double(), -1) @ v.double()).permute(0, 2, 1, 3).reshape(rows, heads * 64)


@pytest.mark.parametrize("mask,with_bias", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("nkeys", [1, 5, 32, 100])
def test_attention_with_identity_ancestors_equals_torch(nkeys, mask, with_bias):
    g = sr.gen(nkeys)
    rows, heads, d = 6, 8, 512
    q = torch.randn(rows, d, generator=g)
    K, V = torch.randn(rows, nkeys, d, generator=g), torch.randn(rows, nkeys, d, generator=g)
    tok = torch.randint(0, 3, (rows, nkeys), generator=g, dtype=torch.int32)
    tok[2] = sr.PAD                                            # a row with every key padded
    bias = torch.randn(heads, nkeys + 2, generator=g)
    t, b = (tok if mask else None), (bias if with_bias else None)
    got = sr.attention_anc(q, K, V, sr.identity_anc(rows, nkeys), nkeys, heads, tok=t, bias=b)
    ref = _torch_attention(q, K, V, t, b, heads)
    allpad = tok.eq(sr.PAD).all(1) if mask else torch.zeros(rows, dtype=torch.bool)
    assert bool(allpad[2]) == mask
    assert (got - ref)[~allpad].abs().max().item() < 1e-12
    if mask:
        # every key padded: the model's fp32 scores are -1e9 + bias = -1e9 exactly - uniform probabilities, the mean of V
        ref32 = _torch_attention(q, K, V, t, b, heads, dtype=torch.float32)
        assert (got - ref32)[allpad].abs().max().item() < 1e-5
        assert (got[allpad] - V.double().mean(1)[allpad]).abs().max().item() < 1e-12


def test_attention_causal_key_count_and_rows_per_kv():
    g = sr.gen(3)
    seq, heads, nkeys = 5, 8, 9
    rows = 2 * seq
    q = torch.randn(rows, 512, generator=g)
    K, V = torch.randn(2, nkeys, 512, generator=g), torch.randn(2, nkeys, 512, generator=g)
    anc = sr.identity_anc(rows, nkeys, rows_per_kv=seq)
    for off in (0, 2, 20):
        got = sr.attention_anc(q, K, V, anc, nkeys, heads, causal=True, seq=seq, causal_off=off)
        for r in range(rows):
            nk = min(nkeys, r % seq + 1 + off)
            one = _torch_attention(q[r:r + 1], K[r // seq:r // seq + 1, :nk], V[r // seq:r // seq + 1, :nk], None, None, heads)
            assert (got[r] - one[0]).abs().max().item() < 1e-12


def test_materialise_is_the_ancestor_gather():
    case = sr.attention_case("a", 13, None)
    dense, dtok = sr.materialise(case["cache"], case["tok"], case["anc"], 13)
    d = case["d"]
    a = sr.attention_case_ref(case, True, True)
    b = sr.attention_anc(case["q"][:, :d], dense[:, :, :d], dense[:, :, d:], sr.identity_anc(sr.ATT_ROWS, 13), 13, 8, tok=dtok,
                         bias=case["bias"])
    assert torch.equal(a, b) and bool(torch.isnan(dense[:, 13:]).all()) and torch.isfinite(dense[:, :13]).all()


@pytest.mark.parametrize("V,ld,n_models,bm", [(17, 20, 3, 5), (300, 301, 1, 8), (1029, 1032, 8, 1)])
def test_ensemble_equals_stack_mean_and_a_stable_sort(V, ld, n_models, bm):
    members, _ = sr.ensemble_case(V, ld, n_models, bm)
    members[0][1, 3] = members[0][1, 9] = 13.0                 # an exact tie in the average when n_models == 1 ...
    for m in members[1:]:
        m[1, 3] = m[1, 9] = 13.0                               # ... and when every member agrees
    val, idx, _ = sr.ensemble_select(members, V, bm)
    avg = torch.stack([torch.log_softmax(m[:, :V].double(), 1) for m in members]).mean(0)
    order = torch.sort(avg, dim=1, descending=True, stable=True)[1][:, :bm]
    assert torch.equal(idx.long(), order)
    assert (val - avg.gather(1, order)).abs().max().item() < 1e-12
    assert idx[1, 0] == 3 and (bm == 1 or idx[1, 1] == 9)


def test_ensemble_minus_infinity_tail():
    members, _ = sr.ensemble_case(5, 8, 2, 5)
    members[1][:, 1] = members[0][:, 4] = float("-inf")
    val, idx, _ = sr.ensemble_select(members, 5, 5)
    assert torch.isinf(val[:, 3:]).all() and torch.isfinite(val[:, :3]).all() and int(idx[:, 3:].abs().max()) == 0
    assert not ((idx[:, :3] == 1) | (idx[:, :3] == 4)).any()


@pytest.mark.parametrize("k,topk", sr.TOPK_SHAPES)
def test_concept_topk_equals_torch_topk_on_tie_free_input(k, topk):
    p = torch.randperm(k, generator=sr.gen(k + topk)).float().view(1, k) / k
    assert torch.equal(sr.concept_topk(p, k, topk), torch.topk(p, topk, dim=1)[1])
    word, pos = torch.randn(k, 64, generator=sr.gen(1)), torch.randn(topk, 64, generator=sr.gen(2))
    g, b = torch.randn(64, generator=sr.gen(3)), torch.randn(64, generator=sr.gen(4))
    lab = sr.concept_topk(p, k, topk)
    ref = torch.nn.functional.layer_norm(word[lab].double() + pos.double().unsqueeze(0), (64,), g.double(), b.double(), 1e-12)
    assert (sr.concept_embed(lab, word, pos, g, b, 1e-12) - ref).abs().max().item() < 1e-12


def test_concept_finish_is_the_literal_formula():
    s = sr.concept_finish_case(5, 500, 512)
    preds, avg = sr.concept_finish(s, 500)
    x = s[:, :500].double()
    p = 1.0 / (1.0 + torch.exp(-x))
    lit = 1.0 - torch.exp(torch.log(torch.clamp(1.0 - p, 1e-12, 1.0)))
    assert (preds - lit).abs().max().item() < 1e-15 and (avg - p.mean(1)).abs().max().item() < 1e-15
    assert preds.min().item() >= 0.0 and preds.max().item() <= 1.0


def test_embed_layer_norm_group_mean_strided_sum_equal_torch():
    c = sr.embed_case(512, 1)
    t = 7
    got = sr.embed_ln_anc(c["tok"], t - 1, sr.identity_anc(15, 33), c["word"], c["pos"], t - 1, c["sem"], 5, c["gamma"], c["beta"],
                          1e-12, 15, 1)
    x = c["word"][c["tok"][:, t - 1].long()].double() + c["pos"][t - 1].double() + c["sem"].double().repeat_interleave(5, 0)
    ref = torch.nn.functional.layer_norm(x, (512,), c["gamma"].double(), c["beta"].double(), 1e-12)
    assert (got - ref).abs().max().item() < 1e-12
    assert torch.equal(got, sr.embed_ln_anc(c["tok"], t - 1, None, c["word"], c["pos"], t - 1, c["sem"], 5, c["gamma"], c["beta"],
                                            1e-12, 15, 1))
    # ancestors: the same as the plain form on the gathered token rows, for seq 1 and a teacher-forced seq 5
    for seq, off in ((1, 6), (5, 2)):
        c = sr.embed_case(512, seq)
        a = sr.embed_ln_anc(c["tok"], off, c["anc"], c["word"], c["pos"], off, c["sem"], 5, c["gamma"], c["beta"], 1e-12, 15, seq)
        b = sr.embed_ln_anc(sr.gather_tokens(c["tok"], c["anc"]), off, None, c["word"], c["pos"], off, c["sem"], 5, c["gamma"],
                            c["beta"], 1e-12, 15, seq)
        assert torch.equal(a, b)
        assert not torch.equal(sr.gather_tokens(c["tok"], c["anc"]), c["tok"][: 15 // seq])   # the table matters
    x = torch.randn(2 * 40, 20, generator=sr.gen(5))
    ref = x.double().view(2, 40, 20)[:, 3:31, :16].mean(1)
    assert (sr.group_mean(x, 40, 3, 28, 2, 16) - ref).abs().max().item() < 1e-14
    x = sr.strided_sum_case(3 * 65, 12, 9)
    for mode in sr.SS_MODES:
        rs, ts, n = sr.strided_sum_strides(mode, 3, 65)
        got, mag = sr.strided_sum(x[:n], 3, 9, 65, rs, ts, 0.25)
        for r in range(3):
            rows = [r * rs + k * ts for k in range(65)]
            assert max(rows) < n
            assert (got[r] - 0.25 * x[rows, :9].double().sum(0)).abs().max().item() < 1e-12
            assert (mag[r] - x[rows, :9].double().abs().sum(0)).abs().max().item() < 1e-12


@pytest.mark.parametrize("h16", H16)
def test_half_ulp_is_half_the_spacing(h16):
    x = torch.tensor([1.0, 1.5, 1.96875, 2.0, -3.0, 0.125, 2.0 ** -10, 96.0, 0.0], dtype=torch.float64)   # exact in both types
    up = torch.nextafter(x.abs().to(h16), torch.tensor(float("inf"), dtype=h16)).double()
    want = (up - x.abs().to(h16).double()) / 2
    want[-1] = 0.0
    assert torch.equal(sr.half_ulp(x, h16), want)
    # a correct rounding meets it, everywhere
    y = torch.randn(10000, generator=sr.gen(9), dtype=torch.float64) * 3
    assert bool(((y.to(h16).double() - y).abs() <= sr.half_ulp(y, h16)).all())


# ---------------------------------------------------------------------------------------------- builders meet their conditions
ATT_CASES = ([(f, n) for f in sr.ATT_FORMS for n in sr.ATT_NKEYS] + [(f, n) for f in ("a", "b") for n in sr.ATT_NKEYS_LONG])


@pytest.mark.parametrize("h16", H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("form,nkeys", ATT_CASES)
def test_attention_builder(form, nkeys, h16):
    """Poison where stated and in bounds; ancestors reach other clips; row 7 wholly padded; the pad mask of rows 0 and 1 (and
    of every case as a whole) differs between `by ancestor` and `by row`, and the reference output moves with it."""
    c = sr.attention_case(form, nkeys, h16)
    anc, tok, cache, T = c["anc"], c["tok"], c["cache"], c["T"]
    assert anc.shape == (15, T + 3) and tok.shape == (16, T + 1) and cache.shape == (16, T, 2 * c["d"])
    assert anc.shape[1] not in (nkeys, T) and tok.shape[1] not in (nkeys, T)
    assert int(anc.min()) >= 0 and int(anc.max()) <= 15 and bool((anc[:, nkeys:] == 15).all()) and int(anc[:, :nkeys].max()) <= 14
    assert bool(torch.isnan(cache[15].float()).all()) and bool(torch.isnan(cache[:, nkeys:].float()).all())
    assert bool(torch.isfinite(cache[:15, :nkeys].float()).all()) and bool(torch.isfinite(c["q"][:, : c["d"]]).all())
    if nkeys >= 4:
        clip = torch.arange(15).view(15, 1) // 5
        assert bool((anc[:, :nkeys] // 5 != clip).any())
    j = torch.arange(nkeys)
    by_anc = torch.stack([tok[anc[r, :nkeys].long(), j] == sr.PAD for r in range(15)])
    by_row = tok[:15, :nkeys] == sr.PAD
    assert bool(by_anc[sr.ATT_ALLPAD_ROW].all())
    assert bool(by_anc[0, 0]) and not bool(by_row[0, 0]) and not bool(by_anc[1, 0]) and bool(by_row[1, 0])
    ref = sr.attention_case_ref(c, True, False)
    wrong = sr.attention_case_ref(c, True, False, mask_by_row=True)
    assert torch.isfinite(ref).all()
    moved = (ref - wrong).abs().amax(1)
    # (nkeys == 1: a softmax over one key is 1 whatever its score - the two rules cannot differ in the output there)
    if nkeys >= 2:
        assert moved[0].item() > 1e-3 or moved[1].item() > 1e-3
        assert moved.max().item() > 1e-2


@pytest.mark.parametrize("V,ld,n_models,bm", sr.ensemble_cases())
def test_ensemble_builder_separates_the_top(V, ld, n_models, bm):
    members, planted = sr.ensemble_case(V, ld, n_models, bm)
    assert all(bool(torch.isnan(m[:, V:]).all()) and bool(torch.isfinite(m[:, :V]).all()) for m in members)
    n = min(bm + 1, V)
    avg, _ = sr.ensemble_average(members, V)
    top, idx = torch.sort(avg, dim=1, descending=True, stable=True)
    assert torch.equal(idx[:, :n], planted)                                     # every row, none left out
    gaps = top[:, : n - 1] - top[:, 1:n]
    assert n == 1 or (gaps - 0.25).abs().max().item() < 1e-9
    if n < V:
        assert (top[:, n - 1] - top[:, n]).min().item() > 0.25                  # and clear of the unplanted columns


@pytest.mark.parametrize("k,topk", sr.TOPK_SHAPES)
def test_concept_topk_builder_has_the_ties(k, topk):
    p = sr.concept_topk_case(k, topk, k + 4)
    assert bool(torch.isnan(p[:, k:]).all()) and float(p[:, :k].min()) >= 0 and float(p[:, :k].max()) <= 1
    s = torch.sort(p[:, :k].double(), dim=1, descending=True)[0]
    if topk < k:
        assert s[1, topk - 1] == s[1, topk]                                     # the tie straddles the boundary
    if topk >= 2:
        assert s[1, topk - 2] == s[1, topk - 1]
    if k > 64:
        assert len(torch.unique(p[0, :k])) <= 64 < k
    assert len(torch.unique(p[2, :k])) == 1
    assert sr.concept_topk(p, k, topk)[2].tolist() == list(range(topk))


@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("k,lds,ldp", sr.CF_SHAPES)
def test_concept_finish_builder_saturates_both_sides(B, k, lds, ldp):
    s = sr.concept_finish_case(B, k, lds)
    assert bool(torch.isnan(s[:, k:]).all()) and bool(torch.isfinite(s[:, :k]).all())
    if k >= 4:
        for b in range(B):
            assert all(bool((s[b, :k] == v).any()) for v in sr.CF_PLANTED)
    else:
        assert [float(s[b, 0]) for b in range(B)] == [sr.CF_PLANTED[b % 4] for b in range(B)]


@pytest.mark.parametrize("terms", sr.SS_TERMS)
def test_strided_sum_builder_and_bar(terms):
    x = sr.strided_sum_case(3 * terms, 504, 500)
    a = x[:, :500].abs()
    assert float(a.min()) >= 0.5 and float(a.max()) <= 1.5 and bool(torch.isnan(x[:, 500:]).all())
    for scale in sr.SS_SCALES:
        for r in range(3):
            bar = sr.strided_sum_bar(terms, scale, a[r * terms:(r + 1) * terms].double().sum(0))
            assert bar.max().item() < 0.1 * scale < 0.5 * scale                 # a dropped term is far outside the bar

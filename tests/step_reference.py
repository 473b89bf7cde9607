"""The tests' own float64 restatements of the kernels a beam step and the encoder's tail go through, written from
include/care_hip.h and the reference lines cited there, plus the input builders the CPU and the GPU tests share:

  care_attention (ancestor table, key-pad mask, bias, causal_off)   care_embed_ln (ancestor table)
  care_ensemble_select                                              care_concept_finish / care_concept_topk_embed
  care_group_mean                                                   care_strided_sum

The yardstick of tests/test_gpu_beam_step_kernels.py and tests/test_gpu_encoder_kernels.py; pinned to torch by
tests/test_step_reference_cpu.py, which also checks on every parametrised case that a builder's inputs have the property
its docstring states (a tie, a gap, a disagreement between a row and its ancestor).  Everything here is CPU tensors; no GPU.
"""
import numpy as np
import torch

PAD = 0
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- 16-bit outputs
def half_ulp(ref, h16):
    """Half the spacing of the 16-bit type h16 at every element of `ref` (float64), 0 where ref is 0: for
    2^e <= |ref| < 2^(e+1) and p significand bits (implicit one included: 8 bfloat16, 11 half) it is 2^(e-p), the largest
    error of a correct round-to-nearest (subnormals: the spacing of the lowest binade)."""
    p, emin = (8, -126) if h16 == torch.bfloat16 else (11, -14)
    e = (torch.frexp(ref)[1] - 1).clamp_min(emin).double()      # ref = m 2^(e + 1), m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.exp2(e - p))


# ---------------------------------------------------------------------------------------------- attention
def identity_anc(rows, ncols, rows_per_kv=1):
    """The ancestor table that says what `anc == NULL` says: every key of row r in block r / rows_per_kv."""
    return (torch.arange(rows) // rows_per_kv).to(torch.int32).view(rows, 1).repeat(1, ncols)


def attention_anc(q, K, V, anc, nkeys, heads, tok=None, pad_id=PAD, bias=None, causal=False, seq=1, causal_off=0, mask_by_row=False):
    """care_attention (Attention.py:83-131): q [rows, heads * 64]; K, V [blocks, T, heads * 64] (the cache as the kernel reads it,
    i.e. already rounded to its type); key j of row r is K[anc[r, j], j], and its pad token is tok[anc[r, j], j].  Per (row, head):
    q.k / 8 -> masked_fill(-1e9) -> + bias[h, j] -> softmax -> P.V over the first min(nkeys, r % seq + 1 + causal_off) keys
    (all nkeys without `causal`).  Float64 throughout, with one exception that is the reference model's own arithmetic: the
    score of a MASKED key is float32(-1e9) + float32(bias) evaluated in float32, where it is -1e9 again for every |bias| < 32
    (the spacing of float32 at 1e9 is 64).  That only shows in a row all of whose keys are padded: its probabilities are
    uniform, not softmax(bias).
    mask_by_row: the pad token taken from row r instead of from its ancestor - a deliberately wrong rule, for showing that an
    input can tell the two apart."""
    rows = q.shape[0]
    q, K, V = q.to(F64), K.to(F64), V.to(F64)
    out = torch.zeros(rows, heads * 64, dtype=F64)
    for r in range(rows):
        nk = min(nkeys, r % seq + 1 + causal_off) if causal else nkeys
        j = torch.arange(nk)
        src = anc[r, :nk].long()
        k = K[src, j].view(nk, heads, 64)
        v = V[src, j].view(nk, heads, 64)
        s = torch.einsum("he,jhe->hj", q[r].view(heads, 64), k) / 8.0
        if tok is not None:
            m = tok[torch.full_like(src, r) if mask_by_row else src, j] == pad_id
            s = s.masked_fill(m.view(1, nk), -1e9)
        if bias is not None:
            s = s + bias[:, :nk].to(F64)
            if tok is not None and bool(m.any()):
                s32 = torch.full((heads, nk), -1e9, dtype=torch.float32) + bias[:, :nk].float()
                s = torch.where(m.view(1, nk), s32.to(F64), s)
        out[r] = torch.einsum("hj,jhe->he", torch.softmax(s, -1), v).reshape(-1)
    return out


ATT_ROWS, ATT_CLIPS, ATT_BEAMS = 15, 3, 5          # 15 rows: no multiple of the 4 waves of a workgroup
ATT_POISON = ATT_ROWS                              # cache / token row 15: in bounds, never a live key
ATT_NKEYS = (1, 2, 4, 5, 8, 9, 13, 16, 17, 21, 24, 25, 29, 32)
ATT_NKEYS_LONG = (100, 128)
ATT_NKEYS_PLAIN = (12, 20, 100, 128)
ATT_ALLPAD_ROW = 7
# form -> (16-bit cache, heads, extra columns of Q's row stride)
ATT_FORMS = {"a": (False, 8, 0), "b": (True, 8, 0), "c": (True, 16, 0), "d": (True, 8, 4)}


def attention_kernel_name(form, nkeys, anc):
    """The instantiation of csrc/attention.hip a call reaches, by care_attention's dispatch (for test ids: the coverage can be
    read off the test list).  The generic kernel has an EXTRA (mask and / or bias) and a plain form of each on top."""
    c16, heads, ldq_extra = ATT_FORMS[form]
    a = "ANC" if anc else "noANC"
    if c16 and heads == 8 and nkeys <= 32 and ldq_extra % 8 == 0:
        return "attention_row_kernel<NK4=%d,%s>" % ((nkeys + 3) // 4, a)
    nkb = next(n for lim, n in ((8, 1), (16, 2), (24, 3), (32, 4), (88, 11), (104, 13), (120, 15), (128, 16)) if nkeys <= lim)
    return "attention_kernel<%s,NKB=%d,%s>" % ("h16" if c16 else "f32", nkb, a)


def attention_case(form, nkeys, h16, seed=0):
    """Inputs of an ancestor-form care_attention call over 3 clips x 5 beams.  cache [16, T, 2 d] (K | V) of fp32 (form a) or
    h16, T = 32 (128 for the long-key cases); anc int32 [15, T + 3]; tok int32 [16, T + 1]; bias fp32 [heads, T + 5];
    q fp32 [15, d + extra] (the extra columns NaN).
      * row 15 of the cache, positions >= nkeys of every cache row, the extra columns of q: NaN.  anc[:, nkeys:] = 15.
      * ancestors are uniform over the 15 live rows (other clips' rows included).
      * row 7 has every key padded: tok[anc[7, j], j] = PAD for every j < nkeys.
      * row 0: its key 0 is padded in the ancestor's token row (anc[0, 0] = anc[7, 0] = 9) and not in row 0's own;
        row 1: its own tok[1, 0] is PAD, its ancestor's (row 0) is not.  A mask looked up by r changes both rows."""
    c16, heads, ldq_extra = ATT_FORMS[form]
    d = heads * 64
    T = 32 if nkeys <= 32 else 128
    g = gen(1000 * (ord(form) - 96) + 7 * nkeys + seed)
    q = torch.full((ATT_ROWS, d + ldq_extra), float("nan"))
    q[:, :d] = torch.randn(ATT_ROWS, d, generator=g)
    cache = torch.randn(ATT_ROWS + 1, T, 2 * d, generator=g)
    cache[:, nkeys:] = float("nan")
    cache[ATT_POISON] = float("nan")
    cache = cache.to(h16 if c16 else torch.float32)
    anc = torch.randint(0, ATT_ROWS, (ATT_ROWS, T + 3), generator=g, dtype=torch.int32)
    anc[:, nkeys:] = ATT_POISON
    tok = torch.randint(1, 6, (ATT_ROWS + 1, T + 1), generator=g, dtype=torch.int32)
    tok[torch.rand(ATT_ROWS + 1, T + 1, generator=g) < 0.2] = PAD
    anc[ATT_ALLPAD_ROW, 0] = 9
    for j in range(nkeys):
        tok[int(anc[ATT_ALLPAD_ROW, j]), j] = PAD
    anc[0, 0], tok[0, 0] = 9, 3
    anc[1, 0], tok[1, 0] = 0, PAD
    bias = torch.randn(heads, T + 5, generator=g)
    return dict(q=q, cache=cache, anc=anc, tok=tok, bias=bias, heads=heads, d=d, T=T, nkeys=nkeys)


def materialise(cache, tok, anc, nkeys, poison=float("nan"), tok_fill=1):
    """The ancestor-indexed cache and token table as the dense per-row layout `anc == NULL` reads: dense[r, j] =
    cache[anc[r, j], j] and dtok[r, j] = tok[anc[r, j], j] for j < nkeys; `poison` / `tok_fill` at the other positions."""
    rows = anc.shape[0]
    dense = torch.full((rows,) + tuple(cache.shape[1:]), poison, dtype=cache.dtype)
    dtok = torch.full((rows, tok.shape[1]), tok_fill, dtype=tok.dtype)
    j = torch.arange(nkeys)
    for r in range(rows):
        src = anc[r, :nkeys].long()
        dense[r, :nkeys] = cache[src, j]
        dtok[r, :nkeys] = tok[src, j]
    return dense, dtok


def attention_case_ref(case, mask, with_bias, **kw):
    d = case["d"]
    cache = case["cache"]
    return attention_anc(case["q"][:, :d], cache[:, :, :d], cache[:, :, d:], case["anc"], case["nkeys"], case["heads"],
                         tok=case["tok"] if mask else None, bias=case["bias"] if with_bias else None, **kw)


# ---------------------------------------------------------------------------------------------- embedding + LayerNorm
def layer_norm64(x, gamma, beta, eps):
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def embed_ln_anc(tok, tok_off, anc, word, pos, pos0, sem, sem_div, gamma, beta, eps, rows, seq):
    """care_embed_ln (Embeddings.py:134-188): out[r] = LN(word[tok(r)] + pos[pos0 + r % seq] + sem[r / sem_div]); the token
    of row r is tok[trow, tok_off + r % seq] with trow = anc[r / seq, tok_off + r % seq], or r / seq without a table."""
    r = torch.arange(rows)
    s, col = r // seq, tok_off + r % seq
    trow = anc[s, col].long() if anc is not None else s
    x = word[tok[trow, col].long()].to(F64) + pos[pos0 + r % seq].to(F64)
    if sem is not None:
        x = x + sem[r // sem_div].to(F64)
    return layer_norm64(x, gamma, beta, eps)


EMB_ROWS, EMB_T, EMB_VOCAB = 15, 31, 53


def embed_case(d, seq, seed=0):
    """tok int32 [15, 31]; anc int32 [15 / seq, 33] over all 15 token rows; word [53, d], pos [31, d], sem [3, d] (sem_div 5)."""
    g = gen(500 + d + 3 * seq + seed)
    tok = torch.randint(0, EMB_VOCAB, (EMB_ROWS, EMB_T), generator=g, dtype=torch.int32)
    anc = torch.randint(0, EMB_ROWS, (EMB_ROWS // seq, EMB_T + 2), generator=g, dtype=torch.int32)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(tok=tok, anc=anc, word=r(EMB_VOCAB, d), pos=r(EMB_T, d), sem=r(3, d), gamma=r(d) + 1.0, beta=r(d), d=d, seq=seq)


def gather_tokens(tok, anc):
    """The token rows an ancestor table selects, as a table of their own: out[s, c] = tok[anc[s, c], c]."""
    c = torch.arange(tok.shape[1])
    return tok[anc[:, : tok.shape[1]].long(), c.view(1, -1)].contiguous()


# ---------------------------------------------------------------------------------------------- ensemble
def topk_desc_stable(v, k):
    """Indices of the k best entries of every row of v [rows, n]: value descending, equal values by ascending column."""
    v = v.numpy()
    return torch.from_numpy(np.stack([np.argsort(-row, kind="stable")[:k] for row in v]))


def ensemble_average(members, V):
    """torch.stack([log_softmax(x_m)]).mean(0) (Translator.py:125-131) in float64: [rows, V].  Also the per-element
    sum of |log_softmax(x_m)| the error bound of the averaged value is stated in."""
    lps = [torch.log_softmax(x[:, :V].to(F64), dim=1) for x in members]
    avg = lps[0].clone()
    for lp in lps[1:]:
        avg = avg + lp
    return avg / len(lps), torch.stack([lp.abs() for lp in lps]).sum(0)


def ensemble_select(members, V, bm):
    """care_ensemble_select: the bm best columns of the average (value desc, column asc); an average of -inf is never
    selected - with fewer than bm finite averages the tail is (-inf, 0), as care_beam_select documents."""
    avg, mag = ensemble_average(members, V)
    idx = topk_desc_stable(avg, bm)
    val = avg.gather(1, idx)
    idx = torch.where(torch.isinf(val), torch.zeros_like(idx), idx)
    return val, idx.to(torch.int32), mag.gather(1, idx.long())


ENS_ROWS = 6
ENS_SHAPES = ((5, 8), (17, 20), (300, 301), (1029, 1032), (10547, 10560))
ENS_MODELS = (1, 2, 3, 8)
ENS_BM = (1, 5, 8)


def ensemble_cases():
    return [(V, ld, n, bm) for V, ld in ENS_SHAPES for n in ENS_MODELS for bm in ENS_BM if bm <= V]


def ensemble_case(V, ld, n_models, bm, seed=0):
    """n_models logit arrays fp32 [6, ld], N(0, 2^2) in the V valid columns and NaN in the pad columns.  min(bm + 1, V) random
    columns per row (`planted` [6, .], best first) hold 12 - 0.25 rank in EVERY member: their averages are 0.25 apart and
    above every other column's, so the order of the top bm + 1 is never decided by rounding."""
    g = gen(31 * V + 7 * n_models + bm + seed)
    members = []
    for _ in range(n_models):
        x = torch.full((ENS_ROWS, ld), float("nan"))
        x[:, :V] = torch.randn(ENS_ROWS, V, generator=g) * 2.0
        members.append(x)
    n = min(bm + 1, V)
    planted = torch.stack([torch.randperm(V, generator=g)[:n] for _ in range(ENS_ROWS)])
    for x in members:
        x.scatter_(1, planted, (12.0 - 0.25 * torch.arange(n, dtype=torch.float32)).repeat(ENS_ROWS, 1))
    return members, planted


def ensemble_value_bar(mag):
    """1e-5 (test_beam_select's bar for one member's log-softmax) + 2^-23 sum_m |lp_m| (the n fp32 additions and the division)."""
    return 1e-5 + 2.0 ** -23 * mag


# ---------------------------------------------------------------------------------------------- concepts
def concept_finish(scores, k):
    """prepare_merged_probs for seq_len == 1, literally (pred_attribute.py:17-46): (preds [B, k], avg [B])."""
    p = torch.sigmoid(scores[:, :k].to(F64))
    return 1.0 - torch.exp(torch.log(torch.clamp(1.0 - p, 1e-12, 1.0))), p.mean(1)


CF_SHAPES = ((1, 4, 4), (500, 512, 512), (1021, 1021, 1024), (1024, 1030, 1024))   # (k, lds, ldp)
CF_PLANTED = (30.0, -30.0, 100.0, -100.0)


def concept_finish_case(B, k, lds, seed=0):
    """scores fp32 [B, lds]: N(0, 1.5^2) in the k valid columns (NaN past them), with +-30 and +-100 planted in every row
    (k = 1: one of them per row, in turn) - saturation on both sides."""
    g = gen(77 + 13 * B + k + seed)
    s = torch.full((B, lds), float("nan"))
    s[:, :k] = torch.randn(B, k, generator=g) * 1.5
    for b in range(B):
        if k >= 4:
            cols = torch.randperm(k, generator=g)[:4]
            s[b, cols] = torch.tensor(CF_PLANTED)
        else:
            s[b, 0] = CF_PLANTED[b % 4]
    return s


def concept_topk(preds, k, topk):
    """labels[b, j] = index of the j-th largest preds[b, :k] (value desc, index asc): int64 [B, topk]."""
    return topk_desc_stable(preds[:, :k].to(F64), topk)


def concept_embed(labels, word, pos, gamma, beta, eps):
    """out[b, j] = LN(word[labels[b, j]] + pos[j])  (pred_attribute.py:262-270, Embeddings.py:53-87): [B, topk, d]."""
    return layer_norm64(word[labels].to(F64) + pos[: labels.shape[1]].to(F64).unsqueeze(0), gamma, beta, eps)


TOPK_SHAPES = ((1, 1), (3, 3), (500, 30), (1021, 64), (1024, 64), (1024, 1))     # (k, topk)
TOPK_B = 3


def concept_topk_case(k, topk, ldp, seed=0):
    """preds fp32 [3, ldp] in [0, 1] (NaN past column k).  Row 0: values on a grid of 64 steps (k > 64: many exact ties all
    over the order).  Row 1: distinct values, then the value of rank topk - 1 copied onto the entries of ranks topk - 2 and
    topk: an exact tie straddling the boundary (topk == k: onto rank topk - 2 alone).  Row 2: all equal."""
    g = gen(900 + 5 * k + topk + seed)
    p = torch.full((TOPK_B, ldp), float("nan"))
    p[0, :k] = torch.floor(torch.rand(k, generator=g) * 64) / 64
    v = torch.randperm(k, generator=g).float() / k          # distinct, exact in fp32 for k <= 1024
    order = torch.argsort(v, descending=True)
    for rank in (topk - 2, topk):
        if 0 <= rank < k:
            v[order[rank]] = v[order[topk - 1]]
    p[1, :k] = v
    p[2, :k] = 0.5
    return p


# ---------------------------------------------------------------------------------------------- group mean, strided sum
def group_mean(x, in_grp_rows, in_row_off, grp, groups, d):
    """out[g, c] = mean over i < grp of x[g * in_grp_rows + in_row_off + i, c]  (Encoder.py:106): [groups, d]."""
    x = x.to(F64)
    return torch.stack([x[g * in_grp_rows + in_row_off: g * in_grp_rows + in_row_off + grp, :d].mean(0) for g in range(groups)])


def strided_sum(x, rows, d, terms, row_stride, term_stride, scale):
    """out[r] = scale * sum_{k < terms} x[r * row_stride + k * term_stride]; also sum_k |x| per element (the bound's scale)."""
    idx = (torch.arange(rows).view(rows, 1) * row_stride + torch.arange(terms).view(1, terms) * term_stride).reshape(-1)
    xs = x[idx, :d].to(F64).view(rows, terms, d)
    return scale * xs.sum(1), xs.abs().sum(1)


SS_TERMS = (1, 8, 63, 64, 65, 79, 80, 81, 96, 97, 1000)
SS_D = (1, 63, 64, 65, 500)
SS_ROWS = (1, 3)
SS_SCALES = (1.0, 0.25)
SS_MODES = ("shared", "blocks", "interleaved")


def strided_sum_strides(mode, rows, terms):
    """(row_stride, term_stride, rows of x): every output row sums the SAME rows / its own block of rows / every rows-th row."""
    return {"shared": (0, 1, terms), "blocks": (terms, 1, rows * terms), "interleaved": (1, rows, rows * terms)}[mode]


def strided_sum_case(nrows_x, ldx, d, seed=0):
    """x fp32 [nrows_x, ldx]: +-U[0.5, 1.5] in the d valid columns (a dropped or doubled term moves a sum by >= 0.5), NaN past them."""
    g = gen(4242 + nrows_x + 3 * d + seed)
    x = torch.full((nrows_x, ldx), float("nan"))
    sign = torch.randint(0, 2, (nrows_x, d), generator=g).float() * 2 - 1
    x[:, :d] = sign * (torch.rand(nrows_x, d, generator=g) + 0.5)
    return x


def strided_sum_bar(terms, scale, mag):
    """terms 2^-24 scale sum_k |x_k|: holds for ANY order of the fp32 additions (each of the terms - 1 partial sums is at most
    sum |x| and is rounded once, by a relative 2^-24; the scales used are powers of two, exact)."""
    return terms * 2.0 ** -24 * scale * mag

"""GPU: the beam step (care_beam_advance, csrc/beam.hip) and the compaction of a running search (care_expand_index,
care_remap_rows with care_active_slots / care_gather_rows / care_scatter_rows, csrc/compact.hip) called directly, step by step,
on scripted candidates - against tests/beam_reference.py, which tests/test_beam_reference_cpu.py pins to the CPU oracle's beam.

Everything is integers and fp32 sums of two fp32 numbers: the comparison is equality of bits of WHOLE tables, after every step.
Device and restatement start from the same bytes - the engine's initial state (engine_beam._beam_init) for the token and
ancestor tables, scores, done and nfin; sentinels for the finished lists and for one clip's worth of guard elements behind every
table - so equality also says that nothing else was written: guards, columns past t, finished slots past nfin, hypothesis
positions past the length."""
import numpy as np
import pytest
import torch

from beam_reference import EOS, SEED, SHAPES, BeamStateRef, candidates, log_softmax, script, script_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT, FSENT = -77, -12345.0


def _call(name, *args):
    from care_amd import _lib

    _lib.call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(x):
    x = x.cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(x)
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def fresh(B, bm, need, T, V):
    """(restatement, device tables): the same bytes on both sides."""
    ref = BeamStateRef(B, bm, need, T, V, sentinel=SENT, fsentinel=FSENT, guard=1)
    return ref, {k: torch.from_numpy(v.copy()).to(DEV) for k, v in ref.arrays().items()}


def advance(dev, t, cv, ci, B, bm, need, T, V):
    """care_beam_advance with the engine's argument convention (engine_beam._beam_advance)."""
    a_old, a_new = dev["anc%d" % ((t - 1) & 1)], dev["anc%d" % (t & 1)]
    _call("care_beam_advance", _p(cv), _p(ci), _p(dev["scores"]), bm, _p(dev["tok"]), _p(a_old), _p(a_new), _p(dev["done"]),
          _p(dev["nfin"]), need + bm, _p(dev["fscore"]), _p(dev["flen"]), _p(dev["fhyp"]), t, T, need, EOS, V, T + 1, B)


def assert_same_state(dev, ref, where):
    torch.cuda.synchronize()
    for k, want in ref.arrays().items():
        assert torch.equal(_bits(dev[k]), _bits(want)), (k, where)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scripted_search_equals_the_restatement_after_every_step(shape, ties):
    B, bm, need, T, V = shape
    logp = script(B, bm, T, V, SEED, ties)
    ref, dev = fresh(B, bm, need, T, V)
    for t in range(1, T + 1):
        cv, ci = candidates(logp[t - 1], bm)
        advance(dev, t, torch.from_numpy(cv).to(DEV), torch.from_numpy(ci).to(DEV), B, bm, need, T, V)
        ref.step(t, cv, ci)
        assert_same_state(dev, ref, t)
    assert ref.done[:B].all()


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("ld,waves", [(40, 1), (40, 4), (37, 1)])
def test_search_on_candidates_from_beam_select(ld, waves, ties):
    """care_beam_select -> care_beam_advance, as the engine chains them: a wave per row, four waves per row, and (a leading
    dimension that is no multiple of 4) the block-per-row kernel.  Kernel and restatement consume the selection's output."""
    B, bm, need, T, V = 9, 5, 7, 12, 37
    logits = script_logits(B, bm, T, V, SEED, ties)
    ref, dev = fresh(B, bm, need, T, V)
    buf = torch.full((B * bm, ld), float("nan"), device=DEV)
    cv = torch.full((B * bm + 1, bm), float("nan"), device=DEV)
    ci = torch.full((B * bm + 1, bm), SENT, device=DEV, dtype=torch.int32)
    for t in range(1, T + 1):
        buf[:, :V] = torch.from_numpy(logits[t - 1]).to(DEV)
        _call("care_beam_select", _p(buf), ld, V, bm, _p(cv), _p(ci), B * bm, waves)
        advance(dev, t, cv, ci, B, bm, need, T, V)
        torch.cuda.synchronize()
        hv, hi = cv.cpu().numpy(), ci.cpu().numpy()
        assert np.isnan(hv[-1]).all() and (hi[-1] == SENT).all()
        # the selection itself: columns in the order of a stable descending sort, values the log-probabilities
        assert np.array_equal(hi[:-1], candidates(logits[t - 1], bm)[1]), t
        want = np.take_along_axis(log_softmax(logits[t - 1]), hi[:-1].astype(np.int64), axis=1)
        assert np.abs(hv[:-1] - want).max() < 1e-5
        ref.step(t, hv[:-1], hi[:-1])
        assert_same_state(dev, ref, t)
    assert ref.done[:B].all()


def test_beam_advance_rejects_bad_arguments():
    """Every one of these returns before a launch: the tables stay as they were."""
    from care_amd import _lib

    B, bm, need, T, V = 2, 2, 2, 3, 11
    ref, dev = fresh(B, bm, need, T, V)
    cv, ci = torch.zeros(B * bm, bm, device=DEV), torch.zeros(B * bm, bm, device=DEV, dtype=torch.int32)

    def go(bm=bm, t=1, stride=T + 1, need=need, cap=need + bm, B=B, tok=dev["tok"]):
        _call("care_beam_advance", _p(cv), _p(ci), _p(dev["scores"]), bm, _p(tok), _p(dev["anc0"]), _p(dev["anc1"]),
              _p(dev["done"]), _p(dev["nfin"]), cap, _p(dev["fscore"]), _p(dev["flen"]), _p(dev["fhyp"]), t, T, need, EOS, V, stride, B)

    for bad in (dict(bm=0), dict(bm=9), dict(t=0), dict(t=T + 1), dict(stride=65), dict(need=5, cap=4)):
        with pytest.raises(_lib.CareHipError, match="ESHAPE"):
            go(**bad)
    for bad in (dict(tok=None), dict(B=0)):
        with pytest.raises(_lib.CareHipError, match="EINVAL"):
            go(**bad)
    assert_same_state(dev, ref, "rejected calls")


def _rows(fn, src, dst, idx, n):
    """care_gather_rows / care_scatter_rows on tensors whose first dimension is the row (engine_decode._call_rows)."""
    rb = src[0].numel() * src.element_size()
    _call(fn, _p(src), src.stride(0) * src.element_size(), _p(dst), dst.stride(0) * dst.element_size(), _p(idx), n, rb)


@pytest.mark.parametrize("pad", [0, 3])
def test_compaction_in_the_middle_of_a_search(pad):
    """Steps 1 .. 5 on 52 clips, then the raw ABI calls of engine_beam._compact_beam in its order - onto the live clips alone, and
    onto the live clips plus `pad` finished ones riding along - then steps 6 .. T on the compacted set: the per-clip finished
    lists are the uncompacted search's, bit for bit.  (52 x 5 rows = 260 elements: past one 256-thread block.)"""
    B, bm, need, T, V = 52, 5, 5, 12, 37
    cap, stride, t_cut = need + bm, T + 1, 5
    logp = script(B, bm, T, V, SEED)
    cands = [candidates(logp[t - 1], bm) for t in range(1, T + 1)]
    ref, v = fresh(B, bm, need, T, V)
    for t in range(1, T + 1):
        ref.step(t, *cands[t - 1])
        if t <= t_cut:
            advance(v, t, torch.from_numpy(cands[t - 1][0]).to(DEV), torch.from_numpy(cands[t - 1][1]).to(DEV), B, bm, need, T, V)
    n, N = B, B * bm
    out = dict(nfin=torch.full((B, 1), SENT, device=DEV, dtype=torch.int32), fscore=torch.full((B, cap), FSENT, device=DEV),
               flen=torch.full((B, cap), SENT, device=DEV, dtype=torch.int32),
               fhyp=torch.full((B, cap * stride), SENT, device=DEV, dtype=torch.int32))

    def flush(s, clip, k):
        _rows("care_scatter_rows", s["nfin"][:k].view(k, 1), out["nfin"], clip, k)
        for name in ("fscore", "flen"):
            _rows("care_scatter_rows", s[name][:k], out[name], clip, k)
        _rows("care_scatter_rows", s["fhyp"][:k].view(k, -1), out["fhyp"], clip, k)

    idx = torch.full((n + 1,), SENT, device=DEV, dtype=torch.int32)
    cnt = torch.full((2,), SENT, device=DEV, dtype=torch.int32)
    _call("care_active_slots", _p(v["done"]), n, _p(idx), _p(cnt))
    torch.cuda.synchronize()
    done = v["done"][:n].cpu()
    live = int(cnt[0])
    assert 0 < live < n - pad and live == int((done == 0).sum()) and int(cnt[1]) == SENT and int(idx[n]) == SENT
    assert idx[:n].cpu().tolist() == [i for i in range(n) if not done[i]] + [i for i in range(n) if done[i]]
    m = live + pad
    M = m * bm
    clip0 = torch.arange(n, device=DEV, dtype=torch.int32)
    flush(v, clip0, n)
    # --- engine_beam._compact_beam
    idx_r = torch.full((M + 1,), SENT, device=DEV, dtype=torch.int32)
    _call("care_expand_index", _p(idx), m, bm, _p(idx_r))
    i = torch.arange(M, device=DEV)
    assert torch.equal(idx_r[:M].long(), idx[:m].long()[i // bm] * bm + i % bm) and int(idx_r[M]) == SENT
    cmap = torch.zeros(n, 1, device=DEV, dtype=torch.int32)  # clips that are dropped map to clip 0
    _rows("care_scatter_rows", torch.arange(m, device=DEV, dtype=torch.int32).view(m, 1), cmap, idx, m)
    _, w = fresh(m, bm, need, T, V)
    w["clip"] = torch.full((m + 1, 1), SENT, device=DEV, dtype=torch.int32)
    for k in ("done", "nfin"):
        _rows("care_gather_rows", v[k][:n].view(n, 1), w[k][:m].view(m, 1), idx, m)
    _rows("care_gather_rows", clip0.view(n, 1), w["clip"], idx, m)
    for k in ("fscore", "flen"):
        _rows("care_gather_rows", v[k], w[k], idx, m)
    _rows("care_gather_rows", v["fhyp"].view(n + 1, -1), w["fhyp"].view(m + 1, -1), idx, m)
    _rows("care_gather_rows", v["tok"], w["tok"], idx_r, M)
    _rows("care_gather_rows", v["scores"].view(-1, 1), w["scores"].view(-1, 1), idx_r, M)
    for k in ("anc0", "anc1"):
        _rows("care_gather_rows", v[k], w[k], idx_r, M)
        before = w[k][:M].clone()
        _call("care_remap_rows", _p(w[k]), M * stride, _p(cmap), bm)
        assert torch.equal(w[k][:M].long(), cmap.view(-1).long()[before.long() // bm] * bm + before.long() % bm), k
        # a kept clip's ancestors are rows of the clip itself: they moved with it
        assert torch.equal(w[k][:M] // bm, (torch.arange(M, device=DEV, dtype=torch.int32) // bm).unsqueeze(1).expand(M, stride))
    assert torch.equal(w["clip"][:m].view(-1), idx[:m]) and torch.equal(w["tok"][:M], v["tok"][:N][idx_r[:M].long()])
    # --- the rest of the search on the compacted set
    for t in range(t_cut + 1, T + 1):
        cv, ci = (torch.from_numpy(c).to(DEV)[idx_r[:M].long()].contiguous() for c in cands[t - 1])
        advance(w, t, cv, ci, m, bm, need, T, V)
    flush(w, w["clip"].view(-1), m)
    torch.cuda.synchronize()
    for k in w:
        rows = m if w[k].shape[0] == m + 1 else M
        assert bool((w[k][rows:] == (SENT if w[k].dtype == torch.int32 else FSENT)).all()), k  # the guards
    assert bool(w["done"][:m].all())
    for k in ("nfin", "fscore", "flen", "fhyp"):
        assert torch.equal(_bits(out[k].view(-1)), _bits(getattr(ref, k)[:B].reshape(-1))), k


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_remap_rows_and_expand_index(n):
    """care_remap_rows on n table entries (below, at and past one 256-thread block) naming rows of kept AND of dropped clips -
    those map into clip 0 - and care_expand_index on n clips."""
    bm, clips = 5, 40
    g = torch.Generator().manual_seed(n)
    cmap = torch.zeros(clips, dtype=torch.int32)
    kept = torch.randperm(clips, generator=g)[:25]
    cmap[kept] = torch.arange(25, dtype=torch.int32)
    anc = torch.randint(0, clips * bm, (n + 2,), generator=g, dtype=torch.int32)
    anc[0], anc[n - 1] = clips * bm - 1, int(kept[3]) * bm + 2
    dev, cm = anc.clone().to(DEV), cmap.to(DEV)
    _call("care_remap_rows", _p(dev), n, _p(cm), bm)
    idx_c = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32).to(DEV)
    idx_r = torch.full((n * bm + 2,), SENT, device=DEV, dtype=torch.int32)
    _call("care_expand_index", _p(idx_c), n, bm, _p(idx_r))
    torch.cuda.synchronize()
    want = anc.clone()
    want[:n] = cmap[anc[:n].long() // bm] * bm + anc[:n] % bm
    assert torch.equal(dev.cpu(), want)   # (the two entries past n untouched)
    i = torch.arange(n * bm)
    assert torch.equal(idx_r[: n * bm].cpu(), idx_c.cpu()[i // bm] * bm + (i % bm).to(torch.int32))
    assert idx_r[n * bm:].cpu().tolist() == [SENT, SENT]

"""GPU: caption retrieval (care_amd/retrieval.py, csrc/retrieval.hip: care_l2_normalize_rows, care_retrieval_query,
care_retrieval_topk, care_retrieval_gather) against tests/retrieval_reference.py, the float64 restatement of
pretreatment/clip_retrieval.py's `load` / `run`.

Planted banks: orthonormal queries q_b; the rows planted for q_b are a q_b + sqrt(1 - a^2) n with n orthogonal to every query and
a stepping down by `gap` as the index goes up; every other row is orthogonal to every query.  The gap is 0.01 wherever 2 topk
such scores fit above the background: topk = 20 (0.95 .. 0.56) and the 200-row bank of topk = 100 (0.99 .. -1.00, nothing
else in the bank).  With topk = 100 in a bank of 1000 the 200 planted scores cannot be 0.01 apart and still lie above the
other 800 rows (200 x 0.01 is the whole of [-1, 1]); there they are 0.004 apart (0.96 .. 0.164), 30 tau.  Ids, their order
and the counts must equal the restatement's in EVERY position.

Random banks: Gaussian unit vectors.  Two fp32 scores may legitimately swap where their float64 scores differ by less than
tau = 4 D 2^-24 (the fp32 dot-product bound D 2^-24 |q| |t| for each score, doubled for the normalisation roundings); a result
is valid when (a) every id is eligible and the caption groups are distinct, (b) the float64 scores of the ids are non-increasing
within tau, (c) no eligible representative left out scores above the last id by more than tau - and at least 90 % of the rows
must equal the restatement exactly.  Shares of rows for which torch's own fp32 `q @ bank.T` ordering on the CPU equals the
restatement, for the seeds used (recorded when the test was written): D 512 seed 5 topk 20: 37/37, topk 100: 37/37; D 640
seed 6 topk 20: 37/37, topk 100: 36/37.
"""
import numpy as np
import pytest
import torch

import retrieval_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FRAMES = 28


def orthonormal_queries(rng, B, D):
    basis = np.linalg.qr(rng.standard_normal((D, D)))[0].T
    return basis[:B], basis[B:]


def frames_of(rng, queries, n=N_FRAMES):
    """[B, n, D] fp32 frames whose mean lies along the queries."""
    B, D = queries.shape
    wobble = rng.standard_normal((B, n, D)) * 0.05
    wobble -= wobble.mean(1, keepdims=True)
    return (queries[:, None, :] * rng.uniform(2.0, 5.0, size=(B, 1, 1)) + wobble).astype(np.float32)


def planted(seed, B, M, D, per_query, gap, a0):
    """(frames, text_embs fp32 [M, D], ranks): ranks[b] = the rows planted for clip b, best (and lowest index) first.  Clip b
    looks along direction b % nq, nq = as many directions as have room for per_query rows each: clips that share a direction
    share its rows (their frames, and so their rounding, differ)."""
    rng = np.random.default_rng(seed)
    nq = min(B, M // per_query)
    queries, noise_dirs = orthonormal_queries(rng, nq, D)

    def noise(count):
        v = rng.standard_normal((count, D - nq)) @ noise_dirs
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    rows = noise(M)
    where = rng.permutation(M)[: nq * per_query].reshape(nq, per_query)
    ranks = []
    for d in range(nq):
        pos = np.sort(where[d])
        a = (a0 - gap * np.arange(per_query))[:, None]
        rows[pos] = a * queries[d] + np.sqrt(np.maximum(0.0, 1 - a * a)) * noise(per_query)
        ranks.append(pos)
    rows *= rng.uniform(0.5, 8.0, size=(M, 1))
    clip_dir = np.arange(B) % nq
    return frames_of(rng, queries[clip_dir]), rows.astype(np.float32), [ranks[d] for d in clip_dir]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_bank(bank, frames, topk, own=None):
    feats_r, ids, scores, count = bank.retrieve(dev(frames), topk, own)
    torch.cuda.synchronize()
    return feats_r.cpu().numpy(), ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


def assert_exact(ids, count, want, topk):
    for b, w in enumerate(want):
        assert count[b] == len(w), (b, count[b], len(w))
        assert ids[b, : len(w)].tolist() == w, (b, ids[b].tolist(), w)
        assert (ids[b, len(w):] == -1).all()
    assert ids.shape == (len(want), topk)


PLANTED = [  # B, M, D, topk, gap, a0
    (1, 1000, 512, 20, 0.01, 0.95), (3, 1000, 640, 20, 0.01, 0.95), (37, 1000, 512, 20, 0.01, 0.95),
    (1, 200, 512, 100, 0.01, 0.99), (3, 1000, 512, 100, 0.004, 0.96), (37, 1000, 640, 100, 0.004, 0.96)]


@pytest.mark.parametrize("B,M,D,topk,gap,a0", PLANTED)
def test_planted_plain_and_own_ranges(B, M, D, topk, gap, a0):
    from care_amd import CaptionBank

    per = 2 * topk
    frames, embs, ranks = planted(100 + B + topk, B, M, D, per, gap, a0)
    bank = CaptionBank(embs, device=DEV)
    _, ids, _, count = run_bank(bank, frames, topk)
    assert_exact(ids, count, R.retrieve_batch(frames, embs, topk), topk)
    # own ranges: from the clip's 2nd best row on, 25 wide; every third clip has none
    own = np.array([[ranks[b][1], ranks[b][1] + 25] if b % 3 != 2 else [0, 0] for b in range(B)], dtype=np.int64)
    if M >= 1000:
        _, ids, _, count = run_bank(bank, frames, topk, own)
        want = R.retrieve_batch(frames, embs, topk, own)
        assert_exact(ids, count, want, topk)
        assert any(ranks[b][1] not in want[b] for b in range(B) if b % 3 != 2)


def unique_case(seed, B, M, D, topk):
    """Groups of BIT-IDENTICAL rows: all outside the own range, the lowest member inside it, wholly inside, and one string 300
    times at the top of clip 0."""
    frames, embs, ranks = planted(seed, B, M, D, 3 * topk, 0.01, 0.95)      # (0.95 .. 0.36: the subset keeps 70 % of them)
    captions = ["caption {}".format(j) for j in range(M)]
    own = []
    for b in range(B):
        r = ranks[b]
        for src, copies in ((0, (5, 9)), (2, (6,)), (1, (3,)), (7, (8, 30))):
            for c in copies:
                embs[r[c]] = embs[r[src]]
                captions[r[c]] = captions[r[src]]
        own.append([r[1], r[3] + 1] if b != B - 1 else [0, 0])       # covers the ranks 1, 2, 3; the last clip has none
    background = np.setdiff1d(np.arange(M), np.concatenate(ranks))
    hot = background[:: max(1, len(background) // 300)][:300]
    rng = np.random.default_rng(seed + 1)
    q0 = R.query64(frames)[0]
    n = rng.standard_normal(D)
    n -= R.query64(frames).T @ (R.query64(frames) @ n)
    embs[hot] = (3.0 * (0.99 * q0 + np.sqrt(1 - 0.99 ** 2) * n / np.linalg.norm(n))).astype(np.float32)
    for j in hot:
        captions[j] = "a man is talking"
    return frames, embs, captions, np.array(own, dtype=np.int64), hot


def test_planted_unique_and_subset():
    from care_amd import CaptionBank

    B, M, D, topk = 3, 1000, 512, 20
    frames, embs, captions, own, hot = unique_case(7, B, M, D, topk)
    groups = R.group_ids(captions)
    bank = CaptionBank(embs, captions, unique=True, device=DEV)
    assert bank.groups_exact is True
    _, ids, _, count = run_bank(bank, frames, topk, own)
    want = R.retrieve_batch(frames, embs, topk, own, groups)
    assert_exact(ids, count, want, topk)
    admissible = [j for j in hot if not own[0][0] <= j < own[0][1]]
    assert want[0][0] == admissible[0] and len(set(want[0]) & set(hot.tolist())) == 1      # 300 copies: one id, the lowest
    # without `unique` on the same bank the copies fill the row, lowest index first
    plain = CaptionBank(embs, device=DEV)
    _, ids, scores, count = run_bank(plain, frames, topk, own)
    assert_exact(ids, count, R.retrieve_batch(frames, embs, topk, own), topk)
    assert ids[0].tolist() == admissible[:topk] and len(set(scores[0].tolist())) == 1
    # --ratio: 70 % of the bank, own ranges and ids in original numbering
    sampled = np.sort(np.random.default_rng(70).permutation(M)[: int(0.7 * M)])
    q64, unit64 = R.query64(frames), R.unit_rows64(embs)
    for full, g in ((bank, groups), (plain, None)):
        _, ids, _, count = run_bank(full.subset(sampled), frames, topk, own)
        want = R.retrieve_batch(frames, embs, topk, own, g, sampled)
        assert all(R.scores64(q64[b], unit64)[w[-1]] > 0.3 for b, w in enumerate(want))     # still among the planted rows
        assert_exact(ids, count, want, topk)
        assert set(ids.reshape(-1).tolist()) <= set(sampled.tolist())


def test_exact_ties_do_not_depend_on_the_batch():
    from care_amd import CaptionBank

    rng = np.random.default_rng(9)
    M, D, topk = 1000, 512, 20
    embs = rng.standard_normal((M, D)).astype(np.float32)
    for j in (3, 500, 999):
        embs[j] = embs[17]
    frames = rng.standard_normal((37, N_FRAMES, D)).astype(np.float32)
    frames[36] = embs[17] * 0.5 + rng.standard_normal((N_FRAMES, D)).astype(np.float32) * 0.1
    bank = CaptionBank(embs, device=DEV)
    _, ids, scores, count = run_bank(bank, frames, topk)
    _, ids1, scores1, count1 = run_bank(bank, frames[36:], topk)
    assert ids[36, :4].tolist() == [3, 17, 500, 999]
    assert len(set(scores[36, :4].tolist())) == 1
    assert np.array_equal(ids[36], ids1[0]) and np.array_equal(scores[36].view(np.int32), scores1[0].view(np.int32)) and count[36] == count1[0]
    # ... nor on the scan form: the same clip among 17 .. 32 rows (2 x 2 tiles a wave)
    _, ids2, scores2, _ = run_bank(bank, frames[12:], topk)
    assert np.array_equal(ids[36], ids2[-1]) and np.array_equal(scores[36].view(np.int32), scores2[-1].view(np.int32))


def test_short_rows():
    from care_amd import CaptionBank

    B, M, D, topk = 3, 50, 512, 100
    rng = np.random.default_rng(11)
    queries, noise_dirs = orthonormal_queries(rng, B, D)
    a = np.stack([0.5 - 0.01 * rng.permutation(M) for _ in range(B)], axis=1)               # [M, B]: every clip its own order
    n = rng.standard_normal((M, D - B)) @ noise_dirs
    rows = a @ queries + np.sqrt(1 - (a * a).sum(1, keepdims=True)) * n / np.linalg.norm(n, axis=1, keepdims=True)
    embs = (rows * rng.uniform(0.5, 8.0, size=(M, 1))).astype(np.float32)
    frames = frames_of(rng, queries)
    own = np.array([[10, 25], [0, 0], [40, 50]], dtype=np.int64)
    gather = rng.standard_normal((M, 768)).astype(np.float32)
    bank = CaptionBank(embs, gather_embs=gather, device=DEV)
    feats_r, ids, scores, count = run_bank(bank, frames, topk, own)
    want = R.retrieve_batch(frames, embs, topk, own)
    assert [len(w) for w in want] == [35, 50, 40] and count.tolist() == [35, 50, 40]
    assert_exact(ids, count, want, topk)
    assert feats_r.shape == (B, topk, 768)
    for b in range(B):
        assert np.array_equal(feats_r[b, : count[b]].view(np.int32), gather[ids[b, : count[b]]].view(np.int32))
        assert not feats_r[b, count[b]:].any() and np.isneginf(scores[b, count[b]:]).all()


def check_valid(ids, count, q64, unit64, topk, own, groups, D):
    """The three conditions of the module docstring for every row; returns the number of rows equal to the restatement."""
    t, exact = R.tau(D), 0
    M = unit64.shape[0]
    for b in range(q64.shape[0]):
        s = R.scores64(q64[b], unit64)
        info = None if own is None else own[b]
        want = R.retrieve(q64[b], unit64, topk, info, groups)
        got = ids[b, : count[b]].tolist()
        assert count[b] == len(want) and (ids[b, count[b]:] == -1).all()
        exact += got == want
        # (a)
        assert all(0 <= j < M and not (info is not None and info[0] <= j < info[1]) for j in got)
        if groups is not None:
            assert len({groups[j] for j in got}) == len(got)
        else:
            assert len(set(got)) == len(got)
        # (b)
        assert all(s[got[i + 1]] <= s[got[i]] + t for i in range(len(got) - 1)), b
        # (c): the restatement's ids are the best eligible representatives; one of them left out may not beat the last id
        for j in set(want) - set(got) if groups is None else [j for j in want if groups[j] not in {groups[g] for g in got}]:
            assert s[j] <= s[got[-1]] + t, (b, j)
    return exact


@pytest.mark.parametrize("D,seed", [(512, 5), (640, 6)])
def test_random_banks(D, seed):
    from care_amd import CaptionBank

    rng = np.random.default_rng(seed)
    B, M = 37, 1000
    embs = rng.standard_normal((M, D)).astype(np.float32)
    frames = rng.standard_normal((B, N_FRAMES, D)).astype(np.float32)
    captions = ["caption {}".format(j % 700) for j in range(M)]               # 300 strings twice, differently embedded
    groups = R.group_ids(captions)
    own = np.stack([np.arange(B) * 20, np.arange(B) * 20 + 20], axis=1).astype(np.int64)
    q64, unit64 = R.query64(frames), R.unit_rows64(embs)
    plain, uniq = CaptionBank(embs, device=DEV), CaptionBank(embs, captions, unique=True, device=DEV)
    assert uniq.groups_exact is False
    for topk in (20, 100):
        _, ids, scores, count = run_bank(plain, frames, topk, own)
        exact = check_valid(ids, count, q64, unit64, topk, own, None, D)
        print("D {} topk {} plain: {} of {} rows equal the restatement".format(D, topk, exact, B))
        assert exact >= 0.9 * B
        for b in range(B):
            assert np.abs(scores[b] - R.scores64(q64[b], unit64)[ids[b]]).max() <= R.tau(D) / 2
    # `unique` over groups that are NOT bit-identical: the representative is the lowest admissible index whatever it scores, so
    # the yardstick is the restatement over the representatives (for the reference's own choice see retrieval.py's docstring)
    _, ids, _, count = run_bank(uniq, frames, 20, own)
    first, prev = uniq.first_host, uniq.prev_host
    from care_amd.retrieval import eligible
    for b in range(B):
        reps = np.array([j for j in range(M) if eligible(j, own[b][0], own[b][1], first, prev)])
        want = R.ranked(R.scores64(q64[b], unit64[reps]), reps)[:20].tolist()
        s = R.scores64(q64[b], unit64)
        got = ids[b].tolist()
        assert count[b] == 20 and set(got) <= set(reps.tolist()) and len({groups[j] for j in got}) == 20
        assert all(s[got[i + 1]] <= s[got[i]] + R.tau(D) for i in range(19))
        assert all(s[j] <= s[got[-1]] + R.tau(D) for j in set(want) - set(got))


def test_query_and_normalisation():
    from care_amd import CaptionBank, _lib

    rng = np.random.default_rng(13)
    for B, D in ((3, 512), (37, 640)):
        frames = (rng.standard_normal((B, N_FRAMES, D)) + 0.3).astype(np.float32)
        embs = (rng.standard_normal((70, D)) * 3).astype(np.float32)
        bank = CaptionBank(embs, device=DEV)
        q = bank.query(dev(frames))
        torch.cuda.synchronize()
        assert np.abs(q.cpu().numpy() - R.query64(frames)).max() <= 1e-6
        assert np.abs(bank.unit.cpu().numpy() - R.unit_rows64(embs)).max() <= 1e-6
        assert np.array_equal(bank.table.cpu().numpy(), embs)
    # the entry points by name, once more through the raw binding: a zero row where an id is out of the table
    table, ids = dev(embs), torch.tensor([5, -1, 69, 70], dtype=torch.int64, device=DEV)
    out = torch.full((4, D), 7.0, device=DEV)
    _lib.call("care_retrieval_gather", _lib.ptr(table), 70, D, _lib.ptr(ids), 4, _lib.ptr(out))
    torch.cuda.synchronize()
    assert torch.equal(out[0], table[5]) and torch.equal(out[2], table[69]) and not out[1].any() and not out[3].any()


def test_end_to_end_captions():
    """translate_batch over attach_retrieval(...) against the same model over feats_r built from the restatement's ids."""
    from care_amd import CaptionBank, attach_retrieval, get_framework, get_translator
    from care_amd.checkpoint import CaptionRunner
    from care_amd.configs import feat_shapes, make_opt
    from care_amd.synth import synth_state_dict

    opt = make_opt("msrvtt_care")
    B, M, topk = 3, 1000, opt["retrieval_topk"]
    runner = CaptionRunner(opt)
    model = runner.captioner.eval()
    model.load_state_dict(synth_state_dict(3, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model.set_compute_dtype("fp32")
    model.to(DEV)
    frames, embs, ranks = planted(21, B, M, opt["dim_i"], 2 * topk, 0.01, 0.95)
    gen = torch.Generator().manual_seed(4)
    shapes = dict(zip(opt["modality"], feat_shapes(opt, B)))
    rest = [torch.from_numpy(frames) if ch == "i" else torch.randn(shapes[ch], generator=gen) for ch in opt["modality"] if ch != "r"]
    own = np.array([[ranks[b][1], ranks[b][1] + 25] for b in range(B)], dtype=np.int64)
    bank = CaptionBank(embs, device=DEV)
    feats = attach_retrieval([f.to(DEV) for f in rest], opt, bank, own)
    at = opt["modality"].index("r")
    assert len(feats) == len(opt["modality"]) and feats[at].shape == shapes["r"]
    want_ids = np.array(R.retrieve_batch(frames, embs, topk, own))
    ref = list(feats)
    ref[at] = dev(embs[want_ids])
    assert torch.equal(feats[at], ref[at])
    tr = get_translator(opt)
    got, want = tr.translate_batch([model], {"feats": feats}), tr.translate_batch([model], {"feats": ref})
    assert got == want and all(len(h[0]) > 0 for h in got[0])
    eng = model.engine()
    labels = eng.translate_greedy(feats, use_graph=False)[0]["semantic_labels"].clone()
    assert torch.equal(labels, eng.translate_greedy(ref, use_graph=False)[0]["semantic_labels"])
    assert runner.translate_step({"feats": feats}) == want

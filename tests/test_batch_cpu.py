"""CPU: the rules of the batch a ClipStore builds - tests/batch_reference.py against the genuine reference where
it imports, against hand-worked cases where it does not, and the store's host-side ingestion against both.

`misc/utils.py` imports in the build image: its equally-sampled ids and the snippet bounds are recorded in
tests/golden/batch/frame_ids.json (tools/gen_batch_golden.py).  `dataloader.py` and `misc/utils_corpora.py` do not (h5py, nltk
and a downloader are absent), so `_padding` (:661-675), source / target (:565-571) and the concept labels
(utils_corpora.py:424-441) are pinned by cases worked out by hand below.

The one statistical test is of the DEFINITION of `all_random`, not of the kernel: over 4096 items with n_total 8, n_frames 3
every frame is included 4096 * 3 / 8 = 1536 times in expectation, a binomial count of standard deviation
sqrt(4096 * 3/8 * 5/8) = 31; the bound is 6 sd = 186.  Seed 20 is fixed; it was checked on the CPU that it passes (counts
1461 .. 1602).
"""
import json
import os

import numpy as np
import pytest
import torch

import batch_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch", "frame_ids.json")
PAD, BOS, EOS = R.PAD, R.BOS, R.EOS


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


def test_equally_sampled_ids_and_bounds_are_the_reference_s():
    from care_amd.clipstore import snippet_bounds
    from care_amd.data import get_uniform_ids_from_k_snippets

    cases = _golden()
    assert len(cases) >= 10
    for c in cases:
        n_total, k = c["n_total"], c["n_frames"]
        assert R.snippet_bounds(n_total, k) == c["bounds"] == snippet_bounds(n_total, k)
        assert R.frame_ids(5, n_total, k, "equally_sampling", seed=3, epoch=9) == c["ids"]
        assert get_uniform_ids_from_k_snippets(n_total, k) == c["ids"]


def test_the_mix_is_the_sampler_s():
    """h with the constants of csrc/sample.hip (smp_mix), and the store's vectorised copy of it."""
    from care_amd.clipstore import _mix, epoch_order

    assert R.h(0, 0) == 0xE220A8397B1DCDAF                       # splitmix64's first output from state 0
    z = 0x9E3779B97F4A7C15 * 3 & R.M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
    assert R.h(0, 2) == z ^ (z >> 31)
    for a, n in [(0, 0), (1, 5), (R.M64, R.M64), (0x123456789ABCDEF, 77), (5, R.SHUFFLE)]:
        assert int(_mix(np.uint64(a), np.uint64(n))) == R.h(a, n)
    for n, seed, epoch in [(1, 0, 0), (37, 5, 2), (200, 2 ** 63 + 1, 7)]:
        assert epoch_order(n, seed, epoch).tolist() == R.epoch_order(n, "train", seed, epoch)
    assert R.epoch_order(37, "train", 5, 2) != R.epoch_order(37, "train", 5, 3)
    assert sorted(R.epoch_order(37, "train", 5, 2)) == list(range(37))
    assert R.epoch_order(37, "validate", 5, 2) == list(range(37))


@pytest.mark.parametrize("n_total,n_frames", [(60, 28), (64, 64), (64, 1), (8, 3), (1, 1), (7, 5)])
def test_segment_random_ids_lie_inside_their_snippets(n_total, n_frames):
    bound = R.snippet_bounds(n_total, n_frames)
    seen = set()
    for item in range(200):
        ids = R.frame_ids(item, n_total, n_frames, "segment_random", seed=11, epoch=4)
        assert all(bound[i] <= ids[i] < bound[i + 1] for i in range(n_frames))
        seen.add(tuple(ids))
    assert len(seen) > 1 or all(bound[i + 1] - bound[i] == 1 for i in range(n_frames))
    assert R.frame_ids(3, n_total, n_frames, "segment_random", 11, 4) == R.frame_ids(3, n_total, n_frames, "segment_random", 11, 4)


@pytest.mark.parametrize("n_total,n_frames", [(60, 28), (64, 64), (64, 1), (8, 3), (1, 1), (8, 8)])
def test_all_random_ids_ascend_in_range(n_total, n_frames):
    for item in range(100):
        ids = R.frame_ids(item, n_total, n_frames, "all_random", seed=1, epoch=item % 3)
        assert len(ids) == n_frames and all(0 <= f < n_total for f in ids)
        assert all(a < b for a, b in zip(ids, ids[1:]))
        if n_frames == n_total:
            assert ids == list(range(n_total))
    with pytest.raises(ValueError, match="n_frames"):
        R.frame_ids(0, 4, 5, "all_random")
    with pytest.raises(ValueError, match="n_frames"):
        R.frame_ids(0, 4, 5, "segment_random")


def test_all_random_includes_every_frame_equally_often():
    counts = np.zeros(8, dtype=np.int64)
    for item in range(4096):
        counts[R.frame_ids(item, 8, 3, "all_random", seed=20, epoch=0)] += 1
    assert counts.sum() == 4096 * 3
    assert np.abs(counts - 1536).max() <= 186, counts.tolist()


def test_padding_and_source_target_by_hand():
    """dataloader.py:661-675 and :565-571, max_len 8."""
    assert R.padding([BOS, EOS], 8) == [2, 3, 0, 0, 0, 0, 0, 0]
    assert R.padding([BOS, 10, 11, 12, 13, 14, EOS], 8) == [2, 10, 11, 12, 13, 14, 3, 0]
    assert R.padding([BOS, 10, 11, 12, 13, 14, 15, EOS], 8) == [2, 10, 11, 12, 13, 14, 15, 3]          # exactly max_len: as it is
    assert R.padding([BOS, 10, 11, 12, 13, 14, 15, 16, EOS], 8) == [2, 10, 11, 12, 13, 14, 15, 3]      # cut, EOS forced
    assert R.source_target([BOS, 10, 11, EOS], 8) == ([2, 10, 11, 3, 0, 0, 0], [10, 11, 3, 0, 0, 0, 0])
    long = [BOS] + list(range(20, 33)) + [EOS]                                                           # 15 tokens
    assert R.source_target(long, 8) == ([2, 20, 21, 22, 23, 24, 25], [20, 21, 22, 23, 24, 25, 3])


def test_concept_labels_by_hand():
    """misc/utils_corpora.py:424-441: attribute a is word 6 + a; BOS / EOS by position, every caption of the video."""
    caps = [[BOS, 5, 6, 7, EOS], [BOS, 6 + 32, 6 + 33, EOS], [BOS, EOS], [BOS, 3005, 3006, 1, EOS]]
    lab = R.attribute_labels(caps)
    assert lab.shape == (3000,) and lab.dtype == np.float32
    assert np.flatnonzero(lab).tolist() == [0, 1, 32, 33, 2999]          # 5 and 3006 lie outside, 1 (UNK) below
    assert np.flatnonzero(R.attribute_labels(caps, 33)).tolist() == [0, 1, 32]
    assert np.flatnonzero(R.attribute_labels(caps, 1)).tolist() == [0]
    assert R.attribute_labels([[BOS, 7, EOS]], 4).tolist() == [0, 1, 0, 0]


# ------------------------------------------------------------------------------------------------- the store's ingestion
NAMES = ["video0", "video1", "video2", "video3"]


def _opt(**over):
    opt = {"modality": "mi", "dim_m": 6, "dim_i": 5, "n_frames": 3, "max_len": 8, "load_feats_type": 0, "retrieval_topk": 2, "dim_r": 4}
    opt.update(over)
    return opt


def _dbs():
    rng = np.random.RandomState(0)
    m_a = {v: rng.randn(8, 4).astype(np.float32) for v in NAMES}
    m_b = {v: rng.randn(2).astype(np.float32) for v in NAMES}              # a 1-D vector beside a 2-D table
    i_a = {v: rng.randn(5).astype(np.float32) for v in NAMES if v != "video2"}   # 1-D alone; video2 is missing
    r_a = {v: rng.randn(5, 4).astype(np.float32) for v in NAMES}
    return {"m": [m_a, m_b], "i": [i_a], "r": [r_a]}


def _caps():
    return {"video0": [[BOS, 10, 11, EOS]], "video1": [[BOS, 12, EOS], [BOS, 13, 14, EOS], [BOS, EOS]],
            "video2": [[BOS, 15, EOS]] * 5, "video3": [[BOS, 16, EOS], [BOS, 17, EOS]]}


def test_ingestion_rules():
    from care_amd import ClipStore
    from care_amd.data import load_video_feats

    dbs = _dbs()
    store = ClipStore(_opt(modality="mir"), dbs, NAMES, device=None)
    m, i, r = store.tables
    assert (m.n_total, i.n_total, store.n_total) == (8, 1, 8)
    assert m.pitch % 16 == 0 and i.pitch % 16 == 0 and r.pitch % 16 == 0 and (m.row_bytes, i.row_bytes, r.row_bytes) == (24, 20, 32)
    want_m = R.ingest_modality(dbs["m"], NAMES, 6)
    assert np.array_equal(m.rows().numpy(), want_m)
    for v, name in enumerate(NAMES):                                        # channel concat; the 1-D vector on every frame
        assert np.array_equal(want_m[v][:, :4], dbs["m"][0][name]) and np.array_equal(want_m[v][5, 4:], dbs["m"][1][name])
    want_i = R.ingest_modality(dbs["i"], NAMES, 5)
    assert np.array_equal(i.rows().numpy(), want_i) and want_i.shape == (4, 1, 5)
    assert not want_i[2].any() and want_i[1].any()                          # the missing video is zeros
    assert np.array_equal(r.rows().numpy(), R.ingest_retrieval(dbs["r"][0], NAMES, 2))
    assert np.array_equal(r.rows().numpy()[3], dbs["r"][0]["video3"][:2])   # the first retrieval_topk rows
    assert not m.data[:, :, 6:].any()                                       # the pitch padding
    # ... `r` as data.py loads it per video
    assert np.array_equal(load_video_feats({"r": dbs["r"]}, "video1", _opt(modality="r"))[0], r.rows().numpy()[1])
    assert store.bounds == [0, 2, 5, 8] and R.frame_ids(0, 8, 3, "equally_sampling") == [1, 3, 6]
    # 16-bit: rounded once, at ingestion
    s16 = ClipStore(_opt(), dbs, NAMES, dtype=torch.bfloat16, device=None)
    assert s16.tables[0].data.dtype == torch.bfloat16 and s16.tables[0].row_bytes == 12 and s16.tables[0].pitch == 16
    assert torch.equal(s16.tables[0].rows(), torch.from_numpy(want_m).to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        store.batch([0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ClipStore(_opt(), dbs, NAMES, device="cpu")


def test_refusals_by_name():
    from care_amd import ClipStore

    dbs = _dbs()
    with pytest.raises(ValueError, match="`t`"):
        ClipStore(_opt(modality="mt"), dict(dbs, t=[{}]), NAMES, device=None)
    with pytest.raises(NotImplementedError, match="load_feats_type"):
        ClipStore(_opt(load_feats_type=1), dbs, NAMES, device=None)
    with pytest.raises(NotImplementedError, match="all_random"):
        big = {"m": [{v: np.zeros((65, 6), np.float32) for v in NAMES}]}
        ClipStore(_opt(modality="m", random_type="all_random"), big, NAMES, device=None)
    with pytest.raises(NotImplementedError, match="n_frames"):
        ClipStore(_opt(n_frames=9), dbs, NAMES, device=None)                # segment_random over 8 frames
    with pytest.raises(ValueError, match="random_type"):
        ClipStore(_opt(random_type="sometimes"), dbs, NAMES, device=None)
    with pytest.raises(ValueError, match="n_attributes"):
        ClipStore(_opt(), dbs, NAMES, device=None, n_attributes=3001)
    with pytest.raises(ValueError, match="channels"):
        ClipStore(_opt(dim_m=7), dbs, NAMES, device=None)
    for bad in ([[10, 11, EOS]], [[BOS, 10, 11]], [[BOS]], []):
        with pytest.raises(ValueError, match="BOS|no caption"):
            ClipStore(_opt(), dbs, NAMES, captions=dict(_caps(), video2=bad), device=None)


def test_caption_table_and_infosets():
    from care_amd import ClipStore

    caps = _caps()
    store = ClipStore(_opt(), _dbs(), NAMES, captions=caps, device=None)
    hc = store.host_captions
    assert hc["vid_first"].tolist() == [0, 1, 4, 9, 11] and hc["cap_video"].tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3]
    assert hc["cap_start"].tolist()[:5] == [0, 4, 7, 11, 13]
    assert hc["tokens"].tolist()[:7] == [BOS, 10, 11, EOS, BOS, 12, EOS]
    assert store.n_items("train") == 11 and store.item_captions("train").tolist() == list(range(11))
    assert store.item_captions("validate").tolist() == [0, 1, 4, 9] == store.item_captions("test").tolist()
    want = R.infoset(caps, NAMES, "train", 0)
    assert [(int(hc["cap_video"][c]), int(c - hc["vid_first"][hc["cap_video"][c]])) for c in store.item_captions("train").tolist()] == want
    # n_caps_per_video = 2: min(2, captions) a video, fixed by opt["seed"]
    sub = ClipStore(_opt(n_caps_per_video=2, seed=5), _dbs(), NAMES, captions=caps, device=None)
    got = [(int(hc["cap_video"][c]), int(c - hc["vid_first"][hc["cap_video"][c]])) for c in sub.item_captions("train").tolist()]
    assert got == R.infoset(caps, NAMES, "train", 2, seed=5) and [v for v, _ in got] == [0, 1, 1, 2, 2, 3, 3]
    again = ClipStore(_opt(n_caps_per_video=2, seed=5), _dbs(), NAMES, captions=caps, device=None)
    assert again.item_captions("train").tolist() == sub.item_captions("train").tolist()
    assert R.infoset(caps, NAMES, "validate", 2, seed=5) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    with pytest.raises(ValueError, match="mode"):
        store.n_items("trainval")

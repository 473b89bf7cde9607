"""numpy / pure-Python restatement of the batch a `care_amd.ClipStore` builds on the device (include/care_hip.h, "Training
and validation batches built on the device") - the expected value of tests/test_batch_cpu.py,
tests/test_gpu_batch_kernels.py and tests/test_gpu_clipstore.py.  Nothing here imports care_amd.clipstore.

What is restated, with the reference's lines:
  frame ids      dataloader.py:23-31 get_frame_ids -> misc/utils.py:311-317 (equally_sampling), :320-326 (segment_random),
                 :329-332 (all_random) - the two random types over the counter-based h below instead of numpy's / Python's
                 global generators, whose streams cannot be reproduced
  ingestion      dataloader.py:232-262 _load_feats (load_feats_type 0), :808-814 load_r_feats
  the infoset    dataloader.py:389-453 _make_infoset, :711-721 (what a mode sets)
  text           dataloader.py:559-571 _make_source_target, :661-675 _padding
  concept labels misc/utils_corpora.py:424-441 get_vid2attribute_mappings
"""
import numpy as np

PAD, BOS, EOS = 0, 2, 3                      # config/Constants.py:1-6
ATTRIBUTE_START, ATTRIBUTE_END = 6, 3006     # config/Constants.py:15-16
N_TOTAL_FRAMES = 60                          # config/Constants.py:27
M64 = (1 << 64) - 1
SHUFFLE = 0xFFFFFFFF                         # the counter of an item's place in the epoch's order (no frame has it)
TYPES = ("equally_sampling", "segment_random", "all_random")


def h(a: int, n: int) -> int:
    """fin(a + 0x9E3779B97F4A7C15 (n + 1)) with the splitmix64 finaliser, in uint64 (csrc/sample.hip, smp_mix)."""
    z = (a + 0x9E3779B97F4A7C15 * ((n + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def item_key(seed: int, epoch: int, item: int) -> int:
    return h(h(seed & M64, epoch & M64), item & M64)


def snippet_bounds(n_total: int, n_frames: int):
    """misc/utils.py:313 / :322."""
    return [int(i) for i in np.linspace(0, n_total, n_frames + 1)]


def frame_ids(item: int, n_total: int, n_frames: int, random_type: str, seed: int = 0, epoch: int = 0):
    bound = snippet_bounds(n_total, n_frames)
    if random_type == "equally_sampling":      # misc/utils.py:311-317
        return [(bound[i] + bound[i + 1]) // 2 for i in range(n_frames)]
    if n_frames > n_total:
        raise ValueError("n_frames {} > n_total {}: the reference's randint / sample raise".format(n_frames, n_total))
    k1 = item_key(seed, epoch, item)
    if random_type == "segment_random":        # :320-326, randint(bound[i], bound[i + 1]) as a multiply-high
        return [bound[i] + (((h(k1, i) >> 32) * (bound[i + 1] - bound[i])) >> 32) for i in range(n_frames)]
    if random_type == "all_random":            # :329-332, sorted(random.sample(range(length), k))
        order = sorted(range(n_total), key=lambda f: (h(k1, f), f))
        return sorted(order[:n_frames])
    raise ValueError(random_type)


def padding(seq, max_len: int):
    """dataloader.py:661-675 with add_eos = True."""
    res = list(seq)
    if len(res) > max_len:
        res = res[:max_len]
        res[-1] = EOS
    else:
        res += [PAD] * (max_len - len(res))
    return res


def source_target(caption, max_len: int):
    """dataloader.py:565-571: (input_ids, labels)."""
    p = padding(caption, max_len)
    return p[:-1], p[1:]


def attribute_labels(captions, n_attributes: int = ATTRIBUTE_END - ATTRIBUTE_START, attribute_start: int = ATTRIBUTE_START):
    """misc/utils_corpora.py:424-441 over the first n_attributes attributes (crit_attribute.py:39 slices the rest away)."""
    out = np.zeros(n_attributes, dtype=np.float32)
    for cap in captions:
        assert cap[0] == BOS and cap[-1] == EOS
        for w in cap[1:-1]:
            if attribute_start <= w < attribute_start + n_attributes:
                out[w - attribute_start] = 1
    return out


def ingest_modality(tables, names, dim: int, n_total_frames: int = N_TOTAL_FRAMES) -> np.ndarray:
    """[n_videos, n_total, dim] fp32 of one modality (dataloader.py:232-262): tables concatenated on the channel axis, a 1-D
    vector repeated over the frames (n_total = 1 when every table is 1-D: every frame id reads row 0), a missing video zeros."""
    per_video, n_total = [], None
    for vid in names:
        if any(vid not in t for t in tables):
            per_video.append(None)
            continue
        parts = [np.asarray(t[vid]) for t in tables]
        lens = {p.shape[0] for p in parts if p.ndim == 2}
        assert len(lens) <= 1
        n = lens.pop() if lens else 1
        parts = [p[np.newaxis, :].repeat(n, axis=0) if p.ndim == 1 else p for p in parts]
        feats = np.concatenate(parts, axis=1).astype(np.float32)
        assert feats.shape[1] == dim and n_total in (None, n)
        n_total = n
        per_video.append(feats)
    n_total = n_total if n_total is not None else n_total_frames
    return np.stack([np.zeros((n_total, dim), np.float32) if f is None else f for f in per_video])


def ingest_retrieval(table, names, topk: int) -> np.ndarray:
    """[n_videos, topk, dim] (dataloader.py:808-814)."""
    return np.stack([np.asarray(table[vid])[:topk, :].astype(np.float32) for vid in names])


def infoset(captions, names, mode: str, n_caps_per_video: int = 0, seed: int = 0):
    """[(video row, cap_id)] (dataloader.py:389-453 with what :711-721 sets): train = every caption, or a subset of
    min(k, captions) a video drawn once from RandomState(seed); validate / test = caption 0 of every video."""
    rng = np.random.RandomState(seed)
    items = []
    for v, vid in enumerate(names):
        n = len(captions[vid])
        if mode != "train":
            ids = [0]
        elif n_caps_per_video == 0:
            ids = list(range(n))
        else:
            ids = [int(i) for i in rng.choice(list(range(n)), min(n, n_caps_per_video), replace=False)]
        items += [(v, c) for c in ids]
    return items


def epoch_order(n_items: int, mode: str, seed: int = 0, epoch: int = 0):
    """The order a loader visits the items in: train = ascending (h(item key, SHUFFLE), item); else as they lie."""
    if mode != "train":
        return list(range(n_items))
    return sorted(range(n_items), key=lambda i: (h(item_key(seed, epoch, i), SHUFFLE), i))


def host_batch(tables, n_totals, captions, names, items, positions, mode, n_frames, max_len, random_type="segment_random",
               n_attributes=ATTRIBUTE_END - ATTRIBUTE_START, seed=0, epoch=0, retrieval=()):
    """The batch of the infoset positions `positions` as numpy arrays.  tables: one [n_videos, n_total_m, dim] array per
    modality (16-bit tables as their uint16 bit patterns - a batch is a copy); retrieval: the indices of modalities whose rows
    are 0 .. n - 1 whatever the frame ids; items: infoset()'s list."""
    n_total = max([n for i, n in enumerate(n_totals) if i not in retrieval and n > 1], default=N_TOTAL_FRAMES)
    rt = random_type if mode == "train" else "equally_sampling"
    fids = np.array([frame_ids(p, n_total, n_frames, rt, seed, epoch) for p in positions], dtype=np.int32).reshape(len(positions), n_frames)
    vids = np.array([items[p][0] for p in positions], dtype=np.int32)
    feats = []
    for m, tab in enumerate(tables):
        if m in retrieval:
            feats.append(tab[vids])
        elif n_totals[m] == 1:
            feats.append(tab[vids][:, np.zeros(n_frames, dtype=np.int64)])
        else:
            feats.append(np.stack([tab[v][f] for v, f in zip(vids, fids)]) if len(vids) else tab[:0, :n_frames])
    out = {"feats": feats, "frame_ids": fids, "video_ids": vids}
    if captions is not None:
        st = [source_target(captions[names[items[p][0]]][items[p][1]], max_len) for p in positions]
        out["caption_ids"] = np.array([items[p][1] for p in positions], dtype=np.int32)
        out["input_ids"] = np.array([s for s, _ in st], dtype=np.int64).reshape(len(positions), max_len - 1)
        out["labels"] = np.array([t for _, t in st], dtype=np.int64).reshape(len(positions), max_len - 1)
        out["labels_attr"] = np.stack([attribute_labels(captions[names[items[p][0]]], n_attributes) for p in positions]) \
            if len(positions) else np.zeros((0, n_attributes), np.float32)
    return out

"""A clip store in HBM: the data set's feature tables and captions live on the MI355X and every batch is built there.

    store = care_amd.ClipStore(opt, databases, video_names, captions=None, dtype=torch.float32, device="cuda")
    for batch in store.loader(mode="train", batch_size=512, epoch=e, seed=s, depth=2): ...
    batch = store.batch(items, mode="train", epoch=e, seed=s, out=None)

Replaces, for `load_feats_type == 0`, what the reference does per item on the host - `JointDataset.__getitem__`
(dataloader.py:777-803: get_frame_ids :23-31, _load_feats :232-262, load_r_feats :808-814, _prepare_input_ids :524-571,
_padding :661-675, the concept labels of misc/utils_corpora.py:424-441), default_collate and the copy over PCIe - by three
launches over a list of item indices (csrc/batch.hip: care_batch_text, care_batch_frame_ids, care_batch_gather).  MSRVTT is
10 000 videos x 60 frames x 2688 floats = 6.5 GB in fp32 against 288 GB of HBM; an epoch moves one index permutation over
the link and nothing else.  `care_amd.data` (load_video_feats, collate_feats, FeaturePrefetcher) stays for host-fed use.

**Ingestion** (once, on the host, plumbing).  `databases` is what `data.load_video_feats` takes: {modality char: [Mapping
video name -> array, ...]}.  Per modality one `[n_videos, n_total_m, dim_m]` tensor on the device, its row pitch padded to a
multiple of 16 bytes:
  * several tables of a modality are concatenated on the channel axis (dataloader.py:260);
  * a 1-D per-video vector is repeated over the frames of the 2-D tables beside it, and a modality of 1-D vectors alone is
    n_total_m = 1, which every frame id reads (:247-251);
  * a video missing from a table is zeros (:243-244);
  * `r` holds the first `retrieval_topk` rows; its frame ids are 0 .. topk - 1 whatever the mode (:808-814).
`dtype` is fp32 or a 16-bit type the engine accepts from a loader; values are rounded ONCE, here, and a batch is a copy of
stored bytes.  `t` is refused as `data.py` refuses it, `load_feats_type != 0` by name.

**Captions** (optional) are `info_corpus`'s {video name: [[BOS, ..., EOS], ...]}: flat int32 tokens with offsets, a caption ->
video and a video -> first-caption array.  A video without a caption, or a caption that does not start with BOS and end with
EOS, is refused (the reference asserts the same, utils_corpora.py:432-433).  A store without captions serves `feats`,
`frame_ids` and `video_ids` only, and its items are the videos.

**Items** (dataloader.py:389-453).  `train`: the (video, caption) pairs of the infoset - every caption when
`opt["n_caps_per_video"]` is 0, else min(k, captions) of each video drawn once from RandomState(opt["seed"]).  `validate` /
`test`: every video with its caption 0 (:418-419), frames equally sampled (:713-715).

**Random numbers** are counter-based (h = care_mix64 of csrc/care_common.h, `captions.mix64` here): an item's frames depend
on (seed, epoch, the item's index in the infoset) alone - not on the batch or the batch size it falls into - and `loader`
visits the `train` items of an epoch in ascending (h(item key, 0xFFFFFFFF), item).  The reference draws from numpy's / Python's global generators; its streams cannot
be reproduced, the distributions and every deterministic rule are.

There is no CPU fallback: a store built with device=None holds the host tables only (what the tests of the ingestion rules
read) and cannot build a batch.
"""
import ctypes
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .captions import mix64 as _mix
from .constants import BOS, EOS, PAD
from .data import N_TOTAL_FRAMES

__all__ = ["ClipStore"]

ATTRIBUTE_START, ATTRIBUTE_END = 6, 3006   # config/Constants.py:15-16
MODES = ("train", "validate", "test")
SHUFFLE = 0xFFFFFFFF                        # the counter of an item's place in the epoch's order (no frame has it)
_U = np.uint64


def snippet_bounds(n_total: int, n_frames: int):
    """The n_frames + 1 snippet bounds, by the reference's own expression (misc/utils.py:313): the float arithmetic is numpy's."""
    return [int(i) for i in np.linspace(0, n_total, n_frames + 1)]


def epoch_order(n_items: int, seed: int, epoch: int) -> np.ndarray:
    """int32 [n_items]: the items in ascending (h(h(h(seed, epoch), item), SHUFFLE), item)."""
    items = np.arange(n_items, dtype=_U)
    keys = _mix(_mix(_mix(_U(seed & (2 ** 64 - 1)), _U(epoch & (2 ** 64 - 1))), items), _U(SHUFFLE))
    return np.lexsort((items, keys)).astype(np.int32)


def ingest_modality(tables: Sequence[Mapping], names: Sequence[str], dim: int, n_total_frames: Optional[int] = None) -> np.ndarray:
    """fp32 [n_videos, n_total, dim] of one frame modality (dataloader.py:232-262, load_feats_type 0)."""
    per_video, n_total = [], None
    for vid in names:
        if any(vid not in t for t in tables):
            per_video.append(None)       # :243-244
            continue
        parts = [np.asarray(t[vid]) for t in tables]
        if any(p.ndim not in (1, 2) for p in parts):
            raise ValueError("{}: a feature table entry must be [frames, dim] or [dim], got shapes {}".format(vid, [p.shape for p in parts]))
        lens = {p.shape[0] for p in parts if p.ndim == 2}
        if len(lens) > 1:
            raise ValueError("{}: tables of one modality with {} frames cannot be concatenated".format(vid, sorted(lens)))
        n = lens.pop() if lens else 1
        feats = np.concatenate([p[np.newaxis, :].repeat(n, axis=0) if p.ndim == 1 else p for p in parts], axis=1)
        if feats.shape[1] != dim:
            raise ValueError("{}: {} channels, the option says {}".format(vid, feats.shape[1], dim))
        if n_total is not None and n != n_total:
            raise ValueError("{}: {} frames where earlier videos have {}".format(vid, n, n_total))
        n_total = n
        per_video.append(feats)
    if n_total is None:
        n_total = n_total_frames or N_TOTAL_FRAMES
    out = np.zeros((len(names), n_total, dim), dtype=np.float32)
    for i, f in enumerate(per_video):
        if f is not None:
            out[i] = f
    return out


def ingest_retrieval(table: Mapping, names: Sequence[str], dim: int, topk: int) -> np.ndarray:
    """fp32 [n_videos, topk, dim]: the first `retrieval_topk` rows (dataloader.py:808-814)."""
    out = np.zeros((len(names), topk, dim), dtype=np.float32)
    for i, vid in enumerate(names):
        if vid not in table:
            raise KeyError("{} is not in the retrieval table (load_r_feats has no rule for a missing video)".format(vid))
        rows = np.asarray(table[vid])[:topk, :]
        if rows.shape != (topk, dim):
            raise ValueError("{}: retrieval rows {} where [{}, {}] are needed".format(vid, rows.shape, topk, dim))
        out[i] = rows
    return out


class _Table(object):
    """One modality on the device: `data` [n_videos, n_total, pitch / elemsize] and what care_batch_table says of it."""

    def __init__(self, host: np.ndarray, dtype, device, block: bool):
        n_videos, n_total, dim = host.shape
        es = torch.empty(0, dtype=dtype).element_size()
        self.shape_out = (n_total, dim) if block else (None, dim)    # block: one [topk, dim] block a video (`r`)
        if block:
            host = host.reshape(n_videos, 1, n_total * dim)
        self.n_total, self.row_elems = host.shape[1], host.shape[2]
        self.row_bytes = self.row_elems * es
        self.pitch = -(-self.row_bytes // 16) * 16
        padded = torch.zeros(n_videos, self.n_total, self.pitch // es, dtype=dtype)
        padded[:, :, : self.row_elems] = torch.from_numpy(host).to(dtype)    # the ONE rounding
        self.block = block
        self.data = padded if device is None else padded.to(device)

    def rows(self) -> torch.Tensor:
        """The stored values without the pitch padding, [n_videos, n_total, dim] ([n_videos, topk, dim] for `r`)."""
        x = self.data[:, :, : self.row_elems]
        return x.reshape(x.shape[0], *self.shape_out) if self.block else x


class ClipStore(object):
    def __init__(self, opt, databases: Dict[str, Sequence[Mapping]], video_names: Sequence[str], captions: Optional[Mapping] = None,
                 dtype=torch.float32, device="cuda", n_attributes: Optional[int] = None, n_total_frames: Optional[int] = None):
        if opt.get("load_feats_type", 0) != 0:
            raise NotImplementedError("load_feats_type {}: the clip store restates load_feats_type 0 (frames picked by id from "
                                      "fixed-length tables)".format(opt["load_feats_type"]))
        if opt.get("decoding_type", "ARFormer") != "ARFormer":
            raise NotImplementedError("decoding_type {!r}: the clip store builds ARFormer source / target pairs, not NARFormer "
                                      "masks".format(opt["decoding_type"]))
        if opt.get("visual_word_generation", False):
            raise NotImplementedError("visual_word_generation: the clip store builds one source / target pair per item")
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise TypeError("`dtype` must be torch.float32 or a 16-bit type the engine accepts from a loader, got {}".format(dtype))
        self.opt, self.dtype = opt, dtype
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("a clip store on {}: batches are built on the MI355X (no CPU fallback; device=None keeps the host "
                               "tables only)".format(self.device))
        self.video_names = list(video_names)
        self.n_videos = len(self.video_names)
        if self.n_videos < 1:
            raise ValueError("a clip store needs at least one video")
        self.modality = opt["modality"].lower()
        self.n_frames, self.max_len = int(opt["n_frames"]), int(opt.get("max_len", 30))
        self.random_type = opt.get("random_type", "segment_random")
        if self.random_type not in _lib.FRAME_TYPES:
            raise ValueError("We do not support `random_type` = {} now".format(self.random_type))   # dataloader.py:31
        self.n_attributes = ATTRIBUTE_END - ATTRIBUTE_START if n_attributes is None else int(n_attributes)
        if not 1 <= self.n_attributes <= ATTRIBUTE_END - ATTRIBUTE_START:
            raise ValueError("`n_attributes` must lie in [1, {}], got {}".format(ATTRIBUTE_END - ATTRIBUTE_START, self.n_attributes))
        if len(self.modality) > _lib.BATCH_MAX_TABLES:
            raise NotImplementedError("{} modalities: care_batch_gather takes {} tables a launch".format(len(self.modality), _lib.BATCH_MAX_TABLES))
        if not 1 <= self.n_frames <= _lib.BATCH_MAX_FRAMES:
            raise NotImplementedError("n_frames {}: care_batch_frame_ids takes 1 .. {}".format(self.n_frames, _lib.BATCH_MAX_FRAMES))

        # ---- the feature tables
        self.tables = []
        for ch in self.modality:
            if ch == "t":
                raise ValueError("retrieved-caption token inputs (`t`) belong to the pointer network, out of scope")
            if ch == "r":
                host = ingest_retrieval(databases[ch][0], self.video_names, int(opt["dim_r"]), int(opt["retrieval_topk"]))
            else:
                host = ingest_modality(databases[ch], self.video_names, int(opt["dim_" + ch]), n_total_frames)
            self.tables.append(_Table(host, dtype, self.device, block=(ch == "r")))
        framed = {t.n_total for t in self.tables if not t.block and t.n_total > 1}
        if len(framed) > 1:
            raise ValueError("the modalities have {} frames a video: one list of frame ids serves them all".format(sorted(framed)))
        self.n_total = framed.pop() if framed else int(n_total_frames or N_TOTAL_FRAMES)
        if n_total_frames is not None and self.n_total != int(n_total_frames):
            raise ValueError("the tables have {} frames a video, `n_total_frames` says {}".format(self.n_total, n_total_frames))
        if self.random_type != "equally_sampling" and self.n_frames > self.n_total:
            raise NotImplementedError("random_type {!r} with n_frames {} > {} frames a video: the reference's draw raises".format(
                self.random_type, self.n_frames, self.n_total))
        if self.random_type == "all_random" and self.n_total > 64:
            raise NotImplementedError("random_type 'all_random' with {} frames a video: care_batch_frame_ids ranks one wave of 64 "
                                      "frames".format(self.n_total))
        self.bounds = snippet_bounds(self.n_total, self.n_frames)
        self._bounds_c = (ctypes.c_int32 * (self.n_frames + 1))(*self.bounds)

        # ---- the caption table and the infosets
        self.has_captions = captions is not None
        self._items = {}
        if self.has_captions:
            self._ingest_captions(captions)
        else:
            ident = torch.arange(self.n_videos, dtype=torch.int32)
            for mode in MODES:
                self._items[mode] = ident
        if self.device is not None:
            self._items = {m: t.to(self.device) for m, t in self._items.items()}
        self._rings = {}

    def _ingest_captions(self, captions: Mapping) -> None:
        tokens, cap_start, cap_video, vid_first = [], [0], [], [0]
        for v, vid in enumerate(self.video_names):
            caps = captions.get(vid) if hasattr(captions, "get") else captions[vid]
            if not caps:
                raise ValueError("{} has no caption".format(vid))
            for c, cap in enumerate(caps):
                cap = [int(w) for w in cap]
                if len(cap) < 2 or cap[0] != BOS or cap[-1] != EOS:
                    raise ValueError("caption {} of {} does not start with BOS and end with EOS".format(c, vid))
                if min(cap) < 0 or max(cap) >= 2 ** 31:
                    raise ValueError("caption {} of {} holds a token outside int32".format(c, vid))
                tokens += cap
                cap_start.append(len(tokens))
                cap_video.append(v)
            vid_first.append(len(cap_video))
        if len(tokens) >= 2 ** 31:
            raise NotImplementedError("{} caption tokens: the offsets are int32".format(len(tokens)))
        host = {"tokens": tokens, "cap_start": cap_start, "cap_video": cap_video, "vid_first": vid_first}
        self.host_captions = {k: np.asarray(a, dtype=np.int32) for k, a in host.items()}
        self.n_caps = len(cap_video)
        # the infosets (dataloader.py:416-426)
        k = int(self.opt.get("n_caps_per_video", 0))
        if k < 0:
            raise ValueError("n_caps_per_video must be >= 0")   # dataloader.py:305
        first = self.host_captions["vid_first"]
        if k == 0:
            train = np.arange(self.n_caps, dtype=np.int32)
        else:
            rng, train = np.random.RandomState(self.opt.get("seed", 0)), []
            for v in range(self.n_videos):
                n = int(first[v + 1] - first[v])
                train += [int(first[v]) + int(i) for i in rng.choice(list(range(n)), min(n, k), replace=False)]
            train = np.asarray(train, dtype=np.int32)
        self._items["train"] = torch.from_numpy(train)
        self._items["validate"] = self._items["test"] = torch.from_numpy(first[:-1].copy())
        self.captions_dev = None
        if self.device is not None:
            self.captions_dev = {k_: torch.from_numpy(a).to(self.device) for k_, a in self.host_captions.items()}

    # ------------------------------------------------------------------------------------------------------------ the items
    def n_items(self, mode: str = "train") -> int:
        return int(self._check_mode(mode).numel())

    def item_captions(self, mode: str = "train") -> torch.Tensor:
        """int32 [n_items]: with captions the index of every item's caption in the flat caption table; without, the video."""
        return self._check_mode(mode)

    def _check_mode(self, mode: str) -> torch.Tensor:
        if mode not in MODES:
            raise ValueError("`mode` must be one of {}, got {!r}".format(MODES, mode))
        return self._items[mode]

    # ------------------------------------------------------------------------------------------------------------- a batch
    def new_slot(self, batch_size: int) -> dict:
        """Device tensors a batch of up to `batch_size` items is written into (`batch(..., out=slot)`, the loader's ring)."""
        self._need_device()
        dev, B = self.device, int(batch_size)
        slot = {"feats": [], "frame_ids": torch.empty(B, self.n_frames, dtype=torch.int32, device=dev),
                "video_ids": torch.empty(B, dtype=torch.int32, device=dev)}
        for t in self.tables:
            n = t.shape_out[0] if t.block else self.n_frames
            slot["feats"].append(torch.empty(B, n, t.shape_out[1], dtype=self.dtype, device=dev))
        if self.has_captions:
            slot["caption_ids"] = torch.empty(B, dtype=torch.int32, device=dev)
            slot["input_ids"] = torch.empty(B, self.max_len - 1, dtype=torch.int64, device=dev)
            slot["labels"] = torch.empty(B, self.max_len - 1, dtype=torch.int64, device=dev)
            slot["labels_attr"] = torch.empty(B, self.n_attributes, dtype=torch.float32, device=dev)
        return slot

    def _need_device(self) -> None:
        if self.device is None:
            raise RuntimeError("this store was built with device=None (host tables only): batches are built on the MI355X (no CPU fallback)")

    def batch(self, items, mode: str = "train", epoch: int = 0, seed: int = 0, out: Optional[dict] = None) -> dict:
        """The batch of the infoset items `items` (a sequence of indices into the mode's infoset, or an int32 tensor on the
        device, which is not read on the host): a dict of device tensors - `feats` [B, n, dim] per modality in
        opt["modality"] order, `frame_ids` int32 [B, n_frames], `video_ids` int32 [B] (the store's video rows), and with
        captions `caption_ids` int32 [B], `input_ids` / `labels` int64 [B, max_len - 1], `labels_attr` fp32 [B, n_attributes].
        `out`: a slot of new_slot(>= B) to write into; the returned tensors are its first B rows.  Nothing synchronises."""
        self._need_device()
        item_cap = self._check_mode(mode)
        if isinstance(items, torch.Tensor):
            if items.dtype != torch.int32 or items.dim() != 1 or items.device != self.device or not items.is_contiguous():
                raise TypeError("`items` as a tensor must be contiguous int32 [B] on {}, got {} {} on {}".format(
                    self.device, items.dtype, tuple(items.shape), items.device))
        else:
            host = np.asarray(list(items), dtype=np.int64).reshape(-1)
            if host.size and (host.min() < 0 or host.max() >= item_cap.numel()):
                raise IndexError("`items` outside the {} items of mode {!r}".format(item_cap.numel(), mode))
            items = torch.from_numpy(host.astype(np.int32)).to(self.device)
        B = int(items.numel())
        slot = out if out is not None else self.new_slot(B)
        if slot["video_ids"].shape[0] < B:
            raise ValueError("`out` holds {} items, the batch has {}".format(slot["video_ids"].shape[0], B))
        res = {k: ([f[:B] for f in v] if k == "feats" else v[:B]) for k, v in slot.items()}
        ptr = _lib.ptr
        with torch.cuda.device(self.device):
            if self.has_captions:
                c = self.captions_dev
                _lib.call("care_batch_text", ptr(items), B, ptr(item_cap), int(item_cap.numel()), ptr(c["tokens"]), ptr(c["cap_start"]),
                          ptr(c["cap_video"]), ptr(c["vid_first"]), self.n_caps, self.n_videos, self.max_len, PAD, EOS,
                          ATTRIBUTE_START, self.n_attributes, ptr(res["video_ids"]), ptr(res["caption_ids"]), ptr(res["input_ids"]),
                          ptr(res["labels"]), ptr(res["labels_attr"]), tag="batch_text")
            else:
                res["video_ids"].copy_(items)
            rt = _lib.FRAME_TYPES[self.random_type if mode == "train" else "equally_sampling"]   # dataloader.py:713-717
            _lib.call("care_batch_frame_ids", ptr(items), B, self.n_total, self.n_frames, rt, self._bounds_c,
                      int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), ptr(res["frame_ids"]), tag="batch_frame_ids")
            descs = (_lib.BatchTable * len(self.tables))()
            for d, t, o in zip(descs, self.tables, res["feats"]):
                d.table, d.out, d.pitch = t.data.data_ptr(), o.data_ptr(), t.pitch
                d.n_total, d.row_bytes, d.n_out = t.n_total, t.row_bytes, (1 if t.block else self.n_frames)
            _lib.call("care_batch_gather", descs, len(self.tables), ptr(res["video_ids"]), ptr(res["frame_ids"]), self.n_videos, B,
                      self.n_frames, tag="batch_gather")
        return res

    def loader(self, mode: str = "train", batch_size: int = 512, epoch: int = 0, seed: int = 0, depth: int = 2,
               shard: Optional[Sequence[int]] = None):
        """One epoch of batches, as an iterable that can be walked more than once (`len()` = its number of batches).  `train`
        items are visited in the epoch's permutation (one small H2D copy a walk), the other modes as they lie; the last batch
        may be short; shard = (rank, world) takes every world-th batch, the rank-th first.

        The batches are written into a ring of `depth` slots that the store keeps per (batch_size, depth): batch k and batch
        k + depth have the same addresses - across epochs too - so the engine's captured graphs replay.  A YIELDED BATCH IS
        OVERWRITTEN `depth` BATCHES LATER: consume it (on the stream it was built on) before asking for the depth-th batch
        behind it, or clone what must live longer.  Do not collect the batches in a list."""
        return _Loader(self, mode, batch_size, epoch, seed, depth, shard)


class _Loader(object):
    def __init__(self, store, mode, batch_size, epoch, seed, depth, shard):
        store._need_device()
        self.store, self.mode, self.epoch, self.seed = store, mode, int(epoch), int(seed)
        self.n = store.n_items(mode)
        self.batch_size, self.depth = int(batch_size), int(depth)
        if self.batch_size < 1 or self.depth < 1:
            raise ValueError("batch_size and depth must be >= 1")
        self.rank, self.world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
        if not 0 <= self.rank < self.world:
            raise ValueError("shard = (rank, world) needs 0 <= rank < world, got {}".format((self.rank, self.world)))

    def __len__(self):
        total = -(-self.n // self.batch_size)
        return len(range(self.rank, total, self.world))

    def __iter__(self):
        store = self.store
        if self.mode == "train":
            order = torch.from_numpy(epoch_order(self.n, self.seed, self.epoch)).to(store.device)
        else:
            order = torch.arange(self.n, dtype=torch.int32, device=store.device)
        ring = store._rings.setdefault((self.batch_size, self.depth), [None] * self.depth)
        k = 0
        for b, start in enumerate(range(0, self.n, self.batch_size)):
            if b % self.world != self.rank:
                continue
            if ring[k % self.depth] is None:
                ring[k % self.depth] = store.new_slot(self.batch_size)
            yield store.batch(order[start: start + self.batch_size], mode=self.mode, epoch=self.epoch, seed=self.seed,
                              out=ring[k % self.depth])
            k += 1

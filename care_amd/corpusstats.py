"""The caption analysis of the reference's test run on the MI355X (csrc/corpus_stats.hip): `ave_length`, `novel`, `unique`, `usage`.

    from care_amd.corpusstats import CorpusBank, EpochCaptions
    corpus = CorpusBank(train_captions, vocab_size)          # the training captions, ids without BOS / EOS (tmp[1:-1])
    epoch = EpochCaptions(4096, vocab_size, corpus)          # room for 4096 captions, a power of two
    for tokens, length in decoded_batches:                   # device tensors, e.g. fed[:, 1:], length of translate_greedy
        epoch.insert(tokens, length)
    analysis = epoch.totals()                                # the ONE host read: ave_length, novel, unique, usage

What `analyze_length_novel_unique` (misc/utils.py:406-419, the live definition) returns for the captions `to_sentence` makes of
an epoch's predictions (misc/utils.py:117-137: a token row cut at the first EOS or PAD), over token ids instead of words:
    ave_length = the mean number of words - an EMPTY caption counts one, ''.split(' ') being [''];
    unique     = distinct captions / captions;
    novel      = distinct captions that no training caption equals / captions - the empty caption is novel unless a training
                 caption is empty too;
    usage      = distinct words in the captions, the empty word of an empty caption included.
All four come from five integers that `care_corpus_insert` keeps on the device (an open-addressing set of the epoch's captions,
a bitmap of the vocabulary, a sorted table of the distinct training captions) - exact whatever the split into batches, with
the divisions done on the host by Python's `/`, so the floats are the reference's bits.  tests/corpus_reference.py restates the
analysis with dicts and sets.

Ids and words: the reference's corpus stores ids, an out-of-vocabulary word as `<unk>` - cal_gt_n_gram reads those ids, so a
bank built from ids is the faithful one: `<unk>` equals `<unk>`.  `CorpusBank.from_words` takes words and gives every word
outside the vocabulary an id of its own above it, like `MetricBank.from_words`; a caption that holds one can equal no
prediction.  Two ids that spell the same word count as two words.  As everywhere in care_amd there is no CPU fallback.
"""
import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .constants import EOS, PAD
from .captions import MAX_CAPTION, MAX_VOCAB, caption_rows, mix64, number_words, upload

__all__ = ["CorpusBank", "EpochCaptions", "caption_key", "caption_keys", "analysis", "ALL_ONES", "TOTAL_NAMES"]

ALL_ONES = (1 << 64) - 1
TOTAL_NAMES = ("n_captions", "length_sum", "n_distinct", "n_novel", "n_empty", "usage", "n_overflow")   # care_hip.h: CARE_CORPUS_*


def caption_keys(captions: Sequence[Sequence[int]], key_mask: int = ALL_ONES) -> np.ndarray:
    """uint64 [len(captions)]: the key csrc/corpus_stats.hip gives each caption (a sequence of ids, already cut) -
    (h(n, 64) + sum_j h(token_j, j)) & key_mask in uint64 with wrap-around, h = captions.mix64."""
    lens = np.asarray([len(c) for c in captions], dtype=np.int64)
    with np.errstate(over="ignore"):
        keys = mix64(lens, np.full(lens.size, 64, dtype=np.uint64))
        if lens.sum():
            flat = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in captions]).astype(np.uint64)
            owner = np.repeat(np.arange(lens.size), lens)
            pos = (np.arange(flat.size) - np.repeat(np.cumsum(lens) - lens, lens)).astype(np.uint64)
            np.add.at(keys, owner, mix64(flat, pos))
    return keys & np.uint64(key_mask)


def caption_key(caption: Sequence[int], key_mask: int = ALL_ONES) -> int:
    return int(caption_keys([list(caption)], key_mask)[0])


def analysis(ints: Dict[str, int]) -> Dict[str, float]:
    """The four numbers of the reference from the integer totals, by its own divisions (misc/utils.py:403, :415-417)."""
    n = int(ints["n_captions"])
    if n < 1:
        raise ValueError("no caption was inserted: the analysis of an empty epoch divides by zero (as the reference's does)")
    return {"ave_length": int(ints["length_sum"]) / n, "novel": int(ints["n_novel"]) / n, "unique": int(ints["n_distinct"]) / n,
            "usage": int(ints["usage"])}


class CorpusBank(object):
    """cal_gt_n_gram's `gt_sents` (misc/utils.py:375-387) as a device table: the DISTINCT training captions - each a sequence of
    ids WITHOUT BOS and EOS, the reference's tmp[1:-1], taken whole - sorted by key, with offsets into one token pool.
    device None keeps the host tables (`host`) only, like MetricBank.  key_mask: ANDed onto every key (tests)."""

    def __init__(self, train_captions: Sequence[Sequence[int]], vocab_size: int, device="cuda", key_mask: int = ALL_ONES):
        if not isinstance(vocab_size, int) or vocab_size < 1:
            raise ValueError("`vocab_size` must be a positive integer, got {!r}".format(vocab_size))
        if vocab_size > MAX_VOCAB:
            raise ValueError("`vocab_size` {} > {}: the vocabulary bitmap holds {} ids".format(vocab_size, MAX_VOCAB, MAX_VOCAB))
        if not 0 <= int(key_mask) <= ALL_ONES:
            raise ValueError("`key_mask` must fit 64 bits, got {!r}".format(key_mask))
        self.vocab_size, self.key_mask = vocab_size, int(key_mask)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("`device` is `{}`: the bank lives on the MI355X (no CPU fallback)".format(self.device))
        self.extra_words = {}
        distinct = sorted({tuple(int(t) for t in c) for c in train_captions})
        for c in distinct:
            if c and (min(c) < 0 or max(c) >= vocab_size):
                raise ValueError("a training caption holds a token outside [0, vocab_size = {})".format(vocab_size))
        self.n_train, self.n = len(train_captions), len(distinct)
        keys = caption_keys(distinct, self.key_mask) if distinct else np.zeros(0, dtype=np.uint64)
        order = np.argsort(keys, kind="stable")   # (equal keys stay in the captions' own order)
        self.captions = [distinct[i] for i in order.tolist()]
        start = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(np.asarray([len(c) for c in self.captions], dtype=np.int64), out=start[1:])
        tokens = np.asarray([t for c in self.captions for t in c], dtype=np.int32)
        self.host = {"keys": keys[order], "start": start, "tokens": tokens}
        self.dev = self.desc = None
        if self.device is None:
            return

        self.dev = {k: upload(a, self.device) for k, a in self.host.items()}
        self.desc = _lib.CorpusBankDesc()
        for k, t in self.dev.items():
            setattr(self.desc, k, t.data_ptr())
        self.desc.n, self.desc.key_mask = self.n, self.key_mask

    @classmethod
    def from_words(cls, train_words: Sequence[Sequence[str]], word_to_id: dict, vocab_size: Optional[int] = None, device="cuda",
                   key_mask: int = ALL_ONES) -> "CorpusBank":
        """A bank from training captions given as lists of WORDS, as MetricBank.from_words numbers them: a word of the model's
        vocabulary (`word_to_id`) gets its id, every other word a fresh id from `vocab_size` upwards - `bank.extra_words`; the
        bank's vocab_size grows by their number (a TestEpoch wants it equal to its MetricBank's: build both from ids when the
        two word sets differ).  More than 65536 ids: a ValueError."""
        caps, extra, total = number_words(train_words, word_to_id, vocab_size)
        bank = cls(caps, total, device=device, key_mask=key_mask)
        bank.extra_words = extra
        return bank

    def __contains__(self, caption) -> bool:
        """Whether a training caption equals `caption` (ids): the kernel's lookup on the host tables."""
        cap = tuple(int(t) for t in caption)
        k = np.uint64(caption_key(cap, self.key_mask))
        i = int(np.searchsorted(self.host["keys"], k, side="left"))
        while i < self.n and self.host["keys"][i] == k:
            if self.captions[i] == cap:
                return True
            i += 1
        return False


def _is_pow2(n) -> bool:
    return isinstance(n, int) and n >= 1 and (n & (n - 1)) == 0


class EpochCaptions(object):
    """The captions of one epoch on the bank's device: a store of `capacity` rows (a power of two: it is the size of the
    open-addressing table as well), the vocabulary bitmap and the totals.  `insert` per batch, `totals` at the end (the one
    read), `reset` before the next epoch."""

    def __init__(self, capacity: int, vocab_size: int, bank: CorpusBank, variant: str = ""):
        if not isinstance(bank, CorpusBank):
            raise TypeError("`bank` must be a care_amd.CorpusBank, got {}".format(type(bank).__name__))
        if not _is_pow2(capacity):
            raise ValueError("`capacity` must be a power of two (the table's slots), got {!r}".format(capacity))
        if vocab_size != bank.vocab_size:
            raise ValueError("`vocab_size` {} != the corpus bank's {}".format(vocab_size, bank.vocab_size))
        if bank.desc is None:
            raise RuntimeError("the corpus bank was built with device=None (host tables only): the analysis runs on the MI355X")
        self.capacity, self.vocab_size, self.bank, self.device = capacity, vocab_size, bank, bank.device
        self.variant = variant   # the library the launches go to (the kernels hold no 16-bit type: both behave alike)
        dev = self.device
        self.slots = torch.empty(capacity, dtype=torch.int32, device=dev)
        self.tokens = torch.zeros(capacity, MAX_CAPTION, dtype=torch.int32, device=dev)
        self.length = torch.zeros(capacity, dtype=torch.int32, device=dev)
        self.keys = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.bitmap = torch.zeros(_lib.CORPUS_BITMAP_WORDS, dtype=torch.int32, device=dev)
        self._totals = torch.zeros(_lib.CORPUS_TOTALS, dtype=torch.int64, device=dev)
        self.desc = _lib.EpochSetDesc()
        for k, t in (("slots", self.slots), ("tokens", self.tokens), ("length", self.length), ("keys", self.keys),
                     ("bitmap", self.bitmap), ("totals", self._totals)):
            setattr(self.desc, k, t.data_ptr())
        self.desc.capacity, self.desc.key_mask = capacity, bank.key_mask
        self.cursor = 0
        self.reset()

    def reset(self) -> None:
        """An empty epoch: every slot -1, the bitmap and the totals zero, the cursor at row 0.  Nothing is read."""
        self.slots.fill_(-1)
        self.bitmap.zero_()
        self._totals.zero_()
        self.cursor = 0

    def insert(self, tokens: torch.Tensor, length: torch.Tensor, offset: int = 0, keys_out: Optional[torch.Tensor] = None) -> int:
        """Adds caption r = tokens[r, offset : offset + length[r]], cut at the first EOS or PAD, for every row: two launches,
        nothing is waited for.  tokens: int32 [rows, width <= 64 behind the offset] with unit stride in the last dimension and
        any row stride (the rules of MetricBank.score).  Returns the store row of the batch's first caption."""
        rows, width, ld, length = caption_rows(tokens, length, offset, "care_corpus_insert")
        if self.cursor + rows > self.capacity:
            raise ValueError("{} captions after {}: the epoch is larger than its capacity {}".format(rows, self.cursor, self.capacity))
        if keys_out is not None and (keys_out.dtype != torch.int64 or keys_out.numel() != rows or not keys_out.is_contiguous()
                                     or keys_out.device != tokens.device):
            raise ValueError("`keys_out` must be a contiguous int64 tensor of {} words on the device".format(rows))
        first = self.cursor
        with torch.cuda.device(tokens.device):
            _lib.call("care_corpus_insert", _lib.ptr(tokens), ld, int(offset), width, _lib.ptr(length), rows, first, EOS, PAD,
                      ctypes.addressof(self.bank.desc), ctypes.addressof(self.desc), _lib.ptr(keys_out), tag="corpus_insert", variant=self.variant)
        self.cursor = first + rows
        return first

    def totals_device(self) -> torch.Tensor:
        """int64 [8] on the device after care_corpus_totals (TOTAL_NAMES and a spare word); nothing is read."""
        with torch.cuda.device(self.device):
            _lib.call("care_corpus_totals", ctypes.addressof(self.desc), tag="corpus_totals", variant=self.variant)
        return self._totals

    def totals(self) -> Dict[str, float]:
        """{"ave_length", "novel", "unique", "usage"} as the reference computes them, and the integers they come from
        (TOTAL_NAMES).  The ONE host read of the analysis."""
        host = self.totals_device().cpu().tolist()
        ints = dict(zip(TOTAL_NAMES, (int(v) for v in host)))
        if ints["n_overflow"]:
            raise RuntimeError("{} captions found no slot in the epoch set: its slots were overwritten".format(ints["n_overflow"]))
        out = analysis(ints)
        out.update(ints)
        return out

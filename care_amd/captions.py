"""Host helpers the caption modules share (reward, capmetrics, corpusstats, clipstore) - checks and numpy only, no launch.

The device half is csrc/caption_core.h.  What is written once here: the checks on a batch of caption rows, the upload of a
bank's host table, the numbering of out-of-vocabulary words (MetricBank and CorpusBank must number alike: TestEpoch builds
both), the trailing-EOS strip of a reference, and the library's counter-based hash in numpy (care_mix64 of
csrc/care_common.h, bit for bit).
"""
from typing import Optional, Sequence

import numpy as np
import torch

from .constants import EOS

MAX_CAPTION = 64      # tokens of a candidate caption (csrc/caption_core.h: 250 n-grams in LDS, a token a lane)
MAX_VOCAB = 1 << 16   # 16 bits a token in an n-gram's key
_U = np.uint64


def need_device(t, what: str, who: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError("`{}` must be a tensor, got {}".format(what, type(t).__name__))
    if t.device.type != "cuda":
        raise RuntimeError("`{}` is on `{}`: {} runs on the MI355X (no CPU fallback)".format(what, t.device, who))


def caption_rows(tokens, length, offset: int, who: str, also=()):
    """(rows, width, ld, length) of a batch of captions tokens[r, offset : offset + length[r]] as the entry point `who`
    takes it: int32 device tensors, tokens [rows, width <= 64 behind the offset] with unit stride in the last dimension and
    any row stride, one length a row (returned contiguous).  also: (name, tensor) pairs held to length's rules (`video`)."""
    per_row = (("length", length),) + tuple(also)
    for what, t in (("tokens", tokens),) + per_row:
        need_device(t, what, who)
        if t.dtype != torch.int32:
            raise TypeError("`{}` must be int32, got {}".format(what, t.dtype))
    if tokens.dim() != 2 or tokens.stride(1) != 1:
        raise ValueError("`tokens` must be [rows, width] with unit stride in the last dimension, got shape {} strides {}".format(
            tuple(tokens.shape), tuple(tokens.stride())))
    rows, width = tokens.shape[0], tokens.shape[1] - int(offset)
    if offset < 0 or width < 1:
        raise ValueError("`offset` {} leaves no column of `tokens` {}".format(offset, tuple(tokens.shape)))
    if width > MAX_CAPTION:
        raise ValueError("captions of up to {} tokens: {} holds {}".format(width, who, MAX_CAPTION))
    if any(t.numel() != rows for _, t in per_row):
        raise ValueError("{} must hold one entry per row of `tokens` {}".format(
            " and ".join("`{}` {}".format(what, tuple(t.shape)) for what, t in per_row), tuple(tokens.shape)))
    ld = tokens.stride(0) if rows > 1 else max(tokens.stride(0), tokens.shape[1])   # (a single row may carry any stride)
    return rows, width, ld, length.contiguous()


def upload(array, device, dtype=None) -> torch.Tensor:
    """A host table on the device: uint64 as the same bits in int64, and at least one element, so that no array of a bank is
    a NULL pointer."""
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    t = torch.from_numpy(a.copy())
    return (t if dtype is None else t.to(dtype)).to(device)


def number_words(sequences: Sequence[Sequence[str]], word_to_id: dict, vocab_size: Optional[int]):
    """(ids, extra, total): every sequence of words as ids - a word of the model's vocabulary (`word_to_id`) gets its id,
    every other word a fresh id from `vocab_size` (default: the largest id of `word_to_id` + 1) upwards in order of first
    appearance (`extra`); total = vocab_size + len(extra).  More than 65536 ids in all is a ValueError."""
    if vocab_size is None:
        vocab_size = max(word_to_id.values()) + 1 if word_to_id else 1
    extra, ids = {}, []
    for seq in sequences:
        row = []
        for w in seq:
            i = word_to_id.get(w)
            if i is None:
                i = extra.get(w)
                if i is None:
                    i = extra[w] = vocab_size + len(extra)
            row.append(int(i))
        ids.append(row)
    total = vocab_size + len(extra)
    if total > MAX_VOCAB:
        raise ValueError("{} words outside the model's vocabulary of {}: {} ids in all > {} (an n-gram's key holds 16 bits "
                         "a token)".format(len(extra), vocab_size, total, MAX_VOCAB))
    return ids, extra, total


def strip_eos(toks, with_eos: bool) -> np.ndarray:
    """A reference as int64 ids; its trailing EOS is dropped unless with_eos (then it stays an ordinary token)."""
    toks = np.asarray(list(toks), dtype=np.int64).reshape(-1)
    if toks.size and not with_eos and toks[-1] == EOS:
        toks = toks[:-1]
    return toks


def mix64(a, n):
    """h(a, n) = fin(a + 0x9E3779B97F4A7C15 (n + 1)), fin = the splitmix64 finaliser, on uint64 arrays / scalars with
    wrap-around: care_mix64 of csrc/care_common.h."""
    with np.errstate(over="ignore"):
        z = np.asarray(a, dtype=_U) + _U(0x9E3779B97F4A7C15) * (np.asarray(n, dtype=_U) + _U(1))
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))

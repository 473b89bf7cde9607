"""Consensus selection among a clip's own candidate captions on the MI355X (csrc/consensus.hip).

    from care_amd import consensus_select

`sample_batch` gives several captions per clip; the only ranking the model offers for them is its own log-probability - the
criterion beam search optimises, and the one sampling was added to get away from.  `consensus_select` keeps, per clip, the
candidate that agrees most with the clip's OTHER candidates under the coco-caption CIDEr-D over token ids (minimum Bayes risk
with the task's metric): one launch, a workgroup per clip, the `fed` / `length` device tensors of HipEngine.translate_sample
as they are.  The bank gives the corpus statistics (ln N, ln df) only - no references of the clip are read.  The definition
is in include/care_hip.h (care_consensus_score) and, in float64, in tests/consensus_reference.py.

As everywhere in care_amd there is no CPU fallback: CPU tensors raise.
"""
import ctypes
from typing import Optional

import torch

from . import _lib
from .captions import caption_rows, need_device
from .constants import EOS
from .reward import CiderBank

__all__ = ["consensus_select", "MAX_CANDIDATES"]

MAX_CANDIDATES = 32   # CARE_CONSENSUS_MAX_N: a clip's candidates live in one workgroup's LDS, 4400 bytes each


def consensus_select(tokens: torch.Tensor, length: torch.Tensor, n: int, bank: CiderBank, offset: int = 0,
                     count: Optional[torch.Tensor] = None, pairs: bool = False):
    """(score fp32 [B, n], winner int32 [B], winner_row int32 [B], pairs fp32 [B, n, n] or None) of B clips with n candidate
    rows each: candidate j of clip b is caption b n + j = tokens[b n + j, offset : offset + length[b n + j]] (the rules of
    CiderBank.score: int32, unit stride in the last dimension, any row stride - a view such as fed[:, 1:] is scored in
    place; the trailing-EOS convention is the bank's).  score[b, j]: the CIDEr-D of candidate j with the clip's other valid
    candidates as references; winner[b]: the best j (the lower among equals), winner_row[b] = b n + winner[b]; pairs[b, j, i]:
    what reference i alone gives candidate j.  count (optional, int32 [B]): only the first count[b] candidates of clip b are
    valid (the others score 0; a clip without a valid candidate has winner -1).  No host synchronisation inside."""
    if not isinstance(bank, CiderBank):
        raise TypeError("`bank` must be a care_amd.CiderBank, got {}".format(type(bank).__name__))
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= MAX_CANDIDATES:
        raise ValueError("`n` must be an integer in 1 .. {} (candidates of a clip), got {!r}".format(MAX_CANDIDATES, n))
    if bank.desc is None:
        raise RuntimeError("this bank was built with device=None (host tables only): the consensus is scored on the MI355X")
    if isinstance(tokens, torch.Tensor) and tokens.dim() == 2 and tokens.shape[0] % n:
        raise ValueError("`tokens` holds {} rows: not a multiple of n = {} candidates a clip".format(tokens.shape[0], n))
    rows, width, ld, length = caption_rows(tokens, length, offset, "care_consensus_score")
    B, dev = rows // n, tokens.device
    if count is not None:
        need_device(count, "count", "care_consensus_score")
        if count.dtype != torch.int32 or count.dim() != 1 or count.numel() != B or count.device != dev:
            raise ValueError("`count` must be int32 [{}] on {}, got {} {} on {}".format(B, dev, count.dtype, tuple(count.shape), count.device))
        count = count.contiguous()
    score = torch.empty(B, n, dtype=torch.float32, device=dev)
    winner = torch.empty(B, dtype=torch.int32, device=dev)
    winner_row = torch.empty(B, dtype=torch.int32, device=dev)
    pair = torch.empty(B, n, n, dtype=torch.float32, device=dev) if pairs else None
    with torch.cuda.device(dev):
        _lib.call("care_consensus_score", _lib.ptr(tokens), ld, int(offset), width, _lib.ptr(length), _lib.ptr(count), B, n,
                  int(bank.with_eos), EOS, ctypes.addressof(bank.desc), _lib.ptr(score), _lib.ptr(pair), _lib.ptr(winner),
                  _lib.ptr(winner_row), tag="consensus_score")
    return score, winner, winner_row, pair

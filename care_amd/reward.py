"""The reward and the loss of self-critical sequence training on the MI355X (csrc/reward.hip).

    from care_amd.reward import CiderBank, reward_advantage, self_critical_loss

`CiderBank` holds the reference captions of a corpus in the form care_cider_score reads: the coco-caption CIDEr-D over integer
token ids (restated in float64 in tests/cider_reference.py).  Building the bank is setup - numpy on the host, once: every
n-gram (n = 1..4) packed into one uint64, 16 bits a token with the orders below 4 zero-filled (PAD = 0 never occurs inside a
caption, so the order is implied and nothing collides), `np.unique` for the per-video sets and the document frequencies.
`bank.score` is one launch, a workgroup per candidate, and reads the `fed` / `length` device tensors of
HipEngine.translate_sample / translate_greedy as they are; `reward_advantage` forms advantages against the greedy caption's
reward or the leave-one-out mean of a clip's other samples; `self_critical_loss` is the advantage-weighted log-likelihood

    loss = -(1 / n_live) * sum over live (r, j) of adv[r] * logp[r, j],   logp[r, j] = x[y] - logsumexp(x)

with its backward to the logits.  n_live, the upstream gradient and every reward stay on the device: nothing here waits for it.

As everywhere in care_amd there is no CPU fallback: CPU tensors raise.  A `DeferredLogits` (model.set_fused_head(True)) is
refused by name - the loss is taken over the [N, t, V] logits the fused head never materialises.
"""
import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .captions import MAX_CAPTION, MAX_VOCAB, caption_rows, need_device, strip_eos, upload  # noqa: F401 (the two limits: re-exported)
from .constants import EOS, PAD
from .criterion import DeferredLogits, _seq_rows, _seq_rows_grad

__all__ = ["CiderBank", "reward_advantage", "self_critical_loss", "pack_ngrams", "MAX_CAPTION"]

ORDERS = 4


def pack_ngrams(tokens: Sequence[int], n: int) -> np.ndarray:
    """The n-grams of `tokens`, in caption order, as uint64 keys: token j of an n-gram in bits [16 j, 16 j + 16)."""
    toks = np.asarray(tokens, dtype=np.uint64).reshape(-1)
    m = toks.size - n + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64)
    keys = np.zeros(m, dtype=np.uint64)
    for j in range(n):
        keys |= toks[j: j + m] << np.uint64(16 * j)
    return keys


def key_order(keys: np.ndarray) -> np.ndarray:
    """The order (1..4) of packed keys: the highest non-zero 16-bit group (no token inside a caption is 0)."""
    keys = np.asarray(keys, dtype=np.uint64)
    return ((keys >> np.uint64(16)) != 0).astype(np.int64) + ((keys >> np.uint64(32)) != 0) + ((keys >> np.uint64(48)) != 0) + 1


class CiderBank(object):
    """The reference captions of a corpus, on the device.  refs: one entry per video, each a list of token-id lists (a trailing
    EOS is dropped unless with_eos; then it stays an ordinary token, in the references and in the candidates).  video_ids
    (optional): the name of each entry as the loader's batch["video_ids"] gives it; default: entry i is video i."""

    def __init__(self, refs: Sequence[Sequence[Sequence[int]]], vocab_size: int, with_eos: bool = False, device="cuda",
                 video_ids: Optional[Sequence] = None):
        if not isinstance(vocab_size, int) or vocab_size < 1:
            raise ValueError("`vocab_size` must be a positive integer, got {!r}".format(vocab_size))
        if vocab_size > MAX_VOCAB:
            raise ValueError("`vocab_size` {} > {}: an n-gram's key holds 16 bits a token".format(vocab_size, MAX_VOCAB))
        refs = list(refs)
        if not refs:
            raise ValueError("`refs` is empty: CIDEr-D needs a corpus of at least one video")
        if video_ids is not None and len(video_ids) != len(refs):
            raise ValueError("{} `video_ids` for {} videos".format(len(video_ids), len(refs)))
        self.vocab_size, self.with_eos, self.n_videos = vocab_size, bool(with_eos), len(refs)
        self.device = None if device is None else torch.device(device)   # (None: the host tables only - `host` - nothing to score with)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("`device` is `{}`: the bank lives on the MI355X (no CPU fallback)".format(self.device))
        self._row_of = None if video_ids is None else {v: i for i, v in enumerate(video_ids)}
        if self._row_of is not None and len(self._row_of) != len(refs):
            raise ValueError("`video_ids` holds a name twice")

        # per reference: its caption, the sorted unique keys of all four orders and their counts
        ref_keys, ref_tf, ref_len, vid_start, video_sets = [], [], [], [0], []
        for v, video in enumerate(refs):
            of_video = []
            for ref in video:
                toks = strip_eos(ref, self.with_eos)
                if toks.size and (toks.min() <= PAD or toks.max() >= vocab_size):
                    raise ValueError("video {}: a reference holds a token outside [1, vocab_size = {})".format(v, vocab_size))
                keys = np.concatenate([pack_ngrams(toks, n) for n in range(1, ORDERS + 1)])
                uniq, counts = np.unique(keys, return_counts=True)
                ref_keys.append(uniq)
                ref_tf.append(counts.astype(np.float64))
                ref_len.append(toks.size)
                of_video.append(uniq)
            vid_start.append(len(ref_keys))
            video_sets.append(np.unique(np.concatenate(of_video)) if of_video else np.zeros(0, dtype=np.uint64))
        corpus_keys, df = np.unique(np.concatenate(video_sets), return_counts=True)   # once per video
        corpus_lndf = np.log(np.maximum(1, df).astype(np.float64))
        self.ln_n = math.log(self.n_videos)

        ref_start = np.zeros(len(ref_keys) + 1, dtype=np.int64)
        np.cumsum(np.asarray([k.size for k in ref_keys], dtype=np.int64), out=ref_start[1:])
        all_keys = np.concatenate(ref_keys) if ref_keys else np.zeros(0, dtype=np.uint64)
        all_tf = np.concatenate(ref_tf) if ref_tf else np.zeros(0, dtype=np.float64)
        all_w = all_tf * (self.ln_n - corpus_lndf[np.searchsorted(corpus_keys, all_keys)])
        order = key_order(all_keys)
        ref_norm = np.zeros((len(ref_keys), ORDERS), dtype=np.float64)
        owner = np.repeat(np.arange(len(ref_keys)), np.diff(ref_start))
        np.add.at(ref_norm, (owner, order - 1), all_w * all_w)
        ref_norm = np.sqrt(ref_norm)

        self.host = {"corpus_keys": corpus_keys, "corpus_lndf": corpus_lndf, "df": df, "ref_keys": all_keys, "ref_w": all_w,
                     "ref_start": ref_start, "ref_norm": ref_norm, "ref_len": np.asarray(ref_len, dtype=np.int32),
                     "vid_start": np.asarray(vid_start, dtype=np.int32)}
        self.n_refs = len(ref_keys)

        self.dev = self.desc = None
        if self.device is None:
            return
        dtypes = {"corpus_keys": torch.int64, "corpus_lndf": torch.float64, "ref_keys": torch.int64, "ref_w": torch.float64,
                  "ref_start": torch.int64, "ref_norm": torch.float64, "ref_len": torch.int32, "vid_start": torch.int32}
        self.dev = {k: upload(self.host[k].reshape(-1), self.device, dt) for k, dt in dtypes.items()}
        self.desc = self._desc()

    def _desc(self) -> "_lib.CiderBankDesc":
        d, desc = self.dev, _lib.CiderBankDesc()
        for k in ("corpus_keys", "corpus_lndf", "ref_keys", "ref_w", "ref_start", "ref_norm", "ref_len", "vid_start"):
            setattr(desc, k, d[k].data_ptr())
        desc.n_corpus, desc.n_videos, desc.n_refs, desc.ln_n = int(self.host["corpus_keys"].size), self.n_videos, self.n_refs, self.ln_n
        return desc

    def rows(self, video_ids) -> torch.Tensor:
        """The bank rows (int32, on the bank's device) of a batch's `video_ids`: names through the `video_ids` the bank was
        built with, integers (a list or a tensor, which is not read on the host) as they are."""
        if isinstance(video_ids, torch.Tensor):
            if self._row_of is not None:
                raise TypeError("the bank was built with named `video_ids`: pass the batch's names, not a tensor")
            return video_ids.to(self.device, torch.int32).reshape(-1)
        ids = list(video_ids)
        if self._row_of is not None:
            missing = [v for v in ids if v not in self._row_of]
            if missing:
                raise KeyError("video_ids not in the bank: {}".format(missing[:4]))
            ids = [self._row_of[v] for v in ids]
        rows = torch.tensor([int(v) for v in ids], dtype=torch.int32)
        return rows if self.device is None else rows.to(self.device)

    def score(self, tokens: torch.Tensor, length: torch.Tensor, video: torch.Tensor, out: Optional[torch.Tensor] = None,
              offset: int = 0, bad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [rows]: the CIDEr-D of caption r = tokens[r, offset : offset + length[r]] against the references of bank row
        video[r].  tokens: int32 [rows, width] with unit stride in the last dimension and any row stride - a view such as
        fed[:, 1:] is scored in place.  bad (optional, int32 [1]): the number of rows whose video is outside the bank."""
        if self.desc is None:
            raise RuntimeError("this bank was built with device=None (host tables only): CIDEr-D is scored on the MI355X")
        rows, width, ld, length = caption_rows(tokens, length, offset, "care_cider_score", also=(("video", video),))
        video = video.contiguous()
        if out is None:
            out = torch.empty(rows, dtype=torch.float32, device=tokens.device)
        elif out.dtype != torch.float32 or out.numel() != rows or not out.is_contiguous() or out.device != tokens.device:
            raise ValueError("`out` must be a contiguous fp32 tensor of {} entries on {}".format(rows, tokens.device))
        with torch.cuda.device(tokens.device):
            _lib.call("care_cider_score", _lib.ptr(tokens), ld, int(offset), width, _lib.ptr(length), _lib.ptr(video), rows,
                      int(self.with_eos), EOS, ctypes.addressof(self.desc), _lib.ptr(out), _lib.ptr(bad), tag="cider_score")
        return out


def reward_advantage(reward: torch.Tensor, baseline: Optional[torch.Tensor] = None):
    """(adv fp32 [B, n], stats float64 [2]) of reward [B, n]: adv = reward - baseline[b] with `baseline` [B] (the greedy
    caption's reward), else reward minus the mean of the clip's OTHER n - 1 samples; stats = the mean reward and the mean
    baseline, device doubles."""
    need_device(reward, "reward", "care_reward_advantage")
    if reward.dim() != 2 or reward.dtype != torch.float32:
        raise ValueError("`reward` must be fp32 [clips, samples], got {} {}".format(reward.dtype, tuple(reward.shape)))
    B, n = reward.shape
    if baseline is None and n < 2:
        raise ValueError("the leave-one-out baseline needs n_samples >= 2, got {}".format(n))
    if baseline is not None:
        need_device(baseline, "baseline", "care_reward_advantage")
        if baseline.dtype != torch.float32 or baseline.numel() != B:
            raise ValueError("`baseline` must be fp32 [{}], got {} {}".format(B, baseline.dtype, tuple(baseline.shape)))
        baseline = baseline.contiguous()
    reward = reward.contiguous()
    adv = torch.empty_like(reward)
    stats = torch.empty(2, dtype=torch.float64, device=reward.device)
    with torch.cuda.device(reward.device):
        _lib.call("care_reward_advantage", _lib.ptr(reward), _lib.ptr(baseline), B, n, _lib.ptr(adv), _lib.ptr(stats), tag="reward_adv")
    return adv, stats


class _WeightedLogLik(torch.autograd.Function):
    """-(1 / n_live) sum adv[r] logp[r, j] over the live label positions; the gradient goes to the logits only."""

    @staticmethod
    def forward(ctx, logits, labels32, adv, acc):
        N, t = logits.shape[0], labels32.shape[1]
        logits, src = _seq_rows(logits, t)
        rows, dev = N * t, logits.device
        stats = torch.empty(3, rows, device=dev, dtype=torch.float32)   # max, log sum exp(x - max), logp
        totals = torch.empty(2, device=dev, dtype=torch.float64)        # sum adv logp, n_live
        loss = torch.empty((), device=dev, dtype=torch.float32)
        seq_logp = torch.empty(N, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.call("care_reward_loss_fwd", *src, _lib.ptr(labels32), _lib.ptr(adv), _lib.ptr(stats[0]), _lib.ptr(stats[1]),
                      _lib.ptr(stats[2]), _lib.ptr(totals), _lib.ptr(loss), _lib.ptr(seq_logp), _lib.ptr(acc), rows,
                      tag="reward_loss_fwd")
        ctx.save_for_backward(logits, labels32, adv, stats, totals)
        ctx.mark_non_differentiable(seq_logp, totals)
        return loss, seq_logp, totals

    @staticmethod
    def backward(ctx, g, _gs, _gt):
        logits, labels32, adv, stats, totals = ctx.saved_tensors
        t = labels32.shape[1]
        g = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernel reads it, the host never does
        d, src, dst = _seq_rows_grad(logits, t)
        with torch.cuda.device(logits.device):
            _lib.call("care_reward_loss_bwd", *src, _lib.ptr(labels32), _lib.ptr(adv), _lib.ptr(stats[0]),
                      _lib.ptr(stats[1]), _lib.ptr(totals), _lib.ptr(g), *dst, tag="reward_loss_bwd")
        return d, None, None, None


def self_critical_loss(logits, labels, advantages, acc: Optional[torch.Tensor] = None, return_aux: bool = False):
    """The advantage-weighted log-likelihood of teacher-forced captions as a 0-dim fp32 device tensor under autograd.

    logits fp32 [N, t, V] (or [N, t + 1, V]: the last position is skipped in place, as the language criterion does), labels
    [N, t] with PAD = a dead position, advantages [N].  No label smoothing; an all-PAD batch gives 0 and a zero gradient.
    acc (optional): 2 device doubles that accumulate (loss, n_live) for recorders.  return_aux: also the per-caption sum of
    log-probabilities fp32 [N] and (sum adv logp, n_live) as 2 device doubles."""
    if isinstance(logits, DeferredLogits):
        raise NotImplementedError(
            "`logits` is a DeferredLogits: the fused head (set_fused_head(True)) never materialises the [N, t, V] logits the "
            "self-critical loss is taken over - call set_fused_head(False) on the module")
    for what, t in (("logits", logits), ("labels", labels), ("advantages", advantages)):
        need_device(t, what, "the self-critical loss")
    if logits.dtype != torch.float32:
        raise TypeError("`logits` must be fp32, got {}".format(logits.dtype))
    if logits.dim() != 3 or labels.dim() != 2 or labels.shape[0] != logits.shape[0] or \
            logits.shape[1] not in (labels.shape[1], labels.shape[1] + 1):
        raise ValueError("logits [N, t (+ 1), V] and labels [N, t] expected, got {} and {}".format(tuple(logits.shape), tuple(labels.shape)))
    if advantages.numel() != logits.shape[0]:
        raise ValueError("`advantages` holds {} entries for N = {} captions".format(advantages.numel(), logits.shape[0]))
    if logits.numel() == 0 or labels.numel() == 0:
        raise ValueError("the loss of empty logits {} is undefined".format(tuple(logits.shape)))
    if labels.device != logits.device or advantages.device != logits.device:
        raise RuntimeError("logits are on `{}`, labels on `{}`, advantages on `{}`".format(logits.device, labels.device, advantages.device))
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() < 2 or acc.device != logits.device):
        raise ValueError("`acc` must hold 2 float64 entries on {}".format(logits.device))
    labels32 = labels.to(torch.int32).contiguous()
    adv = advantages.detach().to(torch.float32).reshape(-1).contiguous()
    loss, seq_logp, totals = _WeightedLogLik.apply(logits, labels32, adv, acc)
    return (loss, seq_logp, totals) if return_aux else loss

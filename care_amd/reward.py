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

`self_critical_head_loss` is the same loss with the vocabulary head inside (csrc/head_reward.hip): it takes
the decoder's hidden states and the head's weight - the two halves of a `DeferredLogits` - and runs the projection, the loss
and its backward over the live label positions only, the [N, t, V] logits and their gradient never in memory.  It needs the
number of live positions on the host: the caller's `live`, or one 4-byte read-back.

As everywhere in care_amd there is no CPU fallback: CPU tensors raise.  `self_critical_loss` itself refuses a `DeferredLogits`
(model.set_fused_head(True)) by name - it is taken over the [N, t, V] logits the fused head never materialises.
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

__all__ = ["CiderBank", "reward_advantage", "self_critical_loss", "self_critical_head_loss", "pack_ngrams", "MAX_CAPTION"]

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


class _HeadRewardLoss(torch.autograd.Function):
    """_WeightedLogLik with the vocabulary head inside (Head.py:26-32 + the loss above), over the live label positions only:
    hidden2d [N * tl, d], W [V, d] -> (loss, seq_logp [N], totals [2]); backward -> (dhidden [N * tl, d] with dead rows exactly
    zero, dW [V, d]).  criterion._HeadLoss's products (csrc/gemm_tile.hip, EPI_HEAD_STATS / EPI_HEAD_GRAD with eps = 0); a row's
    weight - its caption's advantage - is linear, so it multiplies the d-wide rows on either side of the gradient's two
    products (care_rows_scale) and never the [R, V] side.  `live`: the number of live label positions when the host knows
    it; None: read back from the device (4 bytes)."""

    @staticmethod
    def forward(ctx, hidden2d, W, labels32, adv, acc, live=None):
        from . import criterion
        from .training import _absmax_slot, _f32c
        call, ptr = _lib.call, _lib.ptr
        N, t = labels32.shape
        d, V = hidden2d.shape[1], W.shape[0]
        tl = hidden2d.shape[0] // N
        assert hidden2d.shape[0] == N * tl and tl >= t and W.shape[1] == d, (tuple(hidden2d.shape), tuple(W.shape), (N, t))
        h, Wc = _f32c(hidden2d), _f32c(W)
        dev, rows = h.device, N * t
        idx = torch.zeros(3, rows, device=dev, dtype=torch.int32)       # live row -> row of h, label position, label
        cnt = torch.empty(2, device=dev, dtype=torch.int32)
        call("care_head_live_rows", ptr(labels32), N, t, tl, V, ptr(idx[0]), ptr(idx[1]), ptr(idx[2]), ptr(cnt))
        R = int(cnt[0].item()) if live is None else int(live)           # the one 4-byte read-back, unless the caller has it
        if not 0 <= R <= rows:
            raise ValueError("`live` = {} for {} label positions".format(R, rows))
        cst = torch.empty(4, max(R, 1), device=dev, dtype=torch.float32)   # max, log sum exp(x - max), logp, weight per LIVE row
        totals = torch.empty(2, device=dev, dtype=torch.float64)           # sum adv logp, n_live
        loss = torch.empty((), device=dev, dtype=torch.float32)
        seq_logp = torch.empty(N, device=dev, dtype=torch.float32)
        if R > 0:   # (an all-PAD batch launches nothing with M = 0)
            h_live = torch.empty(R, d, device=dev, dtype=torch.float32)
            call("care_gather_rows", ptr(h), h.stride(0) * 4, ptr(h_live), d * 4, ptr(idx[0]), R, d * 4)
            ksd, parts = criterion._ceil64(d), (V + 63) // 64
            h_slot, w_slot = _absmax_slot(h_live), _absmax_slot(Wc)
            a2 = torch.empty(R, 2 * ksd, device=dev, dtype=torch.float16)
            w3 = torch.empty(V, 3 * ksd, device=dev, dtype=torch.float16)
            call("care_split_pieces", ptr(h_live), d, R, d, 0, 1, ksd, ptr(a2), 2, h_slot.data_ptr())
            call("care_split_pieces", ptr(Wc), Wc.stride(0), V, d, 0, 1, ksd, ptr(w3), 3, w_slot.data_ptr())
            for a, b in criterion.head_chunks(R):
                n = b - a
                pf = torch.empty(4, n, parts, device=dev, dtype=torch.float32)
                pi = torch.empty(n, parts, device=dev, dtype=torch.int32)
                call("care_gemm_tile_split3_head_stats", ptr(a2[a:]), ptr(w3), h_slot.data_ptr(), w_slot.data_ptr(), ptr(idx[2][a:]),
                     ptr(pf[0]), ptr(pi), ptr(pf[1]), ptr(pf[2]), ptr(pf[3]), n, V, ksd)
                call("care_head_reward_finish", ptr(pf[0]), ptr(pf[1]), ptr(pf[2]), parts, ptr(idx[1][a:]), ptr(adv), t, V, n,
                     ptr(cst[0][a:]), ptr(cst[1][a:]), ptr(cst[2][a:]), ptr(cst[3][a:]), tag="head_reward_finish")
            # W's pieces are not kept for the backward: split again there from the same |max| - the same bits (as _HeadLoss)
            ctx.save_for_backward(h_live, Wc, a2, idx, cst, h_slot, w_slot, totals)
        call("care_head_reward_reduce", ptr(cst[2]), ptr(cst[3]), ptr(idx[1]), R, t, N, ptr(totals), ptr(loss), ptr(seq_logp), ptr(acc),
             tag="head_reward_reduce")
        ctx.R, ctx.h_shape, ctx.w_shape = R, tuple(hidden2d.shape), tuple(W.shape)
        ctx.mark_non_differentiable(seq_logp, totals)
        return loss, seq_logp, totals

    @staticmethod
    def backward(ctx, g, _gs, _gt):
        from . import criterion
        from .training import _absmax_slot, _strided_sum, _x3_slabs
        call, ptr = _lib.call, _lib.ptr
        (rows_h, d), (V, _) = ctx.h_shape, ctx.w_shape
        R, dev = ctx.R, g.device
        need_dh, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)   # (a fill kernel, not a memset node)
        if R == 0:
            return (zeros(rows_h, d) if need_dh else None), (zeros(V, d) if need_dw else None), None, None, None, None
        h_live, Wc, a2, idx, cst, h_slot, w_slot, totals = ctx.saved_tensors
        g32 = g.to(torch.float32).reshape(1).contiguous()   # a device scalar: the kernels read it, the host never does
        gs = torch.empty(1, device=dev, dtype=torch.float32)   # g / n_live: the factor of dl; |gs| bounds it (the weight is not in dl)
        gslot = torch.empty(1, device=dev, dtype=torch.int32)
        call("care_head_reward_gscale", ptr(g32), ptr(totals), ptr(gs), gslot.data_ptr(), tag="head_reward_gscale")
        ksd, ksv = criterion._ceil64(d), criterion._ceil64(V)
        dh_live = torch.empty(R, d, device=dev, dtype=torch.float32) if need_dh else None
        wh = wh_slot = None
        if need_dw:   # w (.) h_live: the B operand of dW = dl^T (w (.) h), pieces from a |max| of its own
            wh = torch.empty(R, d, device=dev, dtype=torch.float32)
            call("care_rows_scale", ptr(h_live), d, ptr(cst[3]), ptr(wh), d, R, d, tag="rows_scale")
            wh_slot = _absmax_slot(wh)
        plan = [(a, b, _x3_slabs(V, d, b - a)) for a, b in criterion.head_chunks(R)]
        terms = sum(s for _, _, s in plan)
        dw_terms, at = None, 0
        for a, b, slabs in plan:   # _HeadLoss.backward's buffers and their order: one of the size of W's pieces or the chunk's at a time
            n = b - a
            w3 = torch.empty(V, 3 * ksd, device=dev, dtype=torch.float16)
            call("care_split_pieces", ptr(Wc), Wc.stride(0), V, d, 0, 1, ksd, ptr(w3), 3, w_slot.data_ptr())
            dl2 = torch.empty(n, 2 * ksv, device=dev, dtype=torch.float16)
            call("care_gemm_tile_split3_head_grad", ptr(a2[a:]), ptr(w3), h_slot.data_ptr(), w_slot.data_ptr(), ptr(idx[2][a:]),
                 ptr(cst[0][a:]), ptr(cst[1][a:]), ptr(gs), gslot.data_ptr(), 0.0, ptr(dl2), n, V, ksd)
            del w3
            if need_dh:   # dl W: W^T as the [d, V] operand, pieces with the forward's |max| of W; the weight follows below
                wt3 = torch.empty(d, 3 * ksv, device=dev, dtype=torch.float16)
                call("care_split_pieces", ptr(Wc), Wc.stride(0), d, V, 1, 1, ksv, ptr(wt3), 3, w_slot.data_ptr())
                call("care_gemm_tile_split3_scaled", ptr(dl2), ptr(wt3), None, ptr(dh_live[a:]), d, n, d, ksv, gslot.data_ptr(),
                     w_slot.data_ptr(), 1)
                del wt3
            if need_dw:   # dW = dl^T (w (.) h): the reduction runs over the chunk's rows, in slabs when the output has few tiles
                ksr = criterion._ceil64((n + slabs - 1) // slabs)
                dlt = torch.empty(slabs * V, 2 * ksr, device=dev, dtype=torch.float16)
                call("care_pieces_transpose", ptr(dl2), n, V, ksv, slabs, ksr, ptr(dlt))
                del dl2
                if dw_terms is None:
                    dw_terms = torch.empty(terms * V, d, device=dev, dtype=torch.float32)
                ht3 = torch.empty(slabs * d, 3 * ksr, device=dev, dtype=torch.float16)
                call("care_split_pieces", ptr(wh[a:]), d, d, n, 1, slabs, ksr, ptr(ht3), 3, wh_slot.data_ptr())
                call("care_gemm_tile_split3_scaled", ptr(dlt), ptr(ht3), None, ptr(dw_terms[at * V:]), d, V, d, ksr, gslot.data_ptr(),
                     wh_slot.data_ptr(), slabs)
                at += slabs
                del dlt, ht3
        dW = None
        if need_dw:   # slabs and chunks added in order: one grouping, the same bits every time
            dW = dw_terms if terms == 1 else _strided_sum(dw_terms, V, terms, 1, V)
        dhid = None
        if need_dh:   # dh = w (.) (dl W), in place, then to its rows: the dead rows stay the zeros of the fill
            call("care_rows_scale", ptr(dh_live), d, ptr(cst[3]), ptr(dh_live), d, R, d, tag="rows_scale")
            dhid = zeros(rows_h, d)
            call("care_scatter_rows", ptr(dh_live), d * 4, ptr(dhid), d * 4, ptr(idx[0]), R, d * 4)
        return dhid, dW, None, None, None, None


def self_critical_head_loss(hidden, weight, labels, advantages, acc: Optional[torch.Tensor] = None, return_aux: bool = False,
                            live: Optional[int] = None):
    """`self_critical_loss` with the vocabulary head inside: the loss of the logits hidden . weight^T that are
    never written, as a 0-dim fp32 device tensor under autograd with gradients to `hidden` and `weight`.

    hidden fp32 [N, t, d] (or [N, t + 1, d]: the last position is dead), weight [V, d] - what a training forward under
    set_fused_head(True) hands over as a DeferredLogits -, labels [N, t] with PAD (or anything outside [1, V)) = a dead
    position, advantages [N].  Head, loss and backward run over the live positions only, as split fp16 products (the `fp16x3`
    form) in chunks of criterion.HEAD_CHUNK_ROWS rows; dead rows of the gradient of `hidden` are exact zeros whatever the dead
    rows of `hidden` hold.  acc / return_aux: as in `self_critical_loss`.  live: the number of live label positions if the
    caller has it on the host; None: it is read back from the device - 4 bytes, the call's one synchronisation."""
    for what, t in (("hidden", hidden), ("weight", weight), ("labels", labels), ("advantages", advantages)):
        need_device(t, what, "the self-critical loss")
    if hidden.dtype != torch.float32:
        raise TypeError("`hidden` must be fp32, got {}".format(hidden.dtype))
    if weight.dtype != torch.float32:
        raise TypeError("`weight` must be fp32, got {}".format(weight.dtype))
    if hidden.dim() != 3 or weight.dim() != 2 or hidden.shape[2] != weight.shape[1]:
        raise ValueError("hidden [N, t (+ 1), d] and weight [V, d] expected, got {} and {}".format(tuple(hidden.shape), tuple(weight.shape)))
    if labels.dim() != 2 or labels.shape[0] != hidden.shape[0] or hidden.shape[1] not in (labels.shape[1], labels.shape[1] + 1):
        raise ValueError("hidden [N, t (+ 1), d] and labels [N, t] expected, got {} and {}".format(tuple(hidden.shape), tuple(labels.shape)))
    if advantages.numel() != hidden.shape[0]:
        raise ValueError("`advantages` holds {} entries for N = {} captions".format(advantages.numel(), hidden.shape[0]))
    if hidden.numel() == 0 or labels.numel() == 0 or weight.numel() == 0:
        raise ValueError("the loss of empty hidden states {} / weight {} is undefined".format(tuple(hidden.shape), tuple(weight.shape)))
    if weight.device != hidden.device or labels.device != hidden.device or advantages.device != hidden.device:
        raise RuntimeError("hidden states are on `{}`, weight on `{}`, labels on `{}`, advantages on `{}`".format(
            hidden.device, weight.device, labels.device, advantages.device))
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() < 2 or acc.device != hidden.device):
        raise ValueError("`acc` must hold 2 float64 entries on {}".format(hidden.device))
    if live is not None and not 0 <= int(live) <= labels.numel():
        raise ValueError("`live` = {} for {} label positions".format(live, labels.numel()))
    labels32 = labels.to(torch.int32).contiguous()
    adv = advantages.detach().to(torch.float32).reshape(-1).contiguous()
    N, tl, d = hidden.shape
    with torch.cuda.device(hidden.device):
        loss, seq_logp, totals = _HeadRewardLoss.apply(hidden.reshape(N * tl, d), weight, labels32, adv, acc, live)
    return (loss, seq_logp, totals) if return_aux else loss

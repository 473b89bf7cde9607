"""Caption retrieval on device: the `r` modality from a bank of caption embeddings (pretreatment/clip_retrieval.py:47-83 `run`,
:175-176 and :305-321; dataloader.py:808-814 takes the first `retrieval_topk` rows; csrc/retrieval.hip).

The reference writes these rows offline, one video at a time: `[1, D] @ [D, M]`, a full sort of the M scores, a Python walk that
skips the clip's own captions (`info`) and, with `--unique`, captions whose string was already taken.  Here a batch's `i` tensor
goes in and `feats_r` comes out, on the current stream and without a host synchronisation:

    bank = CaptionBank(text_embs, captions, unique=True, device="cuda")
    feats = attach_retrieval(feats_without_r, opt, bank, own_ranges)

The contract, per clip: query = the mean of the clip's CLIP image features over the sampled frames, L2-normalised; bank = the
caption embeddings, L2-normalised per row; scores = q . t in fp32; the `topk` best ELIGIBLE columns in the order (score
descending, index ascending) - the tie rule of this project's other selections, where the reference's unstable sort leaves the
order of equal scores open.  Eligible: outside the clip's own range `[start, end)` and, with `unique`, the REPRESENTATIVE of its
group of equal strings: the group's lowest-index member outside the own range.  The reference takes the best-scoring admissible
member of a group; where the members' embedding rows are bit-identical (`bank.groups_exact`) their scores are too and that is
the same column.  Where they are not (`groups_exact` False: equal strings embedded differently) the choice can differ from the
reference's - only between members of one string, never in which strings are retrieved beyond what their scores decide.

What is returned is rows of the UN-normalised table (`text_embs`, or `gather_embs` of another width: `--arch_f`).  `subset`
is `--ratio`: only a sorted subset of the bank is scanned; own ranges and returned ids stay in the original numbering.

No torch arithmetic is on the scoring path; grouping strings and translating ranges are host-side index plumbing.  As
everywhere in care_amd there is no CPU fallback: CPU tensors raise.
"""
import numpy as np
import torch

from . import _lib

MAX_TOPK, MAX_DIM = 128, 1024


def group_links(captions):
    """(first, prev) int32 arrays over a list of caption strings: first[j] = the lowest index with j's string, prev[j] = the
    previous index with it or -1."""
    first, prev = np.empty(len(captions), dtype=np.int32), np.empty(len(captions), dtype=np.int32)
    head, last = {}, {}
    for j, cap in enumerate(captions):
        first[j] = head.setdefault(cap, j)
        prev[j] = last.get(cap, -1)
        last[cap] = j
    return first, prev


def eligible(j: int, start: int, end: int, first=None, prev=None) -> bool:
    """The scan's O(1) test, written out: column j for a clip with the own range [start, end)."""
    if start <= j < end:
        return False
    if prev is None or prev[j] < 0:
        return True
    return bool(first[j] >= start and prev[j] < end)


def translate_ranges(sampled, own_ranges):
    """Own ranges in original numbering -> positions in the sorted subset `sampled` (a range outside it becomes empty)."""
    r = np.asarray(own_ranges, dtype=np.int64).reshape(-1, 2)
    return np.stack([np.searchsorted(sampled, r[:, 0], side="left"), np.searchsorted(sampled, r[:, 1], side="left")], axis=1)


def _check_dim(what, d):
    if d % 16 or not 16 <= d <= MAX_DIM:
        raise NotImplementedError("{} = {}: the retrieval kernels take widths that are multiples of 16 up to {}".format(what, d, MAX_DIM))


def _device_f32(what, t, device):
    t = torch.as_tensor(t)
    if t.dtype != torch.float32:
        raise NotImplementedError("{} is {}: retrieval is fp32".format(what, t.dtype))
    return t.to(device).contiguous()


class CaptionBank:
    """The caption embeddings to retrieve from.  text_embs [M, D] fp32 (un-normalised, as the text encoder wrote them);
    captions: the M strings (needed with `unique`); gather_embs [M, D_e]: another table whose rows are returned instead."""

    def __init__(self, text_embs, captions=None, unique=False, gather_embs=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("a CaptionBank lives on the MI355X (no CPU fallback), not on `{}`".format(self.device))
        text_embs = torch.as_tensor(text_embs)
        if text_embs.dim() != 2 or text_embs.shape[0] < 1:
            raise ValueError("text_embs must be [M >= 1, D], got {}".format(tuple(text_embs.shape)))
        _check_dim("D", text_embs.shape[1])
        if unique and captions is None:
            raise ValueError("`unique` needs the caption strings")
        if captions is not None and len(captions) != text_embs.shape[0]:
            raise ValueError("{} captions for {} embeddings".format(len(captions), text_embs.shape[0]))
        if gather_embs is not None:
            gather_embs = torch.as_tensor(gather_embs)
            if gather_embs.dim() != 2 or gather_embs.shape[0] != text_embs.shape[0]:
                raise ValueError("gather_embs {} does not match text_embs {}".format(tuple(gather_embs.shape), tuple(text_embs.shape)))
            _check_dim("D_e", gather_embs.shape[1])
        self.unique = bool(unique)
        self.captions = list(captions) if captions is not None else None
        self.groups_exact = self._groups_exact(text_embs, self.captions) if self.captions is not None else None
        self.embs = _device_f32("text_embs", text_embs, self.device)
        self.table = self.embs if gather_embs is None else _device_f32("gather_embs", gather_embs, self.device)
        self.size, self.dim, self.dim_out = self.embs.shape[0], self.embs.shape[1], self.table.shape[1]
        self.unit = torch.empty_like(self.embs)
        with torch.cuda.device(self.device):
            _lib.call("care_l2_normalize_rows", _lib.ptr(self.embs), _lib.ptr(self.unit), self.size, self.dim, tag="l2_normalize_rows")
        self.sampled = None       # numpy int64 [M_s]: the original indices of the scanned rows (subset banks)
        self.orig = None          # the same as a device int32 tensor
        self._set_links(self.captions)

    @staticmethod
    def _groups_exact(text_embs, captions) -> bool:
        """Whether all members of every group of equal strings have bit-identical embedding rows."""
        bits = text_embs.detach().cpu().contiguous().view(torch.int32).numpy()
        head = {}
        for j, cap in enumerate(captions):
            k = head.setdefault(cap, j)
            if k != j and not np.array_equal(bits[k], bits[j]):
                return False
        return True

    def _set_links(self, captions):
        if self.unique:
            first, prev = group_links(captions)
            self.first_host, self.prev_host = first, prev
            self.first, self.prev = torch.from_numpy(first).to(self.device), torch.from_numpy(prev).to(self.device)
        else:
            self.first_host = self.prev_host = self.first = self.prev = None

    def subset(self, sampled_indices):
        """The `--ratio` form: a bank that scans only the rows `sampled_indices` (sorted original indices) and answers in
        original numbering."""
        sampled = np.asarray(sampled_indices, dtype=np.int64)
        if sampled.ndim != 1 or sampled.size < 1 or np.any(np.diff(sampled) <= 0) or sampled[0] < 0 or sampled[-1] >= self.size:
            raise ValueError("sampled_indices must be strictly ascending indices into the bank")
        if self.sampled is not None:
            raise ValueError("a subset of a subset: take it from the full bank")
        sub = object.__new__(CaptionBank)
        sub.device, sub.unique, sub.groups_exact = self.device, self.unique, self.groups_exact
        sub.captions = [self.captions[j] for j in sampled] if self.captions is not None else None
        sub.embs, sub.table = self.embs, self.table                       # gathered from in original numbering
        sub.size, sub.dim, sub.dim_out = int(sampled.size), self.dim, self.dim_out
        sub.sampled = sampled
        sub.orig = torch.from_numpy(sampled.astype(np.int32)).to(self.device)
        ids = torch.from_numpy(sampled).to(self.device)
        sub.unit = torch.empty(sub.size, self.dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):                              # the scanned rows, contiguous
            _lib.call("care_retrieval_gather", _lib.ptr(self.unit), self.size, self.dim, _lib.ptr(ids), sub.size, _lib.ptr(sub.unit),
                      tag="retrieval_gather")
        sub._keep = ids
        sub._set_links(sub.captions)
        return sub

    def _ranges(self, own_ranges, B):
        """own_ranges ([B, 2] original numbering, a ready-made (start, end) pair, or None) -> two device int32 tensors in
        scanned numbering, or (None, None)."""
        if own_ranges is None:
            return None, None
        if isinstance(own_ranges, tuple) and len(own_ranges) == 2 and all(isinstance(t, torch.Tensor) for t in own_ranges):
            start, end = own_ranges                                       # ready-made: two device int32 [B] tensors, scanned numbering
            if any(t.dtype != torch.int32 or t.device.type != "cuda" or t.shape != (B,) or not t.is_contiguous() for t in own_ranges):
                raise ValueError("own ranges as a (start, end) pair must be contiguous device int32 tensors of {} elements".format(B))
            return start, end
        if isinstance(own_ranges, torch.Tensor) and own_ranges.device.type == "cuda" and self.sampled is None:
            r = own_ranges.to(torch.int32).reshape(B, 2)                  # already on device: no host round trip
            return r[:, 0].contiguous(), r[:, 1].contiguous()
        r = np.asarray(own_ranges.cpu() if isinstance(own_ranges, torch.Tensor) else own_ranges, dtype=np.int64).reshape(-1, 2)
        if r.shape[0] != B:
            raise ValueError("{} own ranges for {} clips".format(r.shape[0], B))
        r = np.clip(r, 0, 2 ** 31 - 1)
        if self.sampled is not None:
            r = translate_ranges(self.sampled, r)
        r = torch.from_numpy(np.ascontiguousarray(r.T.astype(np.int32))).to(self.device, non_blocking=True)
        return r[0], r[1]

    def query(self, image_feats):
        """[B, n, D] frame features -> the [B, D] unit queries (clip_retrieval.py:105-110, :175)."""
        if image_feats.device.type != "cuda":
            raise RuntimeError("image_feats are on `{}`: retrieval runs on the MI355X (no CPU fallback)".format(image_feats.device))
        if image_feats.dim() != 3 or image_feats.shape[2] != self.dim or image_feats.shape[0] < 1 or image_feats.shape[1] < 1:
            raise ValueError("image_feats must be [B, n_frames, {}], got {}".format(self.dim, tuple(image_feats.shape)))
        if image_feats.dtype != torch.float32:
            raise NotImplementedError("image_feats are {}: retrieval is fp32".format(image_feats.dtype))
        x = image_feats.contiguous()
        q = torch.empty(x.shape[0], self.dim, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("care_retrieval_query", _lib.ptr(x), _lib.ptr(q), x.shape[0], x.shape[1], self.dim, tag="retrieval_query")
        return q

    def search(self, q, topk, own_ranges=None):
        """Unit queries [B, D] -> (ids int64 [B, topk], scores fp32 [B, topk], count int32 [B])."""
        topk = int(topk)
        if not 1 <= topk <= MAX_TOPK:
            raise NotImplementedError("topk = {}: 1 to {} are supported".format(topk, MAX_TOPK))
        B = q.shape[0]
        start, end = self._ranges(own_ranges, B)
        dev = q.device
        ids = torch.empty(B, topk, dtype=torch.int64, device=dev)
        scores = torch.empty(B, topk, dtype=torch.float32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        scratch = torch.empty(_lib.load().care_retrieval_scratch(B, self.size, topk), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("care_retrieval_topk", _lib.ptr(q), _lib.ptr(self.unit), B, self.size, self.dim, topk, _lib.ptr(start),
                      _lib.ptr(end), _lib.ptr(self.first), _lib.ptr(self.prev), _lib.ptr(self.orig), _lib.ptr(ids), _lib.ptr(scores),
                      _lib.ptr(count), _lib.ptr(scratch), scratch.numel(), tag="retrieval_topk")
        return ids, scores, count

    def gather(self, ids):
        """Rows of the un-normalised table at ids [B, topk] (zeros at -1) -> [B, topk, D_e]."""
        out = torch.empty(ids.shape + (self.dim_out,), dtype=torch.float32, device=ids.device)
        with torch.cuda.device(ids.device):
            _lib.call("care_retrieval_gather", _lib.ptr(self.table), self.table.shape[0], self.dim_out, _lib.ptr(ids), ids.numel(),
                      _lib.ptr(out), tag="retrieval_gather")
        return out

    def retrieve(self, image_feats, topk, own_ranges=None):
        """image_feats [B, n_frames, D] (the batch's `i` tensor) -> (feats_r [B, topk, D_e], ids, scores, count): device
        tensors, enqueued on the current stream."""
        ids, scores, count = self.search(self.query(image_feats), topk, own_ranges)
        return self.gather(ids), ids, scores, count


def attach_retrieval(feats, opt, bank, own_ranges=None):
    """The batch's feature list WITHOUT `r` (in `opt['modality']` order, `r` left out) -> the list with `feats_r`, retrieved
    from its `i` tensor with `opt['retrieval_topk']`, at the position of `r`."""
    modality = opt["modality"].lower()
    if "r" not in modality:
        raise ValueError("modality `{}` has no retrieval stream `r`".format(opt["modality"]))
    if "i" not in modality:
        raise ValueError("modality `{}` has no image stream `i` to retrieve from".format(opt["modality"]))
    rest = [ch for ch in modality if ch != "r"]
    feats = list(feats)
    if len(feats) != len(rest):
        raise ValueError("{} feature tensors for the streams `{}`".format(len(feats), "".join(rest)))
    feats_r = bank.retrieve(feats[rest.index("i")], opt["retrieval_topk"], own_ranges)[0]
    at = modality.index("r")
    return feats[:at] + [feats_r] + feats[at:]

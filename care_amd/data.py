"""Input format of the path: per-video feature tables -> `batch['feats']`.

Restates the evaluation branch of `VideoOnlyDataset` (dataloader.py:142-190,232-282): per
modality a table `video<id> -> [60, dim]` (HDF5 in the reference; any Mapping here, h5py is
absent from this image), 28 of the 60 rows picked by `get_uniform_ids_from_k_snippets`
(misc/utils.py:311-317) for `load_feats_type == 0`, retrieval features = the first
`retrieval_topk` rows (dataloader.py:808-814), missing videos = zeros.  (Those rows need not come from a table written
offline: `care_amd.retrieval.attach_retrieval` retrieves them on device from a `CaptionBank` and the batch's `i` tensor.)
`FeaturePrefetcher`
adds what the reference lacks: pinned double-buffered host staging with the H2D copy on a
side stream, so an 8-GPU node is not input-bound (301 KB per clip over PCIe).
"""
from typing import Dict, List, Mapping, Sequence

import numpy as np
import torch

N_TOTAL_FRAMES = 60  # config/Constants.py:27


def get_uniform_ids_from_k_snippets(length: int, k: int, offset: int = 0) -> List[int]:
    """Middle frame of each of k equal snippets (misc/utils.py:311-317)."""
    bound = [int(i) for i in np.linspace(0, length, k + 1)]
    return [(bound[i] + bound[i + 1]) // 2 + offset for i in range(k)]


def resampling(source_length: int, target_length: int) -> List[int]:
    """misc/utils.py:307-308."""
    return [round(i * (source_length - 1) / (target_length - 1)) for i in range(target_length)]


def load_modality(tables: Sequence[Mapping], vid: str, dim: int, n_frames: int, frame_ids: Sequence[int]) -> np.ndarray:
    """`_load_feats` for load_feats_type 0 (dataloader.py:232-262): concat tables on the channel axis."""
    parts, pre_len = [], None
    for table in tables:
        if vid not in table:
            return np.zeros((n_frames, dim), dtype=np.float32)
        data = np.asarray(table[vid])
        if data.ndim == 1:
            data = data[np.newaxis, :].repeat(pre_len if pre_len is not None else N_TOTAL_FRAMES, axis=0)
        else:
            pre_len = data.shape[0]
        parts.append(data)
    feats = np.concatenate(parts, axis=1)
    return np.ascontiguousarray(feats[list(frame_ids)], dtype=np.float32)


def load_video_feats(databases: Dict[str, Sequence[Mapping]], vid: str, opt: dict) -> List[np.ndarray]:
    """One video's `feats` list in `opt['modality']` order (get_video_features_by_vid, dataloader.py:142-190)."""
    frame_ids = get_uniform_ids_from_k_snippets(N_TOTAL_FRAMES, opt["n_frames"])
    out = []
    for ch in opt["modality"].lower():
        if ch == "r":
            feats = np.asarray(databases[ch][0][vid])[: opt["retrieval_topk"], :].astype(np.float32)
        elif ch == "t":
            raise ValueError("retrieved-caption token inputs (`t`) belong to the pointer network, out of scope")
        else:
            feats = load_modality(databases[ch], vid, opt["dim_" + ch], opt["n_frames"], frame_ids)
        out.append(feats)
    return out


def collate_feats(per_video: Sequence[List[np.ndarray]]) -> List[torch.Tensor]:
    """default_collate of the `feats` lists: one [B, n, dim] fp32 tensor per modality."""
    n_mod = len(per_video[0])
    return [torch.from_numpy(np.stack([v[m] for v in per_video], axis=0)) for m in range(n_mod)]


FP16_MAX = 65504.0


def fp16_range_ok(feats: Sequence[torch.Tensor], margin: float = 0.5) -> bool:
    """Whether a batch's raw features fit the `fp16` compute mode: every |x| below margin x 65504 (the embedder rounds
    features to IEEE half as it multiplies them; every other 16-bit tensor of the path is a LayerNorm output, an attention
    context, a projected key / value or an FFN hidden value - O(1 .. 100) whatever the input).  A loader-side check (one
    reduction per tensor, on the host or the device the tensors live on) - not part of the decode pass.  Post-ReLU CNN /
    ViT features are O(10); features that fail belong in `bf16` mode (8 exponent bits, no bound)."""
    return all(bool(torch.isfinite(f).all()) and float(f.abs().max()) < margin * FP16_MAX for f in feats if f.numel())


class FeaturePrefetcher:
    """Double-buffered pinned staging + asynchronous H2D on a side stream.

    `for feats in FeaturePrefetcher(batches, device)` yields device tensors; the copy of batch
    i+1 overlaps the compute on batch i.  The yielded tensors are reused every `depth` batches, so
    the hipGraph keyed on their addresses (engine.translate_greedy) replays.

    A slot (pinned buffers + device tensors) is restaged only when both of its earlier users are
    done with it, with no host synchronisation of the consumer required:
      * the consumer's kernels that read the device tensors: when the consumer asks for the next
        batch it has enqueued that work on its stream; an event recorded there at that moment is
        what the side stream waits for before the next H2D into the same tensors;
      * the earlier asynchronous H2D that reads the pinned buffers: the host waits for that copy's
        event before overwriting them.
    """

    def __init__(self, batches, device, depth: int = 2):
        self.batches, self.device, self.depth = iter(batches), torch.device(device), depth
        self.stream = torch.cuda.Stream(self.device)
        self.slots = []

    def _slot(self, i, like):
        while len(self.slots) <= i:
            self.slots.append(None)
        slot = self.slots[i]
        if slot is None or any(a.shape != d.shape or a.dtype != d.dtype or (p is None) != a.is_pinned()
                               for a, (p, d) in zip(like, slot["bufs"])):
            if slot is not None:  # both users of the old buffers must be done before they are dropped
                for ev in (slot["staged"], slot["consumed"]):
                    if ev is not None:
                        ev.synchronize()
            # dtype follows the batch: fp32 features, or bf16 ones a loader rounded for a model whose embedder
            # multiplies bf16 operands anyway (engine.feats_dtype_ok: half the bytes over PCIe, the same products)
            slot = {"bufs": [(None if t.is_pinned() else torch.empty(t.shape, dtype=t.dtype).pin_memory(),
                              torch.empty(t.shape, dtype=t.dtype, device=self.device)) for t in like],
                    "staged": None, "consumed": None, "src": None}
            self.slots[i] = slot
        return slot

    def _stage(self, slot, batch):
        if slot["staged"] is not None:
            slot["staged"].synchronize()  # the previous H2D out of these pinned buffers has finished
        with torch.cuda.stream(self.stream):
            if slot["consumed"] is not None:
                self.stream.wait_event(slot["consumed"])  # the consumer's reads of the device tensors
            for src, (pin, dev) in zip(batch, slot["bufs"]):
                if pin is None:     # the loader already pins (DataLoader(pin_memory=True)): no second host copy
                    dev.copy_(src, non_blocking=True)
                else:
                    pin.copy_(src)
                    dev.copy_(pin, non_blocking=True)
            slot["src"] = list(batch)  # pinned sources stay alive until their copy has been waited for
            slot["staged"] = torch.cuda.Event()
            slot["staged"].record(self.stream)

    def _hand_over(self, slot):
        torch.cuda.current_stream(self.device).wait_event(slot["staged"])
        return [dev for _, dev in slot["bufs"]]

    def __iter__(self):
        pending, i = None, 0
        for batch in self.batches:
            slot = self._slot(i % self.depth, batch)
            self._stage(slot, batch)
            if pending is not None:
                yield self._hand_over(pending)
                # resumed: whatever the consumer launched on the yielded tensors is on its stream now
                pending["consumed"] = torch.cuda.Event()
                pending["consumed"].record(torch.cuda.current_stream(self.device))
            pending, i = slot, i + 1
        if pending is not None:
            yield self._hand_over(pending)
            pending["consumed"] = torch.cuda.Event()
            pending["consumed"].record(torch.cuda.current_stream(self.device))

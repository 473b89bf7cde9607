"""HipEngine, sampled decoding: captions drawn from the model's own distribution - temperature, top-k, nucleus - with the
decode loop on the device.  A step is the greedy step with the vocabulary arg-max replaced by the logits
in memory + care_sample_logits (csrc/sample.hip), which hands its token on through the parts = 1 form of the greedy
update's contract: the unchanged care_greedy_update(_embed) appends it, adds its MODEL log-probability, embeds it for the
next step and freezes the row at EOS.  The n samples of a clip are n rows that share the clip's cross-attention source,
as the beams of a clip do.  Methods of care_amd.engine.HipEngine."""
import math
import struct
from typing import List, Optional

import torch

from . import forms
from ._lib import ptr
from .constants import BOS, EOS

PARAMS_BYTES = 24   # { uint64 seed; float inv_temperature; float top_p; int32 top_k; int32 reserved } (include/care_hip.h)


def draw_seed() -> int:
    """A 62-bit seed from torch's generator (as training._Seeds draws its base): torch.manual_seed reproduces a run."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def check_sample_args(n_samples, temperature, top_k, top_p) -> None:
    """The refusals of sampled decoding, by name (Translator_ARFormer.sample_batch, HipEngine.translate_sample)."""
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError("`temperature` must be a finite number > 0, got {!r}".format(temperature))
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise ValueError("`top_p` must lie in (0, 1], got {!r}".format(top_p))
    if not (isinstance(top_k, int) and top_k >= 0):
        raise ValueError("`top_k` must be an integer >= 0 (0: off), got {!r}".format(top_k))
    if not (isinstance(n_samples, int) and n_samples >= 1):
        raise ValueError("`n_samples` must be an integer >= 1, got {!r}".format(n_samples))


def pack_params(seed: int, temperature: float, top_k: int, top_p: float) -> bytes:
    """The device block of care_sample_logits.  inv_temperature and top_p are rounded to fp32 HERE: what the kernel - and
    a reference that wants its bits - multiplies and compares with."""
    return struct.pack("<Qffii", int(seed) & ((1 << 64) - 1), 1.0 / float(temperature), float(top_p), int(top_k), 0)


class SampleMixin:
    def sample_params(self, seed: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
        """The engine's params block (a workspace: one address for every pass and every captured graph), rewritten by one
        small host-to-device copy on the current stream."""
        blk = self._ws_get("smp_params", (32,), torch.uint8)
        blk[:PARAMS_BYTES].copy_(torch.frombuffer(bytearray(pack_params(seed, temperature, top_k, top_p)), dtype=torch.uint8))
        return blk

    def sample(self, mem: torch.Tensor, sem: Optional[torch.Tensor], n: int, params: torch.Tensor,
               sample_ids: Optional[torch.Tensor] = None, sem_embs: Optional[torch.Tensor] = None, steps: Optional[int] = None):
        """n sampled captions for each of the B clips of `mem`: B n rows, row i n + j = sample j of clip i, drawn with the
        key sample_ids[i] n + j (sample_ids: int32 [B], default arange(B)) under the settings of the device block `params`
        (sample_params).  Fixed length: `steps` steps (default T); ended rows ride along frozen.

        Returns device tensors: fed int32 [B n, T + 1] (column 0 = BOS), length int32 [B n], score fp32 [B n] (the sum of
        the MODEL's log-probabilities of the chosen tokens, temperature 1, no filter), score_q fp32 [B n] (the sum of
        their log-probabilities under the distribution they were drawn from).  No host synchronisation inside."""
        B, Lk, d = mem.shape
        T, V, w = self.T, self.V, self.w
        N = B * n
        steps = T if steps is None else steps
        mem = mem.to(self.device, mem.dtype if mem.dtype == self.h16 else torch.float32)
        length, score, score_q, fed = self.ws_block("s_out", [((N,), torch.int32), ((N,), torch.float32), ((N,), torch.float32),
                                                              ((N, T + 1), torch.int32)])
        fin, key = self.ws("s_fin", (N,), torch.int32), self.ws("s_key", (N,), torch.int32)
        sem = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
        x0, x0b = self.ws("s_x0", (N, d)), self.wsb("s_x0", (N, d))   # (what _decode_step reads once the update has embedded)
        fed.zero_(); fed[:, 0] = BOS
        score.zero_(); score_q.zero_(); length.zero_(); fin.zero_()
        ids = self._arange(B) if sample_ids is None else sample_ids.to(self.device, torch.int32)
        torch.add(ids.view(B, 1) * n, self._arange(n).view(1, n), out=key.view(B, n))
        ckv = self.cross_src(mem, N)
        akv = self.attr_kv(sem_embs) if self.attr_att else None
        skv = [self.ws("s_skv%d" % li, (N, T, 2 * d), self.wt) for li in range(self.n_layers)]
        vpad = (V + 63) // 64 * 64   # 16-byte aligned row stride -> the GEMM's vector store path
        logits = self.ws("s_logits", (N, vpad))
        pmax, psum, logq = self.ws("s_pmax", (N,)), self.ws("s_psum", (N,)), self.ws("s_logq", (N,))
        pidx = self.ws("s_pidx", (N,), torch.int32)
        for t in range(1, steps + 1):
            x, xb = self._decode_step(t, N, n, fed, None, sem, ckv, skv, Lk, "s_", akv=akv, embedded=t > 1)
            self.gemm(xb if xb is not None else x, w["vocab"], None, logits[:, :V], tag="step_vocab_logits")
            self.call("care_sample_logits", ptr(logits), vpad, V, N, ptr(key), t, ptr(params), ptr(pmax), ptr(pidx), ptr(psum),
                      ptr(logq), None, tag="step_sample")
            self.call("care_sample_accum", ptr(logq), ptr(fin), ptr(score_q), N)   # (in front of the update, which sets `fin`)
            update = (ptr(pmax), ptr(pidx), ptr(psum), 1, ptr(fed), T + 1, ptr(score), ptr(length), ptr(fin), t, T, EOS, N)
            if t < steps:
                self.call("care_greedy_update_embed", *update, ptr(w["word"]), ptr(w["pos"]), ptr(sem), n, ptr(w["emb_g"]),
                          ptr(w["emb_be"]), self.eps, ptr(x0), ptr(x0b), d, d, tag="step_update_embed")
            else:
                self.call("care_greedy_update", *update)
        return fed, length, score, score_q

    def translate_sample(self, feats: List[torch.Tensor], n: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                         seed: Optional[int] = None, use_graph: bool = True, sample_ids: Optional[torch.Tensor] = None,
                         steps: Optional[int] = None):
        """encode + `sample` of one batch through the multi-launch forms; replayed from a hipGraph when the input buffers
        repeat (the policy of translate_greedy).  The graph's key holds nothing of seed, temperature, top_k or top_p: they
        - and the sample ids - live in workspaces written HERE, outside the capture, in front of the pass or the replay.
        seed None: one from torch's generator.  Returns (enc_outputs, fed, length, score, score_q)."""
        check_sample_args(n, temperature, top_k, top_p)
        feats = self._prep_feats(feats)
        B = feats[0].shape[0]
        plan = self._begin_pass(self.plan_for(B, rows=B * n))
        params = self.sample_params(draw_seed() if seed is None else seed, temperature, top_k, top_p)
        ids = self._ws_get("smp_ids", (B,), torch.int32)
        if sample_ids is None:
            torch.arange(B, device=self.device, dtype=torch.int32, out=ids)
        else:
            ids.copy_(torch.as_tensor(sample_ids).to(torch.int32).view(B))

        def run():
            enc = self.encode(feats, plan.lean)
            return (enc,) + tuple(self.sample(enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), n, params,
                                              sample_ids=ids, sem_embs=enc.get("semantic_embs"), steps=steps))

        return self._replay(forms.graph_key("sample", plan, feats, n, steps), run, use_graph)

"""HipEngine, the small-batch forms: the drivers of the decode as ONE resident launch (csrc/decode_resident*.hip) and as
chained kernels per step (csrc/decode_chain.hip) (models/Translator.py:77-143 on the device); which batches take them is
care_amd/forms.py's.  Methods of care_amd.engine.HipEngine."""
import ctypes
import os
from typing import Dict, List, Optional

import torch

from . import _lib, forms
from ._lib import ACT_CODES, CARE_BF16, CARE_F32, ptr
from .constants import BOS, EOS, PAD
from .engine_util import _LaneOutputs, device_props


class ResidentMixin:
    # ------------------------------------------------------------------ resident decode of small batches
    def _resident_pass(self, kind: str, name: str, feats, run, use_graph: bool, scratch: str, nbytes: int, **stats):
        """A pass whose decode is ONE resident launch of `kind` ("greedy" / "beam"): run() through the graph cache, or None
        where the launch was refused before anything was enqueued (CARE_ESHAPE: the device admits fewer resident workgroups
        than the launch needs - a partition with few CUs, another occupancy).  The refusal is noted (forms.resident_fits), so
        the next plan of this engine takes the multi-launch forms from that row count on: not an error."""
        plan = self.plan
        try:
            out = self._replay(forms.graph_key(name, plan, feats), run, use_graph)
        except _lib.CareHipError as exc:
            if "CARE_ESHAPE" not in str(exc):
                raise
            self._resident_refused[kind] = min(self._resident_refused.get(kind, 1 << 30), plan.rows)
            return None
        self.last_decode = dict(clips=plan.clips, steps=self.ws(scratch, (nbytes,), torch.uint8)[8:12].view(torch.int32)[0],
                                compactions=0, resident=True, **stats)
        return out

    def _resident_layers(self, tag: str, rows: int, rows_per_clip: int, ckv, akv, Lk: int):
        """care_resident_layer[] of this model for a resident launch over `rows` rows (self-attention caches in the
        workspaces `tag`skv*; static K/V per clip, shared by its `rows_per_clip` rows)."""
        w, d, T = self.w, self.d, self.T
        layers = self._res_layers = (_lib.ResidentLayer * self.n_layers)()  # kept: bench.py re-issues the recorded call
        for li in range(self.n_layers):
            L, sa, ffn = layers[li], "d{}_sa".format(li), "d{}_ffn".format(li)
            L.qkv_w, L.qkv_b, L.o_w, L.o_b = ptr(w[sa + "_qkv_w"]), ptr(w[sa + "_qkv_b"]), ptr(w[sa + "_o_w"]), ptr(w[sa + "_o_b"])
            L.ln_g, L.ln_b = ptr(w[sa + "_g"]), ptr(w[sa + "_be"])
            L.self_kv = ptr(self.ws(tag + "skv%d" % li, (rows, T, 2 * d), self.h16))
            blocks = [("d{}_ca".format(li), ckv[li], Lk, w["d{}_hb".format(li)])]
            if self.attr_att:
                blocks.append(("d{}_aa".format(li), akv[li], self.topk, None))
            L.n_att = len(blocks)
            for a, (nm, kv, nkeys, hb) in enumerate(blocks):
                A = L.att[a]
                A.q_w, A.q_b, A.o_w, A.o_b = ptr(w[nm + "_q_w"]), ptr(w[nm + "_q_b"]), ptr(w[nm + "_o_w"]), ptr(w[nm + "_o_b"])
                A.ln_g, A.ln_b = ptr(w[nm + "_g"]), ptr(w[nm + "_be"])
                A.kv, A.kv_batch_stride, A.nkeys, A.rows_per_kv = ptr(kv), nkeys * 2 * d, nkeys, rows_per_clip
                A.bias, A.bias_ld = ptr(hb), (hb.stride(0) if hb is not None else 0)
            L.w1, L.b1, L.w2, L.b2 = ptr(w[ffn + "_w1"]), ptr(w[ffn + "_b1"]), ptr(w[ffn + "_w2"]), ptr(w[ffn + "_b2"])
            L.ffn_g, L.ffn_b = ptr(w[ffn + "_g"]), ptr(w[ffn + "_be"])
        return layers

    def _model_args(self, sem, d: int):
        """The model arguments every decode call leads with, after (layers, n_layers): word .. act."""
        w = self.w
        return (ptr(w["word"]), ptr(w["pos"]), ptr(sem), ptr(w["emb_g"]), ptr(w["emb_be"]), self.eps, ptr(w["vocab"]), self.V, d,
                self.H, self.ff, self.act)

    def _beam_state(self, tag: str, B: int, bm: int, need: int):
        """The beam state of csrc/beam.hip in the workspaces `tag`*."""
        T, N, cap = self.T, B * bm, need + bm
        return dict(tok=self.ws(tag + "tok", (N, T + 1), torch.int32),
                    anc=[self.ws(tag + "anc%d" % i, (N, T + 1), torch.int32) for i in range(2)],
                    scores=self.ws(tag + "scores", (N,)), done=self.ws(tag + "done", (B,), torch.int32),
                    **dict(zip(("nfin", "fscore", "flen", "fhyp"), self.ws_block(tag + "out", self._beam_out_parts(B, cap)))))

    def _beam_state_args(self, v, cap: int, scratch, nbytes: int):
        """The tail of the beam calls: tok, stride, anc0, anc1, scores .. fhyp, cap, scratch, bytes."""
        return (ptr(v["tok"]), self.T + 1, ptr(v["anc"][0]), ptr(v["anc"][1]),
                *(ptr(v[k]) for k in ("scores", "done", "nfin", "fscore", "flen", "fhyp")), cap, ptr(scratch), nbytes)

    def beam_resident(self, mem: torch.Tensor, sem: Optional[torch.Tensor], bm: int, need: int,
                      sem_embs: Optional[torch.Tensor] = None, early_exit: bool = True):
        """Beam search of B clips x bm beams in ONE launch (care_decode_resident_beam): the step loop of
        Translator.translate_batch (models/Translator.py:77-143) with Beam.advance (misc/Decoding/Beam.py:45-85) on the
        device, stopping once every clip is done (Translator.py:77-81).  Returns the per-clip results of engine.beam:
        nfin [B], fscore / flen [B, need + bm], fhyp [B, need + bm, T + 1]; no host synchronisation here."""
        B, Lk, d = mem.shape
        T, N, cap = self.T, mem.shape[0] * bm, need + bm
        sem = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
        ckv = self.cross_kv(mem, tag="rb_ckv", resident=True)
        akv = self.attr_kv(sem_embs, tag="rb_akv") if self.attr_att else None
        v = self._beam_state("rb_", B, bm, need)
        layers = self._resident_layers("rb_", N, bm, ckv, akv, Lk)
        nbytes = self.lib.care_decode_resident_beam_scratch(B, bm, d, self.ff, self.V)
        scratch = self.ws("rb_scratch", (nbytes,), torch.uint8)
        self.call("care_decode_resident_beam", ctypes.addressof(layers), self.n_layers, *self._model_args(sem, d), B, bm, need, T, T,
                  BOS, EOS, PAD, *self._beam_state_args(v, cap, scratch, nbytes), int(bool(early_exit)), 0, tag="decode_resident_beam")
        self.last_decode = dict(clips=B, steps=scratch[8:12].view(torch.int32)[0], compactions=0, resident=True,
                                row_steps=None)
        return v["nfin"], v["fscore"], v["flen"], v["fhyp"]

    def beam_chain_steps(self, mem: torch.Tensor, sem: Optional[torch.Tensor], bm: int, need: int, t0: int, t1: int,
                         sem_embs: Optional[torch.Tensor] = None, count_live: bool = True):
        """Steps t0 .. t1 of the beam search of B clips x bm beams as chains of kernels (care_decode_chain_beam: 10
        launches per step for a one-layer decoder; models/Translator.py:77-143, misc/Decoding/Beam.py:45-85), the beam
        state of csrc/beam.hip in the `cb_` workspaces; t0 == 1 also projects the clips' static K/V and initialises the
        state.  Ends with the partition of the clips by `done` (care_active_slots: cb_cnt = clips still live).  No host
        synchronisation here."""
        B, Lk, d = mem.shape
        T, N, cap = self.T, mem.shape[0] * bm, need + bm
        sem = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
        kvs = self.__dict__.setdefault("_chain_kv", {})
        if t0 == 1:  # (static workspaces: the handles of a (clips, beam) stay valid for the later segments' graphs)
            kvs[(B, bm)] = (self.cross_kv(mem, tag="cb_ckv", resident=True),
                            self.attr_kv(sem_embs, tag="cb_akv") if self.attr_att else None)
        ckv, akv = kvs[(B, bm)]
        v = self._beam_state("cb_", B, bm, need)
        v.update(idx=self.ws("cb_idx", (B,), torch.int32), cnt=self.ws("cb_cnt", (1,), torch.int32))
        layers = self._resident_layers("cb_", N, bm, ckv, akv, Lk)
        nbytes = self.lib.care_decode_chain_beam_scratch(B, bm, d, self.ff, self.V)
        scratch = self.ws("cb_scratch", (nbytes,), torch.uint8)
        self.call("care_decode_chain_beam", ctypes.addressof(layers), self.n_layers, *self._model_args(sem, d), B, bm, need, T,
                  t0, t1, BOS, EOS, PAD, *self._beam_state_args(v, cap, scratch, nbytes),
                  int(os.environ.get("CARE_CHAIN_FORM", "-1")), tag="decode_chain_beam")
        if count_live:
            self.call("care_active_slots", ptr(v["done"]), B, ptr(v["idx"]), ptr(v["cnt"]))
        return v

    def translate_beam_chain(self, feats: List[torch.Tensor], bm: int, need: int, use_graph: bool = True, lean: bool = False,
                             early_exit: bool = True, plan: Optional[forms.PassPlan] = None):
        """encode + beam search with chained steps.  The pass runs in segments of `chain_segment_steps` steps, each a
        hipGraph of its own (the first with the encoder and the static K/V projection); between segments the host reads
        ONE counter - the clips still live - and stops when none is (`if not active_inst_idx_list: break`,
        models/Translator.py:77-81).  early_exit=False: all T steps in one graph.  No compaction: the chain serves the
        row counts below those at which moving the survivors pays (engine.beam_early_exit)."""
        B, T = feats[0].shape[0], self.T
        if plan is None:  # (called on its own, not from translate_beam)
            plan = self._begin_pass(self.plan_for(B, bm, need, lean=lean, early_exit=early_exit))
        S = max(1, self.chain_segment_steps) if early_exit else T

        def steps(enc, t0, t1, count_live=True):
            return self.beam_chain_steps(enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), bm, need, t0, t1,
                                         sem_embs=enc.get("semantic_embs"), count_live=count_live)

        def first():
            enc = self.encode(feats, plan.lean, static=True, small=plan.small)
            return enc, dict(steps(enc, 1, min(S, T), early_exit), enc=enc)

        enc, v = self._segments(B, bm, S, forms.graph_key("bchain", plan, feats, 0, S), first,
                                lambda t, t1, n, par: forms.graph_key("bchain", plan, feats, t, t1),
                                lambda v, t, t1: steps(v["enc"], t, t1), use_graph,
                                cnt=self.ws("cb_cnt", (1,), torch.int32) if early_exit else None, chain=True)
        return enc, v["nfin"], v["fscore"], v["flen"], v["fhyp"]

    def greedy_resident(self, mem: torch.Tensor, sem: Optional[torch.Tensor], sem_embs: Optional[torch.Tensor] = None,
                        steps: Optional[int] = None, early_exit: bool = True):
        """Greedy decoding of B clips in ONE launch: the step loop of Translator.translate_batch with beam_size 1
        (models/Translator.py:77-143) runs on the device, phases of a step separated by grid barriers, and stops once
        every clip has ended (Translator.py:77-81).  Returns device tensors fed int32 [B, T + 1], length int32 [B],
        score fp32 [B]; `self.last_decode["steps"]` is a 0-dim DEVICE tensor (no host synchronisation here)."""
        B, Lk, d = mem.shape
        T = self.T
        steps = T if steps is None else steps
        sem = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
        ckv = self.cross_kv(mem, tag="r_ckv", resident=True)
        akv = self.attr_kv(sem_embs, tag="r_akv") if self.attr_att else None
        length, score, fed = self.ws_block("r_out", [((B,), torch.int32), ((B,), torch.float32), ((B, T + 1), torch.int32)])
        fin = self.ws("r_fin", (B,), torch.int32)
        layers = self._resident_layers("r_", B, 1, ckv, akv, Lk)
        nbytes = self.lib.care_decode_resident_scratch(B, d, self.ff, self.V)
        scratch = self.ws("r_scratch", (nbytes,), torch.uint8)
        model = self._model_args(sem, d)
        self.call("care_decode_resident", ctypes.addressof(layers), self.n_layers, *model[:3], 1, *model[3:], B, T, steps,
                  BOS, EOS, PAD, ptr(fed), T + 1, ptr(score), ptr(length), ptr(fin), ptr(scratch), nbytes,
                  int(bool(early_exit)), 0, tag="decode_resident")
        self.last_decode = dict(clips=B, steps=scratch[8:12].view(torch.int32)[0], compactions=0, resident=True)
        return fed, length, score

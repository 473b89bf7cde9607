"""HipEngine, beam search over many launches: the forms of the per-row top-k (logits + select, group maxima of the tiled
vocabulary product, two fused passes), the segmented search with early exit and compaction, and `translate_beam`, which
picks between all forms of the search (models/Translator.py:35-133, misc/Decoding/Beam.py).  Methods of care_amd.engine.HipEngine."""
import ctypes
from typing import Dict, List, Optional

import torch

from . import _lib, forms
from ._lib import ACT_CODES, CARE_BF16, CARE_F32, ptr
from .constants import BOS, EOS, PAD
from .engine_util import _LaneOutputs


class BeamMixin:
    def _beam_out_parts(self, B: int, cap: int):
        """Per-clip results of a beam search as parts of one block (engine.ws_block): nfin [B], fscore / flen [B, cap],
        fhyp [B, cap, T + 1]."""
        return [((B,), torch.int32), ((B, cap), torch.float32), ((B, cap), torch.int32), ((B, cap, self.T + 1), torch.int32)]

    def _beam_sparse_ws(self, tag: str, rows: int):
        """Workspaces of the sparse second pass (csrc/beam_sparse.hip) - (tile maxima [tiles, rows] fp32, per-tile
        row counts + work-unit prefix sums [2 tiles + 1], per-tile row lists [tiles, rows]) - or None where the 256-row statistics kernel does not apply."""
        if not (self.plan.sparse_second_pass and self.lib.care_beam_sparse_applies(rows, self.V, self.d, 1)):
            return None
        tiles = (self.V + 31) // 32
        return (self.ws(tag + "stmax", (tiles, rows)), self.ws(tag + "stcount", (2 * tiles + 1,), torch.int32),
                self.ws(tag + "stlist", (tiles, rows), torch.int32))

    def _beam_select_ws(self, tag: str, N: int):
        """Workspaces of the pass's form of the per-row top-k (plan.beam_select) over N rows."""
        if self.plan.beam_select == "fused":
            parts, cap = self.lib.care_argmax_parts_bf16_min(N, self.V, self.d, 1, 8), 64  # bf16 rows (code 1)
            return dict(parts=parts, cap=cap, pmax=self.ws(tag + "spmax", (N, parts)), psum=self.ws(tag + "spsum", (N, parts)),
                        pidx=self.ws(tag + "spidx", (N, parts), torch.int32), thr=self.ws(tag + "sthr", (N,)),
                        cnt=self.ws(tag + "scnt", (N,), torch.int32), cval=self.ws(tag + "scval", (N, cap)),
                        cidx=self.ws(tag + "scidx", (N, cap), torch.int32), sparse=self._beam_sparse_ws(tag, N))
        if self.plan.beam_select == "logits":
            vpad = (self.V + 63) // 64 * 64  # 16-byte aligned row stride -> the GEMM's vector store path
            return self.ws(tag + "logits", (N, vpad))[:, : self.V]
        return None

    def _beam_select(self, tag, s, x, xb, N, bm, cval, cidx):
        """The bm best columns of every row's log_softmax -> cval / cidx, in the pass's form (`s`: _beam_select_ws)."""
        d, V, W = self.d, self.V, self.w["vocab"]
        if self.plan.beam_select == "groups":
            parts = (V + 63) // 64
            pmax, psum = self.ws(tag + "gpmax", (N, parts)), self.ws(tag + "gpsum", (N, parts))
            gmax = self.ws(tag + "ggmax", (N, parts, 16))
            self.call("care_gemm_tile_beam", ptr(xb), xb.stride(0), ptr(W), ptr(pmax), ptr(psum), ptr(gmax), N, V, d, tag="beam_vocab_groups")
            self.call("care_beam_pick_groups", ptr(pmax), ptr(psum), ptr(gmax), parts, bm, ptr(xb), xb.stride(0), ptr(W),
                      V, d, ptr(cval), ptr(cidx), N, tag="beam_pick_groups")
        elif self.plan.beam_select == "fused":
            # statistics GEMM -> threshold -> candidate pass -> pick (csrc/beam.hip); the [N, V] logits never exist
            sparse = s["sparse"]
            if sparse is not None:
                # second pass only over the (tile, row) products whose tile maximum reaches the row's threshold
                self.call("care_gemm_argmax_bf16_tiles", ptr(xb), d, self._code(xb), ptr(W), ptr(s["pmax"]),
                     ptr(s["pidx"]), ptr(s["psum"]), ptr(sparse[0]), N, V, d, 8, tag="beam_vocab_stats")
                self.call("care_beam_threshold", ptr(s["pmax"]), s["parts"], bm, ptr(s["thr"]), ptr(s["cnt"]), N)
                self.call("care_beam_sparse_collect", ptr(xb), d, ptr(W), ptr(sparse[0]), ptr(s["thr"]),
                     ptr(s["cnt"]), ptr(s["cval"]), ptr(s["cidx"]), s["cap"], ptr(sparse[1]), ptr(sparse[2]), N, V, d,
                     tag="beam_vocab_collect")
            else:
                self.call("care_gemm_argmax_bf16_min", ptr(xb), d, self._code(xb), ptr(W), ptr(s["pmax"]),
                     ptr(s["pidx"]), ptr(s["psum"]), N, V, d, 8, tag="beam_vocab_stats")
                self.call("care_beam_threshold", ptr(s["pmax"]), s["parts"], bm, ptr(s["thr"]), ptr(s["cnt"]), N)
                self.call("care_gemm_collect_bf16", ptr(xb), d, self._code(xb), ptr(W), ptr(s["thr"]), ptr(s["cnt"]),
                     ptr(s["cval"]), ptr(s["cidx"]), s["cap"], N, V, d, tag="beam_vocab_collect")
            self.call("care_beam_pick", ptr(s["pmax"]), ptr(s["psum"]), s["parts"], ptr(s["cnt"]), ptr(s["cval"]), ptr(s["cidx"]), s["cap"],
                 bm, ptr(xb), d, self._code(xb), ptr(W), V, d, ptr(cval), ptr(cidx), N)
        else:
            # vocabulary logits -> per-row top-bm, in row chunks whose logits (chunk x vpad x 4 B) stay
            # inside the 256 MB Infinity Cache between the GEMM's stores and beam_select's loads
            # (*measured*, 20480 rows x 10560: chunks of 4096 rows = 173 MB +4% on the whole beam pass;
            # 5120 rows = 216 MB no gain, 2048 rows +1%)
            src = xb if xb is not None else x
            chunk = max(128, (176 << 20) // (s.stride(0) * 4) // 128 * 128)
            for lo in range(0, N, chunk):
                hi = min(N, lo + chunk)
                self.gemm(src[lo:hi], W, None, s[lo:hi], tag="step_vocab_logits")
                self.call("care_beam_select", ptr(s[lo:hi]), s.stride(0), V, bm, ptr(cval[lo:hi]),
                     ptr(cidx[lo:hi]), hi - lo, 4 if self.plan.small_beam else 1, tag="step_beam_select")

    # ------------------------------------------------------------------ the step loop; early exit + compaction
    def _beam_init(self, v, rows):
        """The beam state before step 1: every hypothesis EOS after its BOS, every ancestor the row itself (`rows`: the
        row numbers), scores and finished lists zero."""
        v["tok"].fill_(EOS); v["tok"][:, 0] = BOS
        for a in v["anc"]:
            a.copy_(rows.unsqueeze(1).expand(a.shape))
        for k in ("scores", "done", "nfin", "fscore", "flen", "fhyp"):
            v[k].zero_()

    def _beam_advance(self, v, t, bm, need, cval, cidx):
        """Beam.advance of step t (misc/Decoding/Beam.py:45-85) on the candidates cval / cidx of every row."""
        a_old, a_new = v["anc"][(t - 1) & 1], v["anc"][t & 1]
        self.call("care_beam_advance", ptr(cval), ptr(cidx), ptr(v["scores"]), bm, ptr(v["tok"]), ptr(a_old), ptr(a_new),
             ptr(v["done"]), ptr(v["nfin"]), need + bm, ptr(v["fscore"]), ptr(v["flen"]), ptr(v["fhyp"]), t, self.T, need, EOS,
             self.V, self.T + 1, v["n"])

    def _beam_steps(self, v, t0, t1, bm, need):
        """Steps t0 .. t1 of the beam search on the n clips (n * bm rows) of state `v` (tok, anc, scores, done, nfin, fscore,
        flen, fhyp, sem, ckv, akv, skv, Lk, tag, n)."""
        tag, N = v["tag"], v["n"] * bm
        cval, cidx = self.ws(tag + "cval", (N, bm)), self.ws(tag + "cidx", (N, bm), torch.int32)
        sel = self._beam_select_ws(tag, N)  # one form for the whole pass, whatever the compaction leaves
        for t in range(t0, t1 + 1):
            x, xb = self._decode_step(t, N, bm, v["tok"], v["anc"][(t - 1) & 1], v["sem"], v["ckv"], v["skv"], v["Lk"], tag,
                                      akv=v["akv"])
            self._beam_select(tag, sel, x, xb, N, bm, cval, cidx)
            self._beam_advance(v, t, bm, need, cval, cidx)

    def beam_early_exit(self, feats: List[torch.Tensor], bm: int, need: int, lean: bool = False, use_graph: bool = True,
                        plan: Optional[forms.PassPlan] = None):
        """encode + beam search that stops when every clip is done and drops finished clips between
        segments (models/Translator.py:77-81,194-209), like greedy_early_exit: the clip-level state
        (memory, finished lists ...) and the bm rows of every surviving clip (tokens, scores, K/V cache,
        ancestor tables - whose entries are physical row numbers and are renumbered) move to the front of
        a second buffer set.  Results per CLIP: nfin [B], fscore / flen [B, need + bm], fhyp [B, need + bm, T + 1]."""
        feats = self._prep_feats(feats)
        B, T, d = feats[0].shape[0], self.T, self.d
        cap = need + bm
        if plan is None:  # (called on its own, not from translate_beam)
            plan = self._begin_pass(self.plan_for(B, bm, need, lean=lean, early_exit=True, rows=B * bm))
        S = max(1, self.segment_steps) * (1 if B * bm >= 2048 else 2)
        out = dict(zip(("nfin", "fscore", "flen", "fhyp"), self.ws_block("be_out", self._beam_out_parts(B, cap))))
        idx, cnt = self.ws("be_idx", (B,), torch.int32), self.ws("be_cnt", (1,), torch.int32)

        def state(par, n):
            N = n * bm
            self._ws_cap = [(n, B), (N, B * bm)]
            tag = "b%d_" % par
            return dict(tag=tag, n=n, B=B, Lk=self.Lk,
                        tok=self.ws(tag + "tok", (N, T + 1), torch.int32),
                        anc=[self.ws(tag + "anc%d" % i, (N, T + 1), torch.int32) for i in range(2)],
                        scores=self.ws(tag + "scores", (N,)),
                        skv=[self.ws(tag + "skv%d" % li, (N, T, 2 * d), self.wt) for li in range(self.n_layers)],
                        done=self.ws(tag + "done", (n,), torch.int32), nfin=self.ws(tag + "nfin", (n,), torch.int32),
                        fscore=self.ws(tag + "fscore", (n, cap)), flen=self.ws(tag + "flen", (n, cap), torch.int32),
                        fhyp=self.ws(tag + "fhyp", (n, cap, T + 1), torch.int32), clip=self.ws(tag + "clip", (n,), torch.int32))

        def run_steps(v, t0, t1):
            """... and the partition of the clip slots by `done`"""
            self._ws_cap = [(v["n"], B), (v["n"] * bm, B * bm)]
            self._beam_steps(v, t0, t1, bm, need)
            self.call("care_active_slots", ptr(v["done"]), v["n"], ptr(idx), ptr(cnt))

        def first_segment():
            self._ws_cap = None
            enc = self.encode(feats, plan.lean, static=True, small=plan.small)
            mem, sem = enc["encoder_hidden_states"], enc.get("semantic_hidden_states")
            v = state(0, B)
            self._beam_init(v, self._arange(B * bm))
            torch.add(self._arange(B), 0, out=v["clip"])   # (an elementwise kernel, not a memcpy node in the captured graph: see csrc/decode_resident.h, res_zero_kernel)
            v["sem"] = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
            self._ws_cap = None
            v["ckv"] = self.cross_src(mem, B * bm)
            v["akv"] = self.attr_kv(enc.get("semantic_embs")) if self.attr_att else None
            run_steps(v, 1, min(S, T))
            return enc, v

        def flush(v):
            """finished lists of every slot of v -> the per-clip outputs"""
            n = v["n"]
            self._call_rows("care_scatter_rows", v["nfin"].view(n, 1), out["nfin"].view(B, 1), v["clip"], n)
            for k in ("fscore", "flen"):
                self._call_rows("care_scatter_rows", v[k], out[k], v["clip"], n)
            self._call_rows("care_scatter_rows", v["fhyp"].view(n, -1), out["fhyp"].view(B, -1), v["clip"], n)

        def compact(v, par, m, active):
            flush(v)
            return self._compact_beam(v, state(par, m), idx, active, bm)

        enc, v = self._segments(B, bm, S, forms.graph_key("bseg0", plan, feats, S), first_segment,
                                lambda t, t1, n, par: ("bseg", plan, t, t1, n, par), run_steps, use_graph, cnt=cnt,
                                count_last=True, compact=compact)
        flush(v)
        return enc, out["nfin"], out["fscore"], out["flen"], out["fhyp"]

    def _compact_beam(self, v, w, idx, active, bm):
        """The first w['n'] clips of the partition `idx` (unfinished first, finished ones as padding) and their rows
        -> buffer set `w`; ancestor entries are renumbered to the rows' new places."""
        n, m, B = v["n"], w["n"], v["B"]
        N, M = n * bm, m * bm
        self._ws_cap = [(m, B), (M, B * bm), (n, B), (N, B * bm)]
        tag = w["tag"]
        idx_r = self.ws(tag + "idx_r", (M,), torch.int32)
        self.call("care_expand_index", ptr(idx), m, bm, ptr(idx_r))
        cmap = self.ws(tag + "cmap", (n,), torch.int32)
        cmap.zero_()  # clips that are dropped map to clip 0: nothing references their rows any more
        self._call_rows("care_scatter_rows", self._arange(m).view(m, 1), cmap.view(n, 1), idx, m)
        for k in ("done", "nfin", "clip"):
            self._call_rows("care_gather_rows", v[k].view(n, 1), w[k].view(m, 1), idx, m)
        for k in ("fscore", "flen"):
            self._call_rows("care_gather_rows", v[k], w[k], idx, m)
        self._call_rows("care_gather_rows", v["fhyp"].view(n, -1), w["fhyp"].view(m, -1), idx, m)
        self._call_rows("care_gather_rows", v["tok"], w["tok"], idx_r, M)
        self._call_rows("care_gather_rows", v["scores"].view(N, 1), w["scores"].view(M, 1), idx_r, M)
        for a, b in zip(v["anc"], w["anc"]):
            self._call_rows("care_gather_rows", a, b, idx_r, M)
            self.call("care_remap_rows", ptr(b), b.numel(), ptr(cmap), bm)
        for a, b in zip(v["skv"], w["skv"]):
            self._call_rows("care_gather_rows", a, b, idx_r, M)
        return self._move_clips(v, w, idx, active)

    def translate_beam(self, feats: List[torch.Tensor], bm: int, need: int, use_graph: bool = True, lean: bool = False,
                       early_exit: Optional[bool] = None):
        """encode + beam search of one batch, replayed from a hipGraph when the input buffers repeat
        (same policy as translate_greedy).  Returns (enc_outputs, nfin, fscore, flen, fhyp)."""
        feats = self._prep_feats(feats)
        B = feats[0].shape[0]
        plan = self._begin_pass(self.plan_for(B, bm, need, lean=lean, early_exit=early_exit))
        if plan.decode == "resident":  # encode + ONE resident launch for the whole search
            def run_resident():
                enc = self.encode(feats, plan.lean, static=True, small=plan.small)
                return (enc,) + tuple(self.beam_resident(enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), bm, need,
                                                         sem_embs=enc.get("semantic_embs"), early_exit=plan.early_exit))
            out = self._resident_pass("beam", "bres", feats, run_resident, use_graph, "rb_scratch",
                                      self.lib.care_decode_resident_beam_scratch(B, bm, self.d, self.ff, self.V), row_steps=None)
            if out is not None:
                return out
            plan = self.plan = self.plan_for(B, bm, need, lean=lean, early_exit=early_exit)  # (refused, and noted: the other forms)
        if plan.decode == "chain":  # every step a chain of ~10 kernels (csrc/decode_chain.hip)
            return self.translate_beam_chain(feats, bm, need, use_graph, lean, plan.early_exit, plan=plan)
        if plan.early_exit:
            return self.beam_early_exit(feats, bm, need, lean, use_graph, plan=plan)

        def run():
            enc = self.encode(feats, plan.lean, small=plan.small)
            return (enc,) + tuple(self.beam(enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), bm, need,
                                            sem_embs=enc.get("semantic_embs")))

        return self._replay(forms.graph_key("beam", plan, feats), run, use_graph)

    def translate_beam_ensemble(self, others: list, feats_list: List[List[torch.Tensor]], bm: int, need: int, use_graph: bool = True):
        """encode + beam search of one batch by a LIST of models (model ensembling, models/Translator.py:39-52,112-133): this
        engine and `others` each encode their own feature list and decode the SHARED prefixes step by step; the step's word
        log-probabilities are the members' log_softmax averaged (care_ensemble_select) and ONE beam state machine
        (care_beam_advance, this engine's) advances on them.  Greedy decoding is bm = 1 (models/Wrapper.py:34-35).  Every member
        runs its multi-launch step with the vocabulary logits in memory - off the hot path ("out of scope beyond
        accepting the list"; built in round 6 so that a list of checkpoints decodes at all): no resident launch, no fused selection.
        Returns (enc_outputs of this engine, nfin, fscore, flen, fhyp) like translate_beam."""
        engines = [self] + list(others)
        B = feats_list[0][0].shape[0]
        for e in engines:
            if (e.T, e.V) != (self.T, self.V) or e.device != self.device:
                raise ValueError("ensemble members must share max_len, the vocabulary and the device")
        if len(engines) > 8:
            raise ValueError("at most 8 ensemble members (care_ensemble_select)")
        prepped = []
        for e, feats in zip(engines, feats_list):
            feats = e._prep_feats(feats)
            if feats[0].shape[0] != B:
                raise ValueError("ensemble members must see the same clips")
            # (a member steps on the shared search's rows with its logits in memory: no beam-search forms of its own)
            e._begin_pass(e.plan_for(B, rows=B * bm, early_exit=False))
            prepped.append(feats)

        def run():
            members, enc0 = [], None
            for e, feats in zip(engines, prepped):
                enc = e.encode(feats, False)
                enc0 = enc if enc0 is None else enc0
                members.append((e, enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), enc.get("semantic_embs")))
            # (the engines ride along in the result: a captured graph keeps its members alive, so their ids in the key stay theirs)
            return (enc0,) + tuple(self.beam(members[0][1], members[0][2], bm, need, sem_embs=members[0][3], others=members[1:])) + (tuple(engines),)

        # replayed from a hipGraph like the single-model passes; the key carries every member's identity, feature buffers and
        # epoch (an engine that dropped workspaces or re-packed weights since the capture: engine._epoch)
        key = forms.graph_key("ens", self.plan, [f for feats in prepped for f in feats], bm, need,
                              tuple((id(e), e._epoch, e.plan) for e in engines))
        return self._replay(key, run, use_graph)[:-1]

    def beam(self, mem: torch.Tensor, sem: Optional[torch.Tensor], bm: int, need: int,
             sem_embs: Optional[torch.Tensor] = None, others=()):
        """Beam search of B clips x bm beams, state on the device (csrc/beam.hip).  others: further ensemble members as
        (engine, mem, sem, sem_embs) - see translate_beam_ensemble."""
        B, Lk, d = mem.shape
        T, N = self.T, mem.shape[0] * bm
        mem = mem.to(self.device, mem.dtype if mem.dtype == self.h16 else torch.float32)  # bf16: lean encode
        sem = sem.to(self.device, torch.float32).contiguous() if sem is not None else None
        v = dict(self._beam_state("b_", B, bm, need), tag="b_", n=B, Lk=Lk, sem=sem)
        self._beam_init(v, torch.arange(N, device=self.device, dtype=torch.int32))
        if others:
            # model ensembling: every member steps on the shared prefixes (tok / ancestors) with state of its own, its
            # vocabulary logits in memory; the averaged log-probabilities' top bm -> the one state machine
            cval, cidx = self.ws("b_cval", (N, bm)), self.ws("b_cidx", (N, bm), torch.int32)
            vpad = (self.V + 63) // 64 * 64  # 16-byte aligned row stride -> the GEMM's vector store path
            per = []
            for e, m, s_, se in [(self, mem, sem, sem_embs)] + list(others):
                m = m.to(e.device, m.dtype if m.dtype == e.h16 else torch.float32)
                s_ = s_.to(e.device, torch.float32).contiguous() if s_ is not None else None
                per.append(dict(e=e, sem=s_, ckv=e.cross_src(m, N), akv=e.attr_kv(se) if e.attr_att else None, Lk=m.shape[1],
                                skv=[e.ws("b_skv%d" % li, (N, T, 2 * e.d), e.wt) for li in range(e.n_layers)],
                                logits=e.ws("b_logits", (N, vpad))))
            rows_ptr = (ctypes.c_void_p * len(per))(*[p["logits"].data_ptr() for p in per])
            for t in range(1, T + 1):
                for p in per:
                    e = p["e"]
                    x, xb = e._decode_step(t, N, bm, v["tok"], v["anc"][(t - 1) & 1], p["sem"], p["ckv"], p["skv"], p["Lk"], "b_",
                                           akv=p["akv"])
                    e.gemm(xb if xb is not None else x, e.w["vocab"], None, p["logits"][:, : self.V])
                self.call("care_ensemble_select", rows_ptr, len(per), vpad, self.V, bm, ptr(cval), ptr(cidx), N)
                self._beam_advance(v, t, bm, need, cval, cidx)
        else:
            v["ckv"] = self.cross_src(mem, N)
            v["akv"] = self.attr_kv(sem_embs) if self.attr_att else None
            v["skv"] = [self.ws("b_skv%d" % li, (N, T, 2 * d), self.wt) for li in range(self.n_layers)]
            self._beam_steps(v, 1, T, bm, need)
        return v["nfin"], v["fscore"], v["flen"], v["fhyp"]

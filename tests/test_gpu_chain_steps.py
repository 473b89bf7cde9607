"""GPU: the chained beam step (care_decode_chain_beam, csrc/decode_chain.hip; its state machine beam_init_phase / beam_advance_phase,
csrc/decode_beam_phase.h, is shared with the resident beam launches) audited against float64 AFTER EVERY STEP.

The chain is driven one step per call (t0 == t1 == t, engine.beam_chain_steps(..., count_live=False)); after every step the whole
state comes to the host and tests/chain_reference.py audits it (teeth: tests/test_chain_reference_cpu.py):
  (b) the selection - exact where the device's own numbers decide (first step from row 0 only, parents live, slot count, distinct
      pairs, scores non-increasing, ties by ascending parent * V + token, empty slots = (0, EOS, -1e20)); within a bar against
      float64 where 16-bit arithmetic decides: |score - (previous score + logp64)| <= bar, no omitted candidate of the WHOLE pool
      (live parents x all V tokens) better than the smallest kept one by more than 2 bar, the kept ones ordered within 2 bar;
  (c) the transition - S_prev -> BeamStateRef.step(t, chosen = the device's choice) == S_new: token table, both ancestor tables,
      scores, done, nfin, fscore, flen, fhyp, whole tables, bit for bit (for t == 1 S_prev is what beam_init_phase writes over
      whatever the tables held).
No clip and no step is left out; the search goes on two steps past the one at which every clip is done (frozen clips).

float64: oracle.care_cpu on the parameters and features in double - encoding_phase once; per step decoding_phase(...,
last_time_step_logits=True) + log_softmax on the prefixes walked out of the DEVICE's tables (S_prev's ancestor table), so nothing
carries over between steps on the reference side.  bar = tests/test_gpu_parity.py MODES[mode]["lse_peaked"] (one log-probability
on the peaked model), 2 bar for a difference of two.  Cases 5 and 6 (130 / 260 rows) run (c) and the exact part of (b) after every
step, the float64 part at steps 1 .. 4 and at every step at which a clip records a hypothesis.

Self-attention cache (cb_skv*): the QKV phase stores K | V of a row at position t - 1 and nowhere else (csrc/decode_resident.h,
gemm_phase E_QKV) - after step t every other position of every row is bit-identical to what it was, position t - 1 is finite.

Differences from care_beam_advance: none found - the restatement of csrc/beam.hip's step holds for the chain bit for bit, frozen
clips, the all-ended ending and the capacity of the finished lists included; beam_init_phase zeroes the finished lists WHOLE (all
need + bm slots, every column of the stride), where the host-side initialisation of the multi-launch search zeroes the same bytes.

The per-step error against float64, which nobody had measured: on these models (vocabulary rows scaled by 3 .. 20, logits of
+-30) a kept score is further than lse_peaked from float64 at a few (row, token)s of cases 4, 6, 7, 8 and 9 - up to 2.16 x the
bar (case 8, bf16, two layers).  Scored teacher-forced through the multi-launch path of the same mode (framework.decoding_phase ->
engine.decode_full on the same prefixes: independent code, tested against float64 kernel by kernel), the same (row, token)s are
off by errors of the same size wherever the chain is far past the bar (cases 6, 8, 9) - the noise of a 16-bit logit on a scaled
row, not the chain's - and by less (0.16 .. 0.29 bars) at three (row, token)s of cases 4 and 7, where the chain is within 1.35
bars.  Worst of the chain | the
multi-launch path at the (row, token)s past the bar, in bars: case 4 1.005 | 0.29; case 6 1.18 | 0.73, 0.74, 0.91; case 7 1.35 |
0.16, 0.28, 0.87, 0.84; case 8 2.16 | 1.69, 1.95; case 9 1.33 | 1.005.  So
past the bar the check is relative to that path, as measured at that very (row, token): |score - float64| <= lse_peaked + 2 x the
multi-launch path's error there.  Worst share of that allowance: 0.90.  The other two float64 checks hold as they are: no
omitted candidate is better than the smallest kept one by more than 0.23 x (2 bar), the kept order is within 0.33 x (2 bar).

*Measured* on one MI355X (pytest -s), worst figure as a share of its bar - score / bar, (score / its allowance where past the
bar), omitted / 2 bar, kept order / 2 bar - steps run (with float64), branches of the state machine the device went through:
   1 care, 1 clip, fp16              0.10  (-)     0.00  0.00   11 (9)   need 1, frozen 2
   2 base_ami, 3 clips, need 8, bf16 0.97  (-)     0.00  0.00    7 (5)   need 2, all_ended 1, frozen 9
   3 care, 4 clips, fp16             0.77  (-)     0.00  0.00   14 (12)  need 4, frozen 26
   4 cabase, 13 clips, fp16          1.005 (0.64)  0.00  0.04    6 (4)   need 13, frozen 37      (forms 0 / 1 / 3: the same figures)
   5 care, 26 clips, bf16            0.89  (-)     0.03  0.03   23 (9)   need 26, frozen 451
   6 base_ami, 52 clips, fp16        1.18  (0.47)  0.00  0.01   10 (6)   need 52, frozen 289
   7 care, 5 clips, bf16, beam 2     0.80  (-)     0.00  0.00    4 (2)   need 5, frozen 10
     beam 3 need 4 / beam 4 need 4   1.35  (0.90)  0.00  0.00    7 (5)   need 5, frozen 18 / 22
   8 base_ami, 2 layers, bf16        2.16  (0.44)  0.23  0.33   23 (21)  need 3, frozen 32
   9 base_ami, max_len 6, fp16       0.09  (-)     0.00  0.00    5 (5)   maxlen_empty 6
     care, max_len 8, fp16           1.33  (0.44)  0.00  0.00    7 (7)   need 2, maxlen_some 4, frozen 8
  10 base_ami, ff 1024, bf16         0.99  (-)     0.00  0.01    7 (5)   need 5, frozen 14
  11 = 3 on the test's own tables    0.77  (-)     0.00  0.00   14 (12)  need 4, frozen 26
Branches over the file: need 153, maxlen_empty 6, maxlen_some 4, all_ended 1, frozen 1018, boundary_tie 0 - an exact tie of two
fp32 scores at the pruning edge is the one branch a real model does not reach (the scripted searches of
tests/test_gpu_beam_state.py force it for care_beam_advance; here the tie ORDER is checked wherever two kept scores are equal).
The seeds, boosts and max_len values were chosen on the CPU: the float64 oracle free-running into BeamStateRef on the same seeds
and features says which branches a case reaches and after how many steps every clip is done.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_reference as cr
from beam_reference import BRANCHES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MIXED = {"cls_head.tgt_word_prj.weight": {3: 14.0, 0: 3.0}}  # clips ending at mixed steps, generated PADs
PEAKED_ROWS = {"cls_head.tgt_word_prj.weight": {**{r: 12.0 for r in range(6, 46)}, 3: 20.0}}  # tests/test_gpu_properties.py
SENT, FSENT = -77, -12345.0
TOTAL = {k: 0 for k in BRANCHES}  # branches of the state machine the cases of this file went through (printed by the last test)



def _setup(config, B, mode, seed, boost, **overrides):
    """tests/test_gpu_properties.py::_setup with make_opt overrides, features that the CPU can make too (care_amd.synth), and the
    float64 side: parameters in double and the decoder inputs of the B clips from ONE encoding_phase."""
    from care_amd import get_framework
    from care_amd.configs import feat_shapes, make_opt
    from care_amd.synth import synth_feats, synth_state_dict
    from oracle import care_cpu

    opt = make_opt(config, **overrides)
    model = get_framework(opt).eval()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    P = synth_state_dict(seed, shapes, row_scale=boost)
    model.load_state_dict(P, strict=True)
    model.set_compute_dtype(mode)
    model.to(DEV)
    feats = synth_feats(seed, feat_shapes(opt, B))
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        inputs = care_cpu.inputs_for_decoder(opt, care_cpu.encoding_phase(P64, opt, [f.double() for f in feats]))
    eng = model.engine()
    eng.LATENT_MIN_ROWS = 1
    eng.resident_max_rows, eng.resident_beam_max_rows, eng.chain_beam_max_rows = 256, 0, 4096
    return opt, P64, inputs, mode, eng, [f.to(DEV) for f in feats], model


def multi_launch_logp(model, feats, S_prev, t, bm, clips):
    """The same log-probabilities from the multi-launch path of the model's mode - the stateless decoder call on the whole prefix
    (framework.decoding_phase -> engine.decode_full: independent code, tested against float64 kernel by kernel) - as
    {row: [V] float64} for the rows of `clips`.  Only asked where a score of the chain is further than the bar from float64."""
    eng = model.engine()
    plan = eng.plan
    try:
        rows = np.array([b * bm + i for b in clips for i in range(bm)])
        ids = torch.from_numpy(cr.prefixes(S_prev, rows, t)).to(DEV)
        enc = model.encoding_phase(feats)
        clip = torch.from_numpy(rows // bm).to(DEV)
        inputs = {k: v[clip].contiguous() for k, v in model.prepare_inputs_for_decoder(enc, {}).items() if v is not None}
        logits = model.decoding_phase(ids, inputs, last_time_step_logits=True)["logits"]
        logp = torch.log_softmax(logits.double().view(len(rows), -1), dim=1).cpu().numpy()
    finally:
        eng.plan = plan
    return {int(r): logp[k] for k, r in enumerate(rows)}


def logp64_of(opt, P64, inputs, S_prev, t, bm, V, clips):
    """float64 log-probabilities [B*bm, V] of the next token of every row's own prefix (walked through S_prev), rows of the
    clips in `clips`; the other rows NaN (never read)."""
    from oracle import care_cpu

    n = S_prev["done"].shape[0] * bm
    out = np.full((n, V), np.nan)
    if not len(clips):
        return out
    rows = np.array([b * bm + i for b in clips for i in range(bm)])
    ids = torch.from_numpy(cr.prefixes(S_prev, rows, t))
    per_row = {k: v[torch.from_numpy(rows // bm)] for k, v in inputs.items() if v is not None}
    with torch.no_grad():
        logits = care_cpu.decoding_phase(P64, opt, ids, per_row, last_time_step_logits=True)["logits"]
        out[rows] = torch.log_softmax(logits, dim=1).numpy()
    return out


class Chain:
    """One search of B clips driven step by step.  own=False: through engine.beam_chain_steps (the engine's `cb_` state);
    own=True: a direct call of care_decode_chain_beam on tables of the test's own - stride T + 3, one guard clip of sentinels
    behind every table, finished lists pre-filled with sentinels."""

    def __init__(self, eng, feats, bm, need, own=False):
        self.eng, self.bm, self.need, self.own = eng, bm, need, own
        feats = eng._prep_feats(feats)
        self.B, self.T, self.V = feats[0].shape[0], eng.T, eng.V
        B, T, N, cap = self.B, self.T, self.B * bm, need + bm
        plan = eng._begin_pass(eng.plan_for(B, bm, need, lean=True, early_exit=True))
        assert plan.decode == "chain", plan
        enc = eng.encode(feats, plan.lean, static=True, small=plan.small)
        self.mem, self.sem, self.sem_embs = enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), enc.get("semantic_embs")
        if own:
            stride = T + 3

            def table(rows, tail, dtype, fill):
                return torch.full((rows,) + tail, fill, device=DEV, dtype=dtype)

            self.v = dict(tok=table(N + bm, (stride,), torch.int32, SENT), anc0=table(N + bm, (stride,), torch.int32, SENT),
                          anc1=table(N + bm, (stride,), torch.int32, SENT), scores=table(N + bm, (), torch.float32, FSENT),
                          done=table(B + 1, (), torch.int32, SENT), nfin=table(B + 1, (), torch.int32, SENT),
                          fscore=table(B + 1, (cap,), torch.float32, FSENT), flen=table(B + 1, (cap,), torch.int32, SENT),
                          fhyp=table(B + 1, (cap, stride), torch.int32, SENT))
        else:
            v = eng._beam_state("cb_", B, bm, need)
            self.v = dict(tok=v["tok"], anc0=v["anc"][0], anc1=v["anc"][1], **{k: v[k] for k in cr.TABLES[3:]})
        self.skv = [eng.ws("cb_skv%d" % li, (N, T, 2 * eng.d), eng.h16) for li in range(eng.n_layers)]

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: self.v[k].cpu().numpy().copy() for k in cr.TABLES}

    def step(self, t):
        from care_amd._lib import ptr
        from care_amd.constants import BOS, EOS, PAD

        eng, B, bm, need, T = self.eng, self.B, self.bm, self.need, self.T
        if not self.own:
            eng.beam_chain_steps(self.mem, self.sem, bm, need, t, t, sem_embs=self.sem_embs, count_live=False)
            return
        d, Lk = eng.d, self.mem.shape[1]
        sem = self.sem.to(DEV, torch.float32).contiguous() if self.sem is not None else None
        if t == 1:
            self.kv = (eng.cross_kv(self.mem, tag="cb_ckv", resident=True),
                       eng.attr_kv(self.sem_embs, tag="cb_akv") if eng.attr_att else None)
        layers = eng._resident_layers("cb_", B * bm, bm, self.kv[0], self.kv[1], Lk)
        nbytes = eng.lib.care_decode_chain_beam_scratch(B, bm, d, eng.ff, eng.V)
        scratch = eng.ws("cb_scratch", (nbytes,), torch.uint8)
        v = self.v
        eng.call("care_decode_chain_beam", ctypes.addressof(layers), eng.n_layers, *eng._model_args(sem, d), B, bm, need, T, t, t,
                 BOS, EOS, PAD, ptr(v["tok"]), v["tok"].stride(0), ptr(v["anc0"]), ptr(v["anc1"]),
                 *(ptr(v[k]) for k in ("scores", "done", "nfin", "fscore", "flen", "fhyp")), need + bm, ptr(scratch), nbytes,
                 int(os.environ.get("CARE_CHAIN_FORM", "-1")), tag="decode_chain_beam")


def run_case(name, setup, bm, need, own=False, sparse=False, cache=None):
    """The search of one case, audited after every step.  sparse: the float64 part of (b) only at steps 1 .. 4 and where a clip
    records a hypothesis.  cache: float64 log-probabilities by (step, prefixes) - the forms of one case walk the same prefixes
    unless a near-tie falls the other way.  Returns (steps run, branch counts)."""
    from test_gpu_parity import MODES

    opt, P64, inputs, mode, eng, feats, model = setup
    bar = MODES[mode]["lse_peaked"]
    ch = Chain(eng, feats, bm, need, own=own)
    B, T, V = ch.B, ch.T, ch.V
    count = {k: 0 for k in BRANCHES}
    worst = dict(score=0.0, omitted=0.0, order=0.0, relative=0.0)
    S_prev = cr.initial_state(ch.snapshot(), B, bm, T)
    all_done_at, audited, t = None, 0, 0
    while t < T and (all_done_at is None or t < all_done_at + 2):
        t += 1
        before = [k.clone() for k in ch.skv]
        ch.step(t)
        S_new = ch.snapshot()
        for li, (a, b) in enumerate(zip(before, ch.skv)):
            a, b = a.view(torch.int16), b.view(torch.int16)
            other = [p for p in range(T) if p != t - 1]
            assert torch.equal(a[:, other], b[:, other]), (name, t, li, "a position other than t - 1 of the cache was written")
            assert bool(torch.isfinite(ch.skv[li][:, t - 1].float()).all()), (name, t, li)
        live = [b for b in range(B) if not S_prev["done"][b]]
        records = bool((S_new["nfin"][:B] != S_prev["nfin"][:B]).any())
        logp64 = None
        if live and (not sparse or t <= 4 or records):
            key = (t, cr.prefixes(S_prev, np.arange(B * bm), t).tobytes(), S_prev["done"][:B].tobytes())
            if cache is not None and key in cache:
                logp64 = cache[key]
            else:
                logp64 = logp64_of(opt, P64, inputs, S_prev, t, bm, V, live)
                if cache is not None:
                    cache[key] = logp64
            audited += 1
        other = {}

        def yardstick(row, token, S_prev=S_prev, t=t, live=live, logp64=logp64, other=other):
            if not other:
                other.update(multi_launch_logp(model, feats, S_prev, t, bm, live))
            err = abs(float(other[row][token]) - float(logp64[row, token]))
            print("\n{}: step {}: row {} token {}: the multi-launch path is {:.3f} x bar from float64".format(
                name, t, row, token, err / bar))
            return err

        try:
            w, ref = cr.audit_step(S_prev, S_new, t, B, bm, need, T, V, logp64, bar, yardstick)
        except cr.AuditFailure as exc:
            raise AssertionError("{}: step {}: {}".format(name, t, exc)) from exc
        for k in worst:
            worst[k] = max(worst[k], w[k])
        for k in BRANCHES:
            count[k] += ref.count[k]
        if all_done_at is None and S_new["done"][:B].all():
            all_done_at = t
        S_prev = S_new
    assert all_done_at is not None, (name, "the search did not end within T steps")
    hit = {k: n for k, n in count.items() if n}
    print("\n{}: worst / bar: score {:.3f} (past the bar: {:.3f} of bar + 2 x multi-launch error) omitted {:.3f} kept order {:.3f}; "
          "{} steps ({} with float64, all done at {}); {}".format(name, worst["score"], worst["relative"], worst["omitted"],
                                                                  worst["order"], t, audited, all_done_at, hit))
    for k in BRANCHES:
        TOTAL[k] += count[k]
    return t, count


def test_one_row_group_two_step_list_fetch():
    """Case 1: one clip x beam 5 = one row tile: a vocabulary part per column item (165) and the two-step list fetch."""
    _, count = run_case("1 care B1 fp16", _setup("msrvtt_care", 1, "fp16", 101, MIXED), 5, 5)
    assert count["need"] + count["all_ended"] > 0 and count["frozen"] > 0, count


def test_need_above_beam_size():
    """Case 2: need 8 > beam 5."""
    _, count = run_case("2 base_ami B3 need8 bf16", _setup("msrvtt_base_ami", 3, "bf16", 203, MIXED), 5, 8)
    assert count["need"] + count["all_ended"] > 0 and count["frozen"] > 0, count


def test_two_row_tiles_48_parts():
    """Case 3: 20 rows: two row tiles, 48 parts, the one-step fetch."""
    _, count = run_case("3 care B4 fp16", _setup("msrvtt_care", 4, "fp16", 103, MIXED), 5, 5)
    assert count["need"] > 0 and count["frozen"] > 0, count


def test_ragged_fifth_tile_in_every_form():
    """Case 4: 65 rows: form 1 with a ragged fifth tile; again with CARE_CHAIN_FORM 0 and 3 (3: two row groups)."""
    setup = _setup("msrvtt_cabase", 13, "fp16", 104, MIXED)
    cache = {}
    assert "CARE_CHAIN_FORM" not in os.environ
    run_case("4 cabase B13 fp16 form by rows", setup, 5, 5, cache=cache)
    for form in ("0", "3"):
        os.environ["CARE_CHAIN_FORM"] = form
        try:
            run_case("4 cabase B13 fp16 form " + form, setup, 5, 5, cache=cache)
        finally:
            del os.environ["CARE_CHAIN_FORM"]


def test_clip_shared_kv_fetch_130_rows():
    """Case 5: 130 rows: the beams of a clip share a K/V fetch (rows >= 128), two row tiles per vocabulary fetch."""
    run_case("5 care B26 bf16", _setup("msrvtt_care", 26, "bf16", 207, MIXED), 5, 5, sparse=True)


def test_form_3_by_row_count_260_rows():
    """Case 6: 260 rows: form 3 by the row count."""
    run_case("6 base_ami B52 fp16", _setup("msrvtt_base_ami", 52, "fp16", 106, MIXED), 5, 5, sparse=True)


def test_small_beams():
    """Case 7: beams of 2, 3 and 4 (need 2, 4, 4) on one model."""
    setup = _setup("msrvtt_care", 5, "bf16", 107, PEAKED_ROWS)
    for bm, need in ((2, 2), (3, 4), (4, 4)):
        run_case("7 care B5 bf16 beam {} need {}".format(bm, need), setup, bm, need)


def test_two_decoder_layers():
    """Case 8: a decoder of two layers: the second layer's phases (LayerNorm on load of the first layer's FFN output)."""
    run_case("8 base_ami 2 layers B3 bf16", _setup("msrvtt_base_ami", 3, "bf16", 108, MIXED, num_hidden_layers_decoder=2), 5, 5)


def test_max_length_endings():
    """Case 9: the endings at the maximum length - max_len 6 (T = 5) on a model that never ends a caption by itself (every clip
    ends with nothing finished), and max_len 8 on one whose clips end at mixed steps (some with a part of their hypotheses)."""
    _, count = run_case("9a base_ami max_len 6 B6 fp16", _setup("msrvtt_base_ami", 6, "fp16", 109, None, max_len=6), 5, 5)
    assert count["maxlen_empty"] > 0, count
    _, count = run_case("9b care max_len 8 B6 fp16", _setup("msrvtt_care", 6, "fp16", 109, MIXED, max_len=8), 5, 5)
    assert count["maxlen_empty"] + count["maxlen_some"] > 0, count


def test_narrow_ffn():
    """Case 10: intermediate_size 1024 (no configuration of configs.py has d_model 512 with an FFN other than 2048: an override of
    msrvtt_base_ami, which forms.chain_beam accepts): the one form of the narrow FFNs."""
    setup = _setup("msrvtt_base_ami", 5, "bf16", 110, MIXED, intermediate_size=1024)
    assert setup[4].chain_beam_ok(5, 5, 5) and setup[4].ff == 1024
    run_case("10 base_ami ff 1024 B5 bf16", setup, 5, 5)


def test_direct_call_on_the_tests_own_tables():
    """Case 11: case 3 through a direct call: tables of stride T + 3 with a guard clip of sentinels behind each and finished lists
    full of sentinels - whole-table equality says that nothing outside the state is written."""
    _, count = run_case("11 care B4 fp16 own tables", _setup("msrvtt_care", 4, "fp16", 103, MIXED), 5, 5, own=True)
    assert count["need"] > 0 and count["frozen"] > 0, count
    print("\nbranches over the cases run:", TOTAL)

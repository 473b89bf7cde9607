"""tests/chain_reference.py (the yardstick of tests/test_gpu_chain_steps.py) has teeth - shown without a GPU.  The device is played by
tests/beam_reference.py's BeamStateRef on the scripted searches; the auditor is fed float64 log-probabilities that are the
script's plus noise of up to bar / 4 (a 16-bit device is further from float64 than that script is from itself).  The unmutated
restatement passes every step; every mutant and every hand-made fault is rejected, by a check of the expected name."""
import numpy as np
import pytest

import chain_reference as cr
from beam_reference import EOS, MUTANTS, SEED, BeamStateRef, candidates, script

BAR = 5e-3  # (any bar far above fp32 rounding of a sum of two log-probabilities serves here)
SENT, FSENT, UNWRITTEN = -77, -12345.0, -5
SHAPES = [(9, 5, 7, 12, 37), (13, 3, 5, 30, 16), (5, 2, 2, 12, 37)]
# which check has to object to which wrong rule
EXPECT = dict(tie_desc={"tie_order"}, first_all={"first_step_row0"}, ended_stay={"ended_parent"},
              need_plus1={"transition_done", "transition_nfin", "transition_fscore", "transition_tok"})


def _snap(ref):
    return {k: v.copy() for k, v in ref.arrays().items()}


def _noisy(logp, t, seed):
    rng = np.random.RandomState(1000 * seed + t)
    return logp[t - 1].astype(np.float64) + rng.uniform(-BAR / 4, BAR / 4, size=logp[t - 1].shape)


def play(shape, ties, mutant=None):
    """The scripted search as a `device` would leave it: [(t, S_prev, S_new)] of every step, and the script.  Guards and the
    finished lists start as sentinels, the token columns after BOS as a value no step writes."""
    B, bm, need, T, V = shape
    logp = script(B, bm, T, V, SEED, ties)
    dev = BeamStateRef(B, bm, need, T, V, sentinel=SENT, fsentinel=FSENT, guard=1, mutant=mutant)
    dev.tok[: B * bm, 1:] = UNWRITTEN
    steps = []
    for t in range(1, T + 1):
        prev = _snap(dev)
        dev.step(t, *candidates(logp[t - 1], bm))
        steps.append((t, prev, _snap(dev)))
    return steps, logp


_plays = {}


def good(shape, ties):
    if (shape, ties) not in _plays:
        _plays[(shape, ties)] = play(shape, ties)
    return _plays[(shape, ties)]


def audit(shape, t, prev, new, logp64):
    B, bm, need, T, V = shape
    return cr.audit_step(prev, new, t, B, bm, need, T, V, logp64, BAR)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_passes_every_step(shape, ties):
    steps, logp = good(shape, ties)
    hit = {}
    for t, prev, new in steps:
        worst, ref = audit(shape, t, prev, new, _noisy(logp, t, 1))
        assert worst["score"] <= 0.26 and worst["omitted"] <= 0.26 and worst["order"] <= 0.26, (t, worst)
        for k, n in ref.count.items():
            hit[k] = hit.get(k, 0) + n
    assert hit["need"] > 0 and hit["frozen"] > 0, hit


def test_the_initial_state_is_what_the_first_step_starts_from():
    """initial_state() of tables full of other values == the state a fresh restatement starts from, whatever was pre-filled
    beyond what the initialisation writes (stride T + 3, a guard clip) staying."""
    B, bm, need, T, V = 4, 3, 5, 9, 16
    ref = BeamStateRef(B, bm, need, T, V)
    rng = np.random.RandomState(3)
    N, cap, stride = B * bm, need + bm, T + 3
    junk = dict(tok=rng.randint(-9, 9, (N + bm, stride)), anc0=rng.randint(-9, 9, (N + bm, stride)),
                anc1=rng.randint(-9, 9, (N + bm, stride)), scores=rng.randn(N + bm), done=rng.randint(1, 9, (B + 1,)),
                nfin=rng.randint(1, 9, (B + 1,)), fscore=rng.randn(B + 1, cap), flen=rng.randint(1, 9, (B + 1, cap)),
                fhyp=rng.randint(1, 9, (B + 1, cap, stride)))
    junk = {k: v.astype(np.float32 if k in ("scores", "fscore") else np.int32) for k, v in junk.items()}
    S = cr.initial_state(junk, B, bm, T)
    for k, want in ref.arrays().items():
        if k == "fhyp":
            assert np.array_equal(S[k][:B, :, : T + 1], want) and not S[k][:B].any()
        elif want.ndim == 2 and want.shape[1] == T + 1:
            assert np.array_equal(S[k][:N, : T + 1], want), k
            assert np.array_equal(S[k][:N, T + 1:], junk[k][:N, T + 1:]), k
        else:
            assert np.array_equal(S[k][: want.shape[0]], want), k
        assert np.array_equal(S[k][want.shape[0]:], junk[k][want.shape[0]:]), k  # the guards


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_rule_is_rejected(mutant):
    """A device with one wrong rule is caught at the first step at which the rule matters - and by the check that names it."""
    caught = []
    for shape in SHAPES[:2]:
        for ties in (False, True):
            steps, logp = play(shape, ties, mutant)
            for t, prev, new in steps:
                try:
                    audit(shape, t, prev, new, _noisy(logp, t, 2))
                except cr.AuditFailure as exc:
                    assert exc.check in EXPECT[mutant], (mutant, shape, ties, t, exc)
                    caught.append((shape, ties, t, exc.check))
                    break
    assert caught, mutant


def test_a_score_off_by_more_than_the_bar_is_rejected_unless_the_yardstick_is_as_far():
    """A kept score 1.5 x bar from float64: rejected as `score_value`; accepted where the independent implementation is 0.3 x bar
    from float64 at that log-probability (allowance bar + 2 x 0.3 bar), rejected again where it is only 0.2 x bar off."""
    shape = SHAPES[0]
    B, bm, need, T, V = shape
    steps, logp = good(shape, False)
    t, prev, new = steps[3]
    b = int(np.flatnonzero(prev["done"][:B] == 0)[0])
    parent, token, _ = cr.read_choice(new, b, bm, t)
    logp64 = logp[t - 1].astype(np.float64)
    logp64[b * bm + parent[1], token[1]] += 1.5 * BAR

    def go(other):
        asked = []

        def yardstick(row, tok):
            asked.append((row, tok))
            return other * BAR
        try:
            cr.audit_step(prev, new, t, B, bm, need, T, V, logp64, BAR, yardstick if other is not None else None)
        except cr.AuditFailure as exc:
            return exc.check, asked
        return None, asked

    assert go(None)[0] == "score_value" and go(0.2)[0] == "score_value"
    check, asked = go(0.3)
    assert check is None and asked == [(b * bm + int(parent[1]), int(token[1]))]


def _rejected(shape, t, prev, new, logp64):
    try:
        audit(shape, t, prev, new, logp64)
    except cr.AuditFailure as exc:
        return exc.check
    return None


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_a_kept_candidate_replaced_by_a_worse_one_is_rejected(shape, ties):
    """The last kept candidate of a clip replaced by one that is 3 x bar worse (the rest of the step consistent with that choice,
    so only the selection audit can object): rejected as `omitted_better`.  The same with a candidate 1 x bar worse - inside what
    16-bit arithmetic can decide either way - passes."""
    B, bm, need, T, V = shape
    steps, logp = good(shape, ties)
    tried = 0
    for t, prev, new in steps[1:]:
        for b in range(B):
            if prev["done"][b] or tried >= 6:
                continue
            parent, token, score = cr.read_choice(new, b, bm, t)
            if score[bm - 1] <= cr.EMPTY:
                continue
            p = int(parent[0])
            taken = {int(token[i]) for i in range(bm) if parent[i] == p}
            col = next(c for c in range(V) if c not in taken and c != EOS)
            for k, want in ((3, "omitted_better"), (1, None)):
                lp = logp[t - 1].copy()
                lp[b * bm + p, col] = np.float32(np.float64(score[bm - 1]) - k * BAR - np.float64(prev["scores"][b * bm + p]))
                sc = score.copy()
                sc[bm - 1] = np.float32(lp[b * bm + p, col] + prev["scores"][b * bm + p])
                ch = [cr.read_choice(new, c, bm, t) for c in range(B)]
                ch[b] = (np.r_[parent[:-1], p], np.r_[token[:-1], col], sc)
                for c in range(B):
                    if prev["done"][c]:
                        ch[c] = (np.zeros(bm, dtype=np.int64),) + tuple(ch[c][1:])
                dev = BeamStateRef.from_arrays(prev, B, bm, need, T, V)
                dev.step(t, chosen=ch)
                rng = np.random.RandomState(7 * t + b)
                logp64 = lp.astype(np.float64) + rng.uniform(-BAR / 4, BAR / 4, size=lp.shape)
                assert _rejected(shape, t, prev, _snap(dev), logp64) == want, (t, b, k)
            tried += 1
    assert tried > 0


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_a_finished_hypothesis_one_off_is_rejected(shape, ties):
    """A finished hypothesis written one position off, and one written one slot off: rejected by the exact transition."""
    B, bm, need, T, V = shape
    steps, logp = good(shape, ties)
    tried = 0
    for t, prev, new in steps:
        for b in np.flatnonzero(new["nfin"][:B] > prev["nfin"][:B]):
            slot = int(prev["nfin"][b])
            if slot + 1 >= new["fhyp"].shape[1]:
                continue
            bad = {k: v.copy() for k, v in new.items()}
            bad["fhyp"][b, slot] = np.roll(new["fhyp"][b, slot], 1)
            assert _rejected(shape, t, prev, bad, _noisy(logp, t, 3)) == "transition_fhyp", (t, b)
            bad = {k: v.copy() for k, v in new.items()}
            bad["fhyp"][b, slot], bad["fhyp"][b, slot + 1] = new["fhyp"][b, slot + 1], new["fhyp"][b, slot]
            assert _rejected(shape, t, prev, bad, _noisy(logp, t, 3)) == "transition_fhyp", (t, b)
            tried += 1
    assert tried > 0


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_a_frozen_clip_left_unwritten_is_rejected(shape, ties):
    """A clip that is done and whose token column of the step stays as it was: rejected by the exact transition."""
    B, bm, need, T, V = shape
    steps, logp = good(shape, ties)
    tried = 0
    for t, prev, new in steps:
        for b in np.flatnonzero(prev["done"][:B]):
            bad = {k: v.copy() for k, v in new.items()}
            bad["tok"][b * bm:(b + 1) * bm, t] = prev["tok"][b * bm:(b + 1) * bm, t]
            assert _rejected(shape, t, prev, bad, _noisy(logp, t, 4)) == "transition_tok", (t, b)
            tried += 1
    assert tried > 0

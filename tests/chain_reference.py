"""The per-step auditor of the chained beam step (care_decode_chain_beam: csrc/decode_chain.hip with the state machine of
csrc/decode_beam_phase.h), in plain numpy.  It looks at ONE step from the outside: the state before it (S_prev) and after it (S_new),
both as BeamStateRef.arrays() names them, and the float64 log-probabilities of every row's own prefix.

(a) the device's choice is read back from S_new;  (b) the SELECTION is audited - exactly where the device's own numbers decide
(first step, live parents, slot count, distinct pairs, order and tie order), within a bar against float64 where 16-bit arithmetic
does (the kept scores, nothing omitted that is better than what was kept, the order of the kept);  (c) the TRANSITION is exact:
S_prev -> BeamStateRef.step(t, chosen = the device's choice) must be S_new, every table, bit for bit.

The yardstick of tests/test_gpu_chain_steps.py; its teeth are shown in tests/test_chain_reference_cpu.py.  No GPU here."""
import numpy as np

from beam_reference import BOS, EOS, BeamStateRef

EMPTY = np.float32(-1e19)  # a slot whose score is not above this holds no candidate
TABLES = ("tok", "anc0", "anc1", "scores", "done", "nfin", "fscore", "flen", "fhyp")


class AuditFailure(AssertionError):
    """One check of the audit that did not hold: `check` is its name."""

    def __init__(self, check, detail):
        super().__init__("{}: {}".format(check, detail))
        self.check = check


def _require(ok, check, *detail):
    if not ok:
        raise AuditFailure(check, detail)


def initial_state(S, B, bm, T):
    """What beam_init_phase (csrc/decode_beam_phase.h) leaves of the tables `S` (any content, any stride >= T + 1, any guards):
    the token table BOS / EOS up to column T, both ancestor tables the row's own index up to column T, scores and flags 0, the
    clips' finished lists zeroed whole; everything else as it was.  The S_prev of step 1."""
    S = {k: np.array(v, copy=True) for k, v in S.items()}
    N = B * bm
    S["tok"][:N, : T + 1] = EOS
    S["tok"][:N, 0] = BOS
    for k in ("anc0", "anc1"):
        S[k][:N, : T + 1] = np.arange(N, dtype=np.int32)[:, None]
    S["scores"][:N] = 0
    for k in ("done", "nfin", "fscore", "flen", "fhyp"):
        S[k][:B] = 0
    return S


def read_choice(S_new, b, bm, t):
    """(a): what the device chose for clip b at step t, slot by slot: (parent[bm], token[bm], score[bm] fp32).  The parent of a
    slot is where its ancestor of position t - 1 sits: a row's ancestor at the last written position is the row itself."""
    row0 = b * bm
    token = S_new["tok"][row0:row0 + bm, t].astype(np.int64)
    score = S_new["scores"][row0:row0 + bm].astype(np.float32)
    parent = S_new["anc%d" % (t & 1)][row0:row0 + bm, t - 1].astype(np.int64) - row0
    return parent, token, score


def live_parents(S_prev, b, bm, t):
    """Which slots of clip b hold a hypothesis in S_prev that step t can extend (its last token is not EOS)."""
    if t == 1:
        return [True] * bm
    a_old = S_prev["anc%d" % ((t - 1) & 1)]
    return [int(S_prev["tok"][a_old[b * bm + i, t - 1], t - 1]) != EOS for i in range(bm)]


def prefixes(S_prev, rows, t):
    """The t tokens (positions 0 .. t - 1) of the hypotheses that sit in `rows` before step t, walked through S_prev's
    ancestor table: what the device's self-attention reads."""
    a_old = S_prev["anc%d" % ((t - 1) & 1)]
    rows = np.asarray(rows, dtype=np.int64)
    pos = np.arange(t)
    return S_prev["tok"][a_old[rows][:, :t].astype(np.int64), pos[None, :]].astype(np.int64)


def audit_selection(S_prev, S_new, t, B, bm, V, logp64=None, bar=None, yardstick=None):
    """(b) for every clip that was not done in S_prev - none is left out.  logp64 [B*bm, V] float64 (rows of clips that are done
    are never read), bar: one log-probability's; without them only the exact checks run.  Returns the worst figures, each as a
    share of its bar: score (|device - float64| / bar), omitted (best omitted - smallest kept) / (2 bar), order (a kept value
    above its predecessor) / (2 bar).
    yardstick(row, token) - asked only for a kept score that is further than `bar` from float64: the error against float64 of
    another, independently tested implementation of the same arithmetic at the same log-probability (row = the parent's row).
    The score then has to be within bar + 2 x that error; `relative` is the worst such score as a share of ITS allowance."""
    worst = dict(score=0.0, omitted=0.0, order=0.0, relative=0.0)
    for b in range(B):
        if S_prev["done"][b]:
            continue
        row0 = b * bm
        parent, token, score = read_choice(S_new, b, bm, t)
        live = live_parents(S_prev, b, bm, t)
        sources = [0] if t == 1 else [i for i in range(bm) if live[i]]
        kept = [i for i in range(bm) if score[i] > EMPTY]
        # ---- exact: the device's own numbers
        _require(all(0 <= parent[i] < bm for i in range(bm)), "parent_range", b, t, parent)
        _require(len(kept) == min(bm, len(sources) * V), "slot_count", b, t, len(kept), len(sources))
        for i in range(bm):
            if i not in kept:  # an empty slot is (parent 0, EOS, -1e20), and no kept slot follows it
                _require(parent[i] == 0 and token[i] == EOS and score[i] == np.float32(-1e20) and all(k < i for k in kept),
                         "empty_slot", b, t, i, parent[i], token[i], score[i])
        for i in kept:
            _require(0 <= token[i] < V, "token_range", b, t, i, token[i])
            if t == 1:
                _require(parent[i] == 0, "first_step_row0", b, i, parent[i])
            _require(live[parent[i]], "ended_parent", b, t, i, parent[i])
        flat = [int(parent[i]) * V + int(token[i]) for i in kept]
        _require(len(set(flat)) == len(flat), "distinct", b, t, flat)
        for a, c in zip(kept, kept[1:]):
            _require(score[a] >= score[c], "score_order", b, t, a, score[a], score[c])
            if score[a] == score[c]:
                _require(flat[kept.index(a)] < flat[kept.index(c)], "tie_order", b, t, a, flat)
        if logp64 is None or not kept:
            continue
        # ---- within the bar: float64
        base = np.zeros(bm) if t == 1 else S_prev["scores"][row0:row0 + bm].astype(np.float64)
        pool = base[sources, None] + logp64[row0 + np.asarray(sources)]  # [sources, V]
        _require(bool(np.isfinite(pool).all()), "reference_finite", b, t)
        src_of = {p: k for k, p in enumerate(sources)}
        val = np.array([pool[src_of[int(parent[i])], token[i]] for i in kept])
        err = np.abs(score[kept].astype(np.float64) - val)
        worst["score"] = max(worst["score"], float(err.max()) / bar)
        for k, i in enumerate(kept):
            if err[k] > bar:
                other = float(yardstick(row0 + int(parent[i]), int(token[i]))) if yardstick is not None else 0.0
                worst["relative"] = max(worst["relative"], float(err[k]) / (bar + 2 * other))
                _require(err[k] <= bar + 2 * other, "score_value", b, t, i, err[k], bar, other)
        rest = pool.copy()
        for i in kept:
            rest[src_of[int(parent[i])], token[i]] = -np.inf
        if np.isfinite(rest).any():
            excess = float(rest.max() - val.min())
            worst["omitted"] = max(worst["omitted"], excess / (2 * bar))
            _require(excess <= 2 * bar, "omitted_better", b, t, excess, 2 * bar,
                     np.unravel_index(int(rest.argmax()), rest.shape))
        if len(val) > 1:
            rise = float((val[1:] - val[:-1]).max())
            worst["order"] = max(worst["order"], rise / (2 * bar))
            _require(rise <= 2 * bar, "kept_order", b, t, rise, 2 * bar)
    return worst


def audit_transition(S_prev, S_new, t, B, bm, need, T, V):
    """(c): S_prev -> step(t, chosen = the device's choice) == S_new, whole tables, bit for bit (columns past t, slots past nfin,
    hypothesis positions past the length and guards included).  Returns the restatement (its branch counters say what ran)."""
    for k in TABLES:
        _require(S_prev[k].shape == S_new[k].shape and S_prev[k].dtype == S_new[k].dtype, "table_shape", k)
    ref = BeamStateRef.from_arrays(S_prev, B, bm, need, T, V)
    chosen = []
    for b in range(B):
        parent, token, score = read_choice(S_new, b, bm, t)
        if S_prev["done"][b]:
            parent = np.zeros(bm, dtype=np.int64)  # (ignored by the step: a frozen clip chooses nothing)
        _require(all(0 <= parent[i] < bm for i in range(bm)), "parent_range", b, t, parent)
        chosen.append((parent, token, score))
    ref.step(t, chosen=chosen)
    for k, want in ref.arrays().items():
        got = S_new[k]
        same = np.array_equal(got.view(np.int32), want.view(np.int32))
        if not same:
            where = np.argwhere(got.view(np.int32) != want.view(np.int32))[:4].tolist()
            _require(False, "transition_" + k, t, where, [got[tuple(w)] for w in where], [want[tuple(w)] for w in where])
    return ref


def audit_step(S_prev, S_new, t, B, bm, need, T, V, logp64=None, bar=None, yardstick=None):
    """(b) + (c) of one step.  Returns (worst figures of (b), the restatement of (c))."""
    worst = audit_selection(S_prev, S_new, t, B, bm, V, logp64, bar, yardstick)
    return worst, audit_transition(S_prev, S_new, t, B, bm, need, T, V)

"""The tests' own restatement of one beam step as the device keeps it (care_beam_advance, csrc/beam.hip) in plain numpy, over
the same physical tables the engine allocates (engine_beam.state / _beam_init), and scripted per-step log-probabilities that
reach every branch of the step.  The yardstick of tests/test_gpu_beam_state.py; pinned to the CPU oracle's per-clip beam
(oracle.care_cpu.HostBeam, misc/Decoding/Beam.py) by tests/test_beam_reference_cpu.py.  No GPU here."""
import numpy as np

PAD, BOS, EOS = 0, 2, 3
BRANCHES = ("need", "maxlen_empty", "maxlen_some", "all_ended", "frozen", "boundary_tie")
MUTANTS = ("tie_desc", "first_all", "ended_stay", "need_plus1")
# class of a clip = clip % 4: the shift of its EOS logit (never ends / ends late / ends early / ends all at once at step 3)
EOS_SHIFT = (-30.0, 1.5, 4.0, 0.0)


class BeamStateRef:
    """B clips x bm beams, `need` hypotheses wanted, T steps at the most, vocabulary V.

    tok [B*bm, stride]: the token a physical row chose at each position (never moved); anc[p] [B*bm, stride]: for the beam
    that sits in a row now, the physical row that holds its token of each position - double-buffered by the step's parity.
    `guard` rows / clips of `sentinel` follow every table, and fscore / flen / fhyp start wholly as sentinels where
    `sentinel` is given (the device test allocates the same), so that equality of whole tables also says what was NOT written.
    `mutant`: one deliberately wrong rule (MUTANTS) - only for showing that the comparison has teeth."""

    def __init__(self, B, bm, need, T, V, sentinel=None, fsentinel=None, guard=0, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.B, self.bm, self.need, self.T, self.V, self.mutant = B, bm, need, T, V, mutant
        self.stride, self.cap = T + 1, need + bm
        N, stride, cap = B * bm, self.stride, self.cap
        s = 0 if sentinel is None else sentinel
        fs = 0.0 if fsentinel is None else fsentinel
        g, gr = guard, guard * bm

        def table(rows, tail, dtype, fill):
            return np.full((rows,) + tail, fill, dtype=dtype)

        self.tok = table(N + gr, (stride,), np.int32, s)
        self.tok[:N] = EOS
        self.tok[:N, 0] = BOS
        self.anc = [table(N + gr, (stride,), np.int32, s) for _ in range(2)]
        for a in self.anc:
            a[:N] = np.arange(N, dtype=np.int32)[:, None]
        self.scores = table(N + gr, (), np.float32, fs)
        self.scores[:N] = 0
        self.done = table(B + g, (), np.int32, s)
        self.done[:B] = 0
        self.nfin = table(B + g, (), np.int32, s)
        self.nfin[:B] = 0
        self.fscore = table(B + g, (cap,), np.float32, fs)
        self.flen = table(B + g, (cap,), np.int32, s)
        self.fhyp = table(B + g, (cap, stride), np.int32, s)
        if sentinel is None:
            assert guard == 0
        self.count = {k: 0 for k in BRANCHES}
        self.clip_count = [{k: 0 for k in BRANCHES} for _ in range(B)]

    @classmethod
    def from_arrays(cls, arrays, B, bm, need, T, V, mutant=None):
        """A restatement that goes on from COPIES of existing tables (those of arrays(): a device state copied to the host), with
        any row stride >= T + 1 and any number of guard rows / clips behind the B * bm rows / B clips."""
        self = cls.__new__(cls)
        assert mutant is None or mutant in MUTANTS
        self.B, self.bm, self.need, self.T, self.V, self.mutant = B, bm, need, T, V, mutant
        a = {k: np.array(v, copy=True) for k, v in arrays.items()}
        self.tok, self.anc, self.scores = a["tok"], [a["anc0"], a["anc1"]], a["scores"]
        self.done, self.nfin, self.fscore, self.flen, self.fhyp = a["done"], a["nfin"], a["fscore"], a["flen"], a["fhyp"]
        self.stride, self.cap = self.tok.shape[1], self.fscore.shape[1]
        assert self.stride >= T + 1 and self.tok.shape[0] >= B * bm and self.done.shape[0] >= B and self.cap >= 1
        assert self.anc[0].shape == self.anc[1].shape == self.tok.shape and self.fhyp.shape == self.fscore.shape + (self.stride,)
        assert self.tok.dtype == np.int32 and self.scores.dtype == np.float32 and self.fscore.dtype == np.float32
        self.count = {k: 0 for k in BRANCHES}
        self.clip_count = [{k: 0 for k in BRANCHES} for _ in range(B)]
        return self

    def arrays(self):
        return dict(tok=self.tok, anc0=self.anc[0], anc1=self.anc[1], scores=self.scores, done=self.done, nfin=self.nfin,
                    fscore=self.fscore, flen=self.flen, fhyp=self.fhyp)

    def _hit(self, b, what):
        self.count[what] += 1
        self.clip_count[b][what] += 1

    def live_rows(self, b, t):
        """Which of clip b's beams can still be extended at step t (their last token is not EOS)."""
        bm, a_old = self.bm, self.anc[(t - 1) & 1]
        if t == 1:
            return [True] * bm
        return [self.tok[a_old[b * bm + i, t - 1], t - 1] != EOS for i in range(bm)]

    def pool_choice(self, b, t, cand_val, cand_idx):
        """What the selection rule keeps for clip b at step t from the candidates [B*bm, bm] of every row, slot by slot:
        (parent[bm], token[bm], score[bm] fp32; an empty slot is (0, EOS, -1e20)), and whether the pruning edge was a tie."""
        bm, V, row0 = self.bm, self.V, b * self.bm
        # candidate pool: (value, flat index i*V + col); the first step looks at row 0 only, ended beams offer nothing
        n_src = bm if (t > 1 or self.mutant == "first_all") else 1
        live = self.live_rows(b, t)
        pool = []
        for i in range(n_src):
            if not live[i] and self.mutant != "ended_stay":
                continue
            for j in range(bm):
                v = np.float32(cand_val[row0 + i, j])
                if t > 1:
                    v = np.float32(v + self.scores[row0 + i])
                col = int(cand_idx[row0 + i, j])
                pool.append((v, i * V + col, i, col))
        # the bm best: value descending, flat index ascending
        sign = -1 if self.mutant == "tie_desc" else 1
        pool.sort(key=lambda c: (-float(c[0]), sign * c[1]))
        sc = [np.float32(-1e20)] * bm
        parent, token = [0] * bm, [EOS] * bm
        for k, (v, _, i, col) in enumerate(pool[:bm]):
            sc[k], parent[k], token[k] = v, i, col
        return (parent, token, sc), len(pool) > bm and pool[bm - 1][0] == pool[bm][0]

    def step(self, t, cand_val=None, cand_idx=None, chosen=None):
        """Step t (1 .. T) on the candidates [B*bm, bm] of every row: value (a log-probability) and column.  Or, with `chosen` -
        one (parent[bm], token[bm], score[bm] fp32) per clip - on a selection made elsewhere: the pool and its sort are
        bypassed (the entry of a frozen clip is ignored), everything after them - ancestors, tokens, scores, finished lists, the
        endings, frozen clips, the branch counters but `boundary_tie` - is the same code."""
        assert 1 <= t <= self.T
        assert (chosen is None) != (cand_val is None)
        bm, V, need, cap = self.bm, self.V, self.need, self.cap
        a_old, a_new, tok = self.anc[(t - 1) & 1], self.anc[t & 1], self.tok
        stop_at = need + 1 if self.mutant == "need_plus1" else need
        for b in range(self.B):
            row0 = b * bm
            if self.done[b]:
                # frozen clip: the tables stay valid, nothing else moves
                for i in range(bm):
                    a_new[row0 + i, :t] = a_old[row0 + i, :t]
                    a_new[row0 + i, t] = row0 + i
                    tok[row0 + i, t] = EOS
                self._hit(b, "frozen")
                continue
            if chosen is None:
                (parent, token, sc), tie = self.pool_choice(b, t, cand_val, cand_idx)
                if tie:
                    self._hit(b, "boundary_tie")
            else:
                parent, token = [int(x) for x in chosen[b][0]], [int(x) for x in chosen[b][1]]
                sc = [np.float32(x) for x in chosen[b][2]]
                assert len(parent) == len(token) == len(sc) == bm and all(0 <= i < bm for i in parent)
            # rewire the ancestors, record tokens and scores
            anew = [a_old[row0 + parent[i], :t].copy() for i in range(bm)]
            for i in range(bm):
                a_new[row0 + i, :t] = anew[i]
                a_new[row0 + i, t] = row0 + i
                tok[row0 + i, t] = token[i]
                self.scores[row0 + i] = sc[i]
            nf = int(self.nfin[b])

            def record(i):
                nonlocal nf
                if nf < cap:  # (a slot past the capacity is counted, not written)
                    self.fscore[b, nf] = sc[i]
                    self.flen[b, nf] = t
                    for p in range(1, t):
                        self.fhyp[b, nf, p - 1] = tok[anew[i][p], p]
                    self.fhyp[b, nf, t - 1] = token[i]
                nf += 1

            is_done = False
            if sc[0] <= np.float32(-1e19):  # no beam left to extend: the clip ends with what it has
                is_done = True
                self._hit(b, "all_ended")
            for i in range(bm):
                if not is_done and token[i] == EOS and sc[i] > np.float32(-1e19):
                    record(i)
                    if nf >= stop_at:
                        is_done = True
                        self._hit(b, "need")
            if not is_done and t >= self.T:
                is_done = True
                if nf == 0:
                    self._hit(b, "maxlen_empty")
                    for i in range(bm):
                        record(i)
                else:
                    self._hit(b, "maxlen_some")
            self.nfin[b] = nf
            if is_done:
                self.done[b] = 1


def script_logits(B, bm, T, V, seed, ties=False):
    """Scripted vocabulary logits of every step, [T, B*bm, V] fp32 (entry t - 1 = step t), whatever the search does with them:
    2 * randn - or, with `ties`, integers in {0, 1, 2} that are the same for the bm rows of a clip, which gives exact ties
    inside rows, across beams and at the selection boundary - with the EOS logit shifted by the clip's class (EOS_SHIFT)."""
    rng = np.random.RandomState(seed)
    if ties:
        x = rng.randint(0, 3, size=(T, B, 1, V)).astype(np.float64).repeat(bm, axis=2)
    else:
        x = 2.0 * rng.randn(T, B, bm, V)
    for b in range(B):
        x[:, b, :, EOS] += EOS_SHIFT[b % 4]
        if b % 4 == 3 and not ties and T >= 3:
            x[2, b, :, EOS] += 40.0  # step 3: every beam ends at once
    return x.reshape(T, B * bm, V).astype(np.float32)


def log_softmax(x):
    x = x.astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def script(B, bm, T, V, seed, ties=False):
    """The scripted per-step log-probabilities [T, B*bm, V] fp32: log_softmax of script_logits."""
    return log_softmax(script_logits(B, bm, T, V, seed, ties))


def candidates(logp, bm):
    """The bm best columns of every row, value descending and equal values by ascending column (care_beam_select's order):
    (values [rows, bm] fp32, columns [rows, bm] int32)."""
    order = np.argsort(-logp, axis=1, kind="stable")[:, :bm]
    return np.take_along_axis(logp, order, axis=1).astype(np.float32), order.astype(np.int32)


# (B, bm, need, T, V) of the scripted searches: bm 1, need > bm, stride 64 (lane 63 in use), bm = 8 (a full 64-lane pool),
# several workgroups of 4 clips with a ragged last one
SHAPES = [(1, 1, 1, 3, 11), (5, 2, 2, 12, 37), (9, 5, 5, 12, 37), (9, 5, 7, 12, 37), (8, 8, 8, 63, 37), (13, 3, 5, 30, 16),
          (6, 8, 10, 63, 9), (130, 5, 5, 12, 37), (131, 3, 5, 12, 16)]
SEED = 1

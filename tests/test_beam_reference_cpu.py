"""tests/beam_reference.py (the yardstick of tests/test_gpu_beam_state.py) against the CPU oracle's per-clip beam, the branches
its scripts reach, and the teeth of the comparison - all on the CPU."""
import numpy as np
import pytest
import torch

from beam_reference import BRANCHES, MUTANTS, SEED, SHAPES, BeamStateRef, candidates, script
from oracle.care_cpu import HostBeam


def run_ref(shape, ties, mutant=None, snapshots=False):
    B, bm, need, T, V = shape
    logp = script(B, bm, T, V, SEED, ties)
    ref = BeamStateRef(B, bm, need, T, V, mutant=mutant)
    snaps = []
    for t in range(1, T + 1):
        ref.step(t, *candidates(logp[t - 1], bm))
        if snapshots:
            snaps.append({k: v.copy() for k, v in ref.arrays().items()})
    return ref, snaps


_runs = {}


def cached_run(shape, ties):
    """The unmutated search of a script, computed once (with the state after every step)."""
    if (shape, ties) not in _runs:
        _runs[(shape, ties)] = run_ref(shape, ties, snapshots=True)
    return _runs[(shape, ties)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_the_host_beam_on_tie_free_scripts(shape):
    B, bm, need, T, V = shape
    logp = script(B, bm, T, V, SEED)
    ref = BeamStateRef(B, bm, need, T, V)
    host = [HostBeam(bm, T + 1, need) for _ in range(B)]
    for t in range(1, T + 1):
        rows = torch.from_numpy(logp[t - 1]).view(B, bm, V)
        # the one place the device leaves the reference (csrc/beam.hip, "topk > beam_size"): a clip none of whose beams is
        # live ends with what it has, where the reference goes on from -1e20 rows in an order torch leaves unspecified
        go = [not ref.done[b] and any(ref.live_rows(b, t)) for b in range(B)]
        ref.step(t, *candidates(logp[t - 1], bm))
        for b in range(B):
            if go[b]:
                assert not host[b].done
                host[b].advance(rows[b].clone())
                assert bool(ref.done[b]) == host[b].done, (b, t)
            assert int(ref.nfin[b]) == len(host[b].finished), (b, t)
    for b in range(B):
        h = host[b]
        # no clip is left out: every decision of every clip's search was free of ties
        assert min(h.gap_select, h.gap_order) > 0, (b, h.gap_select, h.gap_order)
        assert ref.done[b] == 1 and int(ref.nfin[b]) == len(h.finished) <= ref.cap
        for k, (score, t, beam, _) in enumerate(h.finished):
            assert float(ref.fscore[b, k]) == score, (b, k)  # fp32, bit for bit
            assert int(ref.flen[b, k]) == t
            assert ref.fhyp[b, k, :t].tolist() == h.hypothesis(t, beam), (b, k)


def test_scripts_reach_every_branch():
    total = {k: 0 for k in BRANCHES}
    for shape in SHAPES:
        for ties in (False, True):
            ref, _ = cached_run(shape, ties)
            assert ref.done[: shape[0]].all()
            for k in BRANCHES:
                total[k] += ref.count[k]
            if ties and shape[0] >= 5:
                assert ref.count["boundary_tie"] > 0, shape
            if not ties:
                assert ref.count["boundary_tie"] == 0, shape
            if not ties and shape[0] >= 5:
                for k in ("need", "maxlen_empty", "frozen"):
                    assert ref.count[k] > 0, (shape, k)
            if shape[2] > shape[1] and shape[0] >= 9:  # need > bm: clips that run out of live beams before `need` ended
                assert ref.count["all_ended"] > 0, shape
    assert all(total[k] > 0 for k in BRANCHES), total


@pytest.mark.parametrize("ties", [False, True])
def test_a_step_on_a_given_choice_equals_the_step_on_the_pool(ties):
    """step(chosen = what the pool rule picks), on a restatement built from copies of the tables (from_arrays), leaves the bytes
    of step() - after every step of every scripted search, boundary_tie apart the same branch counts."""
    for shape in SHAPES[:7]:
        B, bm, need, T, V = shape
        logp = script(B, bm, T, V, SEED, ties)
        ref, snaps = cached_run(shape, ties)
        other = BeamStateRef(B, bm, need, T, V)
        total = {k: 0 for k in BRANCHES}
        for t in range(1, T + 1):
            cv, ci = candidates(logp[t - 1], bm)
            other = BeamStateRef.from_arrays(other.arrays(), B, bm, need, T, V)
            other.step(t, chosen=[other.pool_choice(b, t, cv, ci)[0] for b in range(B)])
            for k, want in snaps[t - 1].items():
                assert np.array_equal(other.arrays()[k].view(np.int32), want.view(np.int32)), (shape, t, k)
            for k in BRANCHES:
                total[k] += other.count[k]
        assert total["boundary_tie"] == 0
        assert all(total[k] == ref.count[k] for k in BRANCHES if k != "boundary_tie"), (shape, total, ref.count)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_rule_changes_what_the_device_test_compares(mutant):
    """tie-break by descending flat index / first step over all rows / ended beams left in the pool / stop at need + 1: each
    differs from the restatement in an array tests/test_gpu_beam_state.py compares, on a script it runs."""
    caught = []
    for shape in SHAPES[:7]:
        for ties in (False, True):
            _, good = cached_run(shape, ties)
            _, bad = run_ref(shape, ties, mutant=mutant, snapshots=True)
            if any(not np.array_equal(g[k], w[k]) for g, w in zip(good, bad) for k in g):
                caught.append((shape, ties))
    assert caught, mutant

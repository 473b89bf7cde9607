"""care_amd/forms.py on the CPU: the plan of a pass (`PassPlan`) against what the engine's predicates answered before the
plan existed, over a grid that has a point on each side of every hand-over of DESIGN.md 5; the plan as a graph key."""
import dataclasses
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forms_grid.json")
DTYPES = ("bf16", "fp16", "fp32", "fp16x3")
CLIPS = (1, 3, 32, 128, 129, 256, 257, 512, 1024, 1279, 1280, 2048, 2049, 4096, 8191, 8192, 10239, 10240, 16383, 16384, 32768)
BEAMS = (1, 5, 8)
# one bit per answer, in this order (lanes_for's count above them)
BITS = ("resident", "chain", "small_forms", "latent_for", "ln_fusable", "vocab_as", "beam_fused_for", "beam_groups_for",
        "lean_ok", "tf_fast_ok", "q_tile", "mid_tile")


def _engines():
    """(key, engine) over every config x compute mode x resident_max_rows (default, 0) x latent (True, False)."""
    from care_amd.configs import CONFIG_NAMES, make_opt
    from care_amd.engine import HipEngine

    for cfg in CONFIG_NAMES:
        for dtype in DTYPES:
            for rmax in (None, 0):
                for latent in (True, False):
                    eng = HipEngine(make_opt(cfg), dtype)
                    if rmax is not None:
                        eng.resident_max_rows = rmax
                    eng.latent = latent
                    yield "{}|{}|{}|{}".format(cfg, dtype, "default" if rmax is None else rmax, int(latent)), eng


def _record(eng, clips, bm):
    """What the engine's public predicates answer for a pass over `clips` clips x `bm` beams (asked before any pass)."""
    rows = clips * bm
    return dict(resident=eng.resident_ok(clips) if bm == 1 else eng.resident_beam_ok(clips, bm, bm),
                chain=eng.chain_beam_ok(clips, bm, bm), small_forms=eng.small_forms(clips), latent_for=eng.latent_for(rows),
                ln_fusable=eng.ln_fusable(rows), vocab_as=eng._vocab_as(rows), beam_fused_for=eng.beam_fused_for(rows),
                beam_groups_for=eng.beam_groups_for(rows, bm), lean_ok=eng.lean_ok, tf_fast_ok=eng.tf_fast_ok(29, False),
                lanes=eng.lanes_for(clips))


def _pack(rec):
    return sum(int(bool(rec[name])) << i for i, name in enumerate(BITS) if name in rec) | int(rec["lanes"]) << len(BITS)


def _grid():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert tuple(g["clips"]) == CLIPS and tuple(g["beams"]) == BEAMS and tuple(g["bits"]) == BITS
    return g


def test_predicates_and_plan_reproduce_the_recorded_grid():
    """tests/golden/forms_grid.json is what `_record` answered on the commit before care_amd/forms.py existed (with two
    columns for the tests that stood inline in the step code then: `q_tile` - d_model 512 and rows >= 8192 - and `mid_tile` -
    1280 <= rows < 16384).  The engine's views answer the same today, and the plan of the pass over the same shape holds the
    same decisions - exactly: a threshold that moves by one row fails here."""
    g = _grid()
    seen = 0
    for key, eng in _engines():
        want = iter(g["rows"][g["index"][key]])
        for clips in CLIPS:
            for bm in BEAMS:
                w = next(want)
                w = dict({name: bool(w >> i & 1) for i, name in enumerate(BITS)}, lanes=w >> len(BITS))
                rows, at = clips * bm, (key, clips, bm)
                assert eng.plan is None           # (before any pass: latent_for has no small beam pass to remember)
                got = _record(eng, clips, bm)
                assert got == {k: w[k] for k in got}, at
                p = eng.plan_for(clips, bm if bm > 1 else None, bm, lean=True)
                assert p.decode == ("resident" if w["resident"] else "chain" if w["chain"] else "multi"), at
                assert (p.clips, p.rows, p.need, p.lanes) == (clips, rows, bm, w["lanes"]), at
                assert p.small_beam == (bm > 1 and w["small_forms"]), at
                # the embedder's small forms: every beam search over a small batch and every resident decode of one
                assert p.small == ((bm > 1 and w["resident"]) or (w["small_forms"] and (bm > 1 or w["resident"]))), at
                assert p.latent == (w["latent_for"] and not p.small_beam), at
                assert (p.fuse_ln, p.vocab_as, p.q_tile, p.mid_tile) == (w["ln_fusable"], w["vocab_as"], w["q_tile"], w["mid_tile"]), at
                sel = "" if bm == 1 or p.decode != "multi" else "fused" if w["beam_fused_for"] else "groups" if w["beam_groups_for"] else "logits"
                assert p.beam_select == sel and p.sparse_second_pass == (sel == "fused" and eng.d == 512), at
                assert p.lean == w["lean_ok"] and p.early_exit is True, at
                seen += 1
    assert seen == len(g["index"]) * len(CLIPS) * len(BEAMS) == 10080


def test_latent_for_remembers_a_small_beam_pass():
    """bench.py asks latent_for AFTER its passes: a beam search over a small batch ran on projected K/V, and says so."""
    from care_amd.configs import make_opt
    from care_amd.engine import HipEngine

    eng = HipEngine(make_opt("msrvtt_care_beam5"), "bf16")
    eng.resident_beam_max_rows = 0
    assert eng.latent_for(640)
    eng.plan = eng.plan_for(128, 5, 5)
    assert eng.plan.small_beam and not eng.plan.latent and not eng.latent_for(640)
    eng.plan = eng.plan_for(128)   # a greedy pass over the same clips: the resident launch, nothing to remember
    assert eng.plan.decode == "resident" and eng.latent_for(640)
    eng.plan = eng.plan_for(257, 5, 5)
    assert eng.plan.latent and eng.latent_for(640)


def test_a_step_helper_outside_a_pass_chooses_by_its_rows():
    from care_amd.configs import make_opt
    from care_amd.engine import HipEngine

    eng = HipEngine(make_opt("msrvtt_base_ami"), "bf16")
    assert eng.plan is None and not eng._vocab_as(2048) and eng._vocab_as(2049)
    eng.plan = eng.plan_for(4096)      # in a pass: the initial row count, whatever compaction left
    assert eng._vocab_as(128) and eng.plan.vocab_as
    # teacher forcing: the rows are sequences x positions, the forms the multi-launch ones
    p = eng.plan_for(512, rows=512 * 29)
    assert p.decode == "multi" and p.rows == 14848 and p.fuse_ln and p.vocab_as and p.bm is None and p.beam_select == ""
    # a lane of a two-lane pass plans its own rows; the pass's plan carries the lane count and no early exit
    eng.lanes = 2
    p = eng.plan_for(20479, n_lanes=eng.lanes_for(20479))
    assert p.lanes == 2 and p.decode == "multi" and not p.early_exit and eng.lanes_for(1) == 1
    assert not eng.plan_for(10239, rows=10239).fuse_ln and eng.plan_for(10240, rows=10240).fuse_ln


def test_a_refused_resident_launch_moves_the_plan():
    from care_amd.configs import make_opt
    from care_amd.engine import HipEngine

    eng = HipEngine(make_opt("msrvtt_care_beam5"), "bf16")
    assert eng.plan_for(128).decode == "resident" and eng.plan_for(64, 5, 5).decode == "resident"
    eng._resident_refused["greedy"] = 100
    assert eng.plan_for(128).decode == "multi" and eng.plan_for(99).decode == "resident" and not eng.resident_ok(100)
    assert eng.plan_for(64, 5, 5).decode == "resident"
    eng._resident_refused["beam"] = 320
    p = eng.plan_for(64, 5, 5)
    assert p.decode == "multi" and p.small and p.small_beam and p.beam_select == "groups" and not eng.resident_beam_ok(64, 5, 5)
    eng.chain_beam_max_rows = 4096
    assert eng.plan_for(64, 5, 5).decode == "chain" and eng.plan_for(63, 5, 5).decode == "resident"
    eng._cus = 32   # a partition with 32 compute units: a workgroup per 16-row tile up to 512 rows
    eng.resident_max_rows = 1024
    eng._resident_refused.clear()
    assert eng.plan_for(32 * 16).decode == "resident" and eng.plan_for(32 * 16 + 1).decode == "multi"
    eng._cus = 16
    assert eng.resident_beam_ok(51, 5, 5) and not eng.resident_beam_ok(52, 5, 5)   # (255 rows = 16 tiles; 260 rows = 17)


def test_plan_is_a_hashable_value_and_every_field_tells():
    from care_amd import forms
    from care_amd.configs import make_opt
    from care_amd.engine import HipEngine

    eng = HipEngine(make_opt("msrvtt_care_beam5"), "bf16")
    p = eng.plan_for(512, 5, 5, lean=True)
    assert p == eng.plan_for(512, 5, 5, lean=True) and hash(p) == hash(eng.plan_for(512, 5, 5, lean=True)) and {p: 1}[p] == 1
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.rows = 1
    other = dict(decode="resident", bm=None, beam_select="fused")
    for f in dataclasses.fields(p):
        v = getattr(p, f.name)
        q = dataclasses.replace(p, **{f.name: other[f.name] if f.name in other else (not v) if isinstance(v, bool) else v + 1})
        assert q != p and hash(q) != hash(p), f.name
    needed = {"decode", "rows", "small", "latent", "fuse_ln", "vocab_as", "q_tile", "mid_tile", "beam_select", "sparse_second_pass",
              "lean", "early_exit", "lanes"}
    assert needed <= {f.name for f in dataclasses.fields(p)}
    # limits are plain engine attributes, read when the plan is built
    eng.BEAM_FUSED_MIN_ROWS = 1
    assert eng.plan_for(512, 5, 5).beam_select == "fused" and p.beam_select == "groups"
    eng.latent = False
    assert not eng.plan_for(512, 5, 5).latent and p.latent


def test_graph_keys_carry_the_plan():
    """Every captured graph is keyed (kind, plan, what is the site's own, feature addresses, feature shapes): two passes
    over the same buffers whose forms differ in ANY decision never share a graph."""
    import torch

    from care_amd import forms
    from care_amd.configs import make_opt
    from care_amd.engine import HipEngine

    eng = HipEngine(make_opt("msrvtt_base_ami"), "bf16")
    feats = [torch.zeros(4, 3), torch.zeros(4, 5)]
    p = eng.plan_for(4096, lean=True)
    key = forms.graph_key("gseg0", p, feats, 8)
    assert key == ("gseg0", p, 8, tuple(f.data_ptr() for f in feats), ((4, 3), (4, 5))) and hash(key) is not None
    for name in ("greedy", "gres", "gseg0", "beam", "bres", "bseg0", "bchain", "ens"):
        k = forms.graph_key(name, p, feats)
        assert k[0] == name and k[1] is p and eng.GRAPH_CAPS.get(k[0], 8) >= 8
    eng.latent = False
    assert forms.graph_key("gseg0", eng.plan_for(4096, lean=True), feats, 8) != key
    eng.latent = True
    assert forms.graph_key("gseg0", eng.plan_for(4096, lean=True), feats, 8) == key
    assert forms.graph_key("gseg0", eng.plan_for(4096, lean=False), feats, 8) != key
    # the engine files build no key by hand (segments of engine-owned buffers: kind, plan, bounds, rows, parity)
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "care_amd")
    for fn in sorted(os.listdir(src)):
        if fn.startswith("engine") and fn.endswith(".py"):
            for ln in open(os.path.join(src, fn)):
                if "_replay(" in ln or "replayable(" in ln:
                    if "def _replay" in ln or "replayable = lambda" in ln or "key, run" in ln:
                        continue
                    assert "forms.graph_key(" in ln or '("gseg", plan,' in ln or '("bseg", plan,' in ln, (fn, ln)

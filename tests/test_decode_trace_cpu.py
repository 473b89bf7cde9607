"""CPU: what the multi-launch decodes ENQUEUE, launch by launch, against a recording of the commit before the step loops,
the segment driver and the clip mover of care_amd/engine_decode.py / engine_beam.py / engine_resident.py were each written
once.

A `HipEngine` is built without a device: its workspaces are CPU tensors, its weights zero tensors, `engine.call` a recorder
that names every address it is handed (`ws:<lane>:<workspace>[shape,dtype]+<byte offset>`, `w:<key>`, `feat:<i>`), `encode`
one trace entry that hands back the `enc_out_*` workspaces, `_host_count` a scripted list of survivor counts.  No kernel
runs; the library's integer helpers (`care_argmax_parts_*`, `care_beam_sparse_applies`, the scratch sizes) are host code and
do.  Per scenario tests/golden/decode_launch_trace.json holds the SHA-256 of the canonical trace, the launches per function,
the replay keys in order, `last_decode` and the SHA-256 of the final bytes of every int32 / uint8 workspace (what torch's
own fill_ / zero_ / copy_ / add left in buffers that start as a sentinel: the initial state and the -1 padding).

The fixture is recorded from ANOTHER tree's care_amd (the parent commit's), by this module as a script:

    python tests/test_decode_trace_cpu.py --record --tree PATH [--dump DIR]

`--dump DIR` also writes the full trace of every scenario, one JSON line per entry: what to diff when a hash moves."""
import bisect
import collections
import ctypes
import dataclasses
import hashlib
import json
import os
import sys
import weakref

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launch_trace.json")
SENTINEL32, SENTINEL8 = 0x5A5A5A5A, 0x5A   # what a workspace holds before torch writes to it

# name -> (config, overrides, dtype, clips, beam, engine attributes, survivor script, must show)
#   must show: launches = launches in all; kinds = replay keys per kind; last = entries of last_decode; select = the plan's
#   beam_select; fns = functions launched at least once; moved = workspaces that compaction gathers INTO
# A scenario that stops compacting has stopped testing: these are conditions on the RECORDING, asserted before it is compared.
SCENARIOS = collections.OrderedDict([
    ("greedy_bf16_4096", ("msrvtt_base_ami", {}, "bf16", 4096, None, {}, [3000, 2000, 900, 100, 100, 0],
                          dict(launches=407, kinds={"gseg0": 1, "gseg": 5}, moved=["g1_mem", "g0_mem"],
                               last=dict(clips=4096, steps=24, row_steps=49152, compactions=3)))),
    ("greedy_bf16_2304_fixed", ("msrvtt_base_ami", {}, "bf16", 2304, None, dict(early_exit=False), [],
                                dict(launches=437, kinds={"greedy": 1}, last={}))),
    ("greedy_care_fp32_2048", ("msrvtt_care", {}, "fp32", 2048, None, dict(resident_max_rows=0), [1500, 800, 0],
                               dict(kinds={"gseg0": 1, "gseg": 2}, moved=["g1_sem", "g1_ckv0"],
                                    last=dict(clips=2048, steps=12, compactions=1)))),
    ("beam5_groups_512", ("msrvtt_care_beam5", {}, "bf16", 512, 5, {}, [380, 200, 64, 0],
                          dict(select="groups", kinds={"bseg0": 1, "bseg": 3}, fns=["care_gemm_tile_beam", "care_beam_pick_groups"],
                               last=dict(clips=512, steps=16, row_steps=33280, compactions=1)))),
    ("beam5_fused_512", ("msrvtt_care_beam5", {}, "bf16", 512, 5, dict(BEAM_FUSED_MIN_ROWS=2048), [380, 200, 64, 0],
                         dict(select="fused", sparse=True, fns=["care_gemm_argmax_bf16_min", "care_gemm_collect_bf16", "care_beam_pick"],
                              last=dict(clips=512, steps=16, row_steps=33280, compactions=1)))),
    ("beam5_cabase_448", ("msrvtt_cabase", {}, "bf16", 448, 5, {}, [300, 100, 0],
                          dict(moved=["b1_akv0"], last=dict(clips=448, steps=12, compactions=1)))),
    ("beam5_fp32_448", ("msrvtt_base_ami", {}, "fp32", 448, 5, {}, [300, 100, 0],
                        dict(select="logits", moved=["b1_ckv0"], fns=["care_beam_select"],
                             last=dict(clips=448, steps=12, compactions=1)))),
    ("beam5_256_fixed", ("msrvtt_care_beam5", {}, "bf16", 256, 5, dict(early_exit=False), [],
                         dict(launches=437, kinds={"beam": 1}, last={}))),
    ("beam5_chain_96", ("msrvtt_care_beam5", {}, "bf16", 96, 5, dict(resident_beam_max_rows=0, chain_beam_max_rows=640), [50, 10, 0],
                        dict(kinds={"bchain": 3}, fns=["care_decode_chain_beam"],
                             last=dict(clips=96, steps=24, compactions=0, chain=True)))),
    ("beam5_chain_96_fixed", ("msrvtt_care_beam5", {}, "bf16", 96, 5,
                              dict(resident_beam_max_rows=0, chain_beam_max_rows=640, early_exit=False), [],
                              dict(kinds={"bchain": 1}, last=dict(clips=96, steps=29, compactions=0, chain=True)))),
    # beyond the ten of the issue: the other 16-bit type with a two-layer decoder, a pre-LN decoder, the fused dense + LayerNorm
    # of a large batch, the ensemble branch of `beam`, and the teacher-forced decoder on both forms of dense -> LayerNorm
    ("greedy_fp16_2layers_2048", ("msrvtt_care", dict(num_hidden_layers_decoder=2), "fp16", 2048, None, dict(resident_max_rows=0),
                                  [1000, 0], dict(kinds={"gseg0": 1, "gseg": 1}, moved=["g1_sem", "g1_mem"],
                                                  last=dict(clips=2048, steps=8, compactions=1)))),
    ("greedy_preln_fp32_2048", ("msrvtt_base_ami", dict(transformer_pre_ln=True), "fp32", 2048, None, {}, [1024, 0],
                                dict(moved=["g1_ckv0"], last=dict(clips=2048, steps=8, compactions=1)))),
    ("greedy_bf16_12288_fused_ln", ("msrvtt_base_ami", {}, "bf16", 12288, None, {}, [6000, 0],
                                    dict(fns=["care_gemm_ln"], last=dict(clips=12288, steps=8, compactions=1)))),
    ("beam5_preln_bf16_448", ("msrvtt_care_beam5", dict(transformer_pre_ln=True), "bf16", 448, 5, {}, [300, 0],
                              dict(last=dict(clips=448, steps=8, compactions=1)))),
    # ... and at a row count where the library's sparse second pass applies (the plan of the 512-clip scenario asks for it, the
    # library's statistics kernel takes it from 8192 rows)
    ("beam5_fused_sparse_2048", ("msrvtt_care_beam5", {}, "bf16", 2048, 5, {}, [1500, 0],
                                 dict(select="fused", sparse=True, fns=["care_gemm_argmax_bf16_tiles", "care_beam_sparse_collect"],
                                      last=dict(clips=2048, steps=8, compactions=1)))),
    # clips that never end: the segmented passes read the counter once more after step T, the chain does not
    ("greedy_bf16_2048_to_the_end", ("msrvtt_base_ami", {}, "bf16", 2048, None, {}, [2048] * 8,
                                     dict(kinds={"gseg0": 1, "gseg": 7}, last=dict(clips=2048, steps=29, row_steps=2048 * 29, compactions=0)))),
    ("beam5_640_to_the_end", ("msrvtt_care_beam5", {}, "bf16", 640, 5, {}, [640, 600, 500, 481, 481, 481, 481, 481],
                              dict(kinds={"bseg0": 1, "bseg": 7}, last=dict(clips=640, steps=29, row_steps=3200 * 29, compactions=0)))),
    ("beam5_chain_96_to_the_end", ("msrvtt_care_beam5", {}, "bf16", 96, 5, dict(resident_beam_max_rows=0, chain_beam_max_rows=640),
                                   [50, 50, 50], dict(kinds={"bchain": 4}, last=dict(clips=96, steps=29, compactions=0, chain=True)))),
    ("ensemble_beam3_64", ("msrvtt_care", {}, "bf16", 64, 3, dict(others=[("msrvtt_base_ami", {}), ("msrvtt_cabase", {})]), [],
                           dict(kinds={"ens": 1}, fns=["care_ensemble_select", "e1/care_embed_ln", "e2/care_embed_ln"], last={}))),
    ("teacher_forced_bf16_512x29", ("msrvtt_care", {}, "bf16", 512, None, dict(teacher_forced=29), [],
                                    dict(fns=["care_attention_seq", "care_gemm_ln"], last={}))),
    ("teacher_forced_bf16_64x29", ("msrvtt_cabase", {}, "bf16", 64, None, dict(teacher_forced=29), [],
                                   dict(fns=["care_attention_seq", "care_add_ln"], last={}))),
])


class _Weights(dict):
    """engine.w without a checkpoint: a missing key is a zero tensor of the shape the packer gives it (by suffix); the
    `#packed` / `#split` / `#split3` re-orderings are absent, as are the parameters a model does not have."""

    def __init__(self, eng):
        super().__init__()
        self.eng = weakref.proxy(eng)

    def __missing__(self, key):
        import torch

        e = self.eng
        d, ff = e.d, e.ff
        if "#" in key:
            raise KeyError(key)
        if key in ("emb_g", "emb_be") and e.pre_ln:
            t = None
        elif key.endswith("_hb"):
            t = torch.zeros(e.H, e.Lk) if e.opt.get("add_hybrid_attention_bias") else None
        else:
            shape = ((3 * d, d) if key.endswith("_qkv_w") else (d, d) if key.endswith(("_q_w", "_o_w", "_v_w")) else
                     (2 * d, d) if key.endswith("_kv_w") else (ff, d) if key.endswith("_w1") else (d, ff) if key.endswith("_w2") else
                     (e.V, d) if key == "vocab" else None)
            if shape is not None:
                t = torch.zeros(shape, dtype=e.wt)
            elif key.endswith("_wkt"):
                t = torch.zeros(e.H, d, 64, dtype=e.h16)
            else:
                t = torch.zeros(8)
        self[key] = t
        return t


class Recorder:
    """The trace of one scenario and the names of the addresses in it."""

    def __init__(self):
        self.engines, self.inputs, self.trace, self.keys = [], [], [], []
        self.unnamed, self.script, self.consumed = [], [], 0
        self._sig, self._starts, self._iv = None, [], []

    # ---------------------------------------------------------------- engines
    def engine(self, care_amd, config, overrides, dtype, attrs):
        import torch

        eng = care_amd.engine.HipEngine(care_amd.configs.make_opt(config, **overrides), dtype)
        eng.device, eng._cus, eng.ws_budget_bytes = torch.device("cpu"), 256, 1 << 60
        eng.w = _Weights(eng)
        for k, v in attrs.items():
            setattr(eng, k, v)
        i = len(self.engines)
        self.engines.append(eng)
        pre = "e%d/" % i if i else ""
        ws_get = eng._ws_get

        def sentinel_ws_get(name, shape, dtype):
            new = (eng._lane, name, tuple(shape), dtype) not in eng._ws
            t = ws_get(name, shape, dtype)
            if new and dtype in (torch.int32, torch.uint8):
                t.fill_(SENTINEL32 if dtype == torch.int32 else SENTINEL8)
            return t

        def call(fn, *args, tag=None):
            self.trace.append([pre + fn, [self.canon(a) for a in args], tag])

        def encode(feats, lean=False, static=False, small=False):
            self.trace.append([pre + "encode", [bool(lean), bool(static), bool(small)], None])
            B, shape = feats[0].shape[0], (feats[0].shape[0], eng.Lk, eng.d)
            memb = eng.ws("enc_out_memb", shape, eng.h16) if eng.bf_act else None
            if lean and eng.lean_ok:
                return {"encoder_hidden_states": memb}
            mem = eng.ws("enc_out_mem", shape)
            out = {"encoder_hidden_states": mem}
            if eng.sem:
                out["semantic_hidden_states"] = eng.ws("enc_out_sem_hidden", (B, eng.d))
            if eng.attr_att:
                out["semantic_embs"] = eng.ws("enc_out_sem_embs", (B, eng.topk, eng.d))
            eng._mem_mirror = (weakref.ref(mem), memb)
            return out

        def host_count(cnt):
            assert self.consumed < len(self.script), "the pass asks for more survivor counts than the script holds"
            self.trace.append([pre + "host_count", [self.canon(cnt.data_ptr())], None])
            self.consumed += 1
            return self.script[self.consumed - 1]

        def replay(key, fn, use_graph=True):
            key = self.canon_key(key)
            self.keys.append(key)
            self.trace.append([pre + "replay", [key, bool(use_graph)], None])
            return fn()

        eng._ws_get, eng.call, eng.encode, eng._host_count, eng._replay = sentinel_ws_get, call, encode, host_count, replay
        eng._prep_feats = lambda feats: feats
        return eng

    # ---------------------------------------------------------------- names
    def _index(self):
        sig = tuple((len(e._ws), len(e.w)) for e in self.engines) + (len(self.inputs),)
        if sig != self._sig:
            iv = []
            for i, e in enumerate(self.engines):
                pre = "e%d/" % i if i else ""
                for (lane, name, shape, dt), t in e._ws.items():
                    if t.numel():
                        label = "{}ws:{}:{}[{},{}]".format(pre, lane, name, "x".join(map(str, shape)), str(dt).replace("torch.", ""))
                        iv.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), label))
                for k, t in e.w.items():
                    if t is not None and t.numel():
                        iv.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), pre + "w:" + k))
            for label, t in self.inputs:
                iv.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), label))
            iv.sort()
            for a, b in zip(iv, iv[1:]):
                assert a[1] <= b[0], ("two named buffers overlap", a[2], b[2])
            self._sig, self._iv, self._starts = sig, iv, [x[0] for x in iv]
        return self._iv, self._starts

    def lookup(self, a):
        iv, starts = self._index()
        k = bisect.bisect_right(starts, a) - 1
        if k >= 0 and iv[k][0] <= a < iv[k][1]:
            return "{}+{}".format(iv[k][2], a - iv[k][0])
        return None

    def canon(self, a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, ctypes.Array):   # (care_ensemble_select: the members' logits)
            return [self.canon(x) for x in a]
        if isinstance(a, int):
            for e in self.engines:
                layers = getattr(e, "_res_layers", None)
                if layers is not None and a == ctypes.addressof(layers):
                    return {"layers": [self.canon_struct(L) for L in layers]}
            name = self.lookup(a)
            if name is None and a >= 1 << 32:
                self.unnamed.append(a)
                return "unnamed:{}".format(len(self.unnamed))
            return a if name is None else name
        raise TypeError("argument {!r} of a launch".format(a))

    def canon_struct(self, s):
        out = {}
        for name, _ in s._fields_:
            v = getattr(s, name)
            out[name] = ([self.canon_struct(x) for x in v] if isinstance(v, ctypes.Array) else self.canon(v))
        return out

    def canon_key(self, key):
        def one(x):
            if dataclasses.is_dataclass(x):
                return dataclasses.asdict(x)
            if isinstance(x, tuple):
                return [one(y) for y in x]
            if isinstance(x, int) and not isinstance(x, bool):
                for i, e in enumerate(self.engines):
                    if x == id(e):
                        return "engine:%d" % i
                return self.canon(x)
            return x
        feats = tuple(t.data_ptr() for label, t in self.inputs if label.startswith("feat:"))
        return [one(x) for x in key if not (isinstance(x, tuple) and x and x == feats)]

    # ---------------------------------------------------------------- the result
    def result(self, plan):
        lines = [json.dumps(e, sort_keys=True, separators=(",", ":")) for e in self.trace]
        # (the stubbed encode counts as one launch)
        launches = collections.Counter(e[0] for e in self.trace if not e[0].split("/")[-1] in ("host_count", "replay"))
        ws = {}
        import torch
        for i, e in enumerate(self.engines):
            for (lane, name, shape, dt), t in sorted(e._ws.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], str(kv[0][3]))):
                if dt in (torch.int32, torch.uint8):
                    label = "{}{}:{}[{},{}]".format("e%d/" % i if i else "", lane, name, "x".join(map(str, shape)), str(dt).replace("torch.", ""))
                    ws[label] = hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()
        last = {k: (int(v) if not isinstance(v, bool) and v is not None else v) for k, v in self.engines[0].last_decode.items()}
        return dict(trace_sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest(), entries=len(lines),
                    launches=dict(sorted(launches.items())), keys=self.keys, last_decode=last, host_counts=self.consumed,
                    beam_select=plan.beam_select if plan is not None else "",
                    sparse_second_pass=bool(plan is not None and plan.sparse_second_pass), workspaces=ws), lines


def run_scenario(name, care_amd=None):
    """(what the fixture holds for scenario `name`, the full trace as JSON lines, the recorder)."""
    import torch

    if care_amd is None:
        import care_amd
    import care_amd.configs
    import care_amd.engine
    config, overrides, dtype, clips, bm, attrs, script, _ = SCENARIOS[name]
    attrs = dict(attrs)
    others, tf = attrs.pop("others", []), attrs.pop("teacher_forced", None)
    rec = Recorder()
    rec.script = list(script)
    eng = rec.engine(care_amd, config, overrides, dtype, attrs)
    feats_list = []
    for e in [eng] + [rec.engine(care_amd, c, o, dtype, {}) for c, o in others]:
        feats = [torch.zeros(clips, 1) for _ in e.modality]
        for f in feats:
            rec.inputs.append(("feat:%d" % len(rec.inputs), f))
        feats_list.append(feats)
    if tf is not None:   # the teacher-forced decoder on the workspaces of a static encode (decode_full, scoring's call)
        ids = torch.zeros(clips, tf, dtype=torch.int32)
        rec.inputs.append(("in:input_ids", ids))
        eng._begin_pass(eng.plan_for(clips, rows=clips * tf))
        enc = eng.encode(feats_list[0], False, static=True)
        out = eng.decode_full(ids, enc["encoder_hidden_states"], enc.get("semantic_hidden_states"), want_logits="none",
                              sem_embs=enc.get("semantic_embs"), hidden_fp32=False, plan=eng.plan)
        hidden = out["hidden_states"]   # (a fresh tensor where the fp32 hidden state is written: the one address without a name)
        assert len(rec.unnamed) == (0 if hidden is None else 1) and (hidden is None or rec.unnamed[0] == hidden.data_ptr())
        rec.unnamed = []
    elif others:
        eng.translate_beam_ensemble(rec.engines[1:], feats_list, bm, bm)
    elif bm is None:
        eng.translate_greedy(feats_list[0])
    else:
        eng.translate_beam(feats_list[0], bm, bm)
    assert not rec.unnamed, "{} addresses without a name".format(len(rec.unnamed))
    assert eng._ws_cap is None
    res, lines = rec.result(eng.plan)
    return res, lines, rec


def check_conditions(name, res, lines):
    """What the scenario must show (SCENARIOS), on a recording."""
    show = SCENARIOS[name][-1]
    assert res["host_counts"] == len(SCENARIOS[name][6]), "the survivor script was not consumed to its end"
    if "launches" in show:
        assert sum(res["launches"].values()) == show["launches"]
    kinds = collections.Counter(k[0] for k in res["keys"])
    for kind, n in show.get("kinds", {}).items():
        assert kinds[kind] == n, (kinds, kind)
    if "select" in show:
        assert res["beam_select"] == show["select"]
    if "sparse" in show:
        assert res["sparse_second_pass"] == show["sparse"]
    for fn in show.get("fns", []):
        assert res["launches"].get(fn, 0) > 0, fn
    last = show["last"]
    assert (res["last_decode"] == {}) if last == {} else all(res["last_decode"].get(k) == v for k, v in last.items()), res["last_decode"]
    gathers = [json.loads(ln) for ln in lines if ln.startswith('["care_gather_rows"')]
    for wsname in show.get("moved", []):
        assert any(":{}[".format(wsname) in g[1][2] for g in gathers), "compaction moved nothing into " + wsname


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_a_pass_enqueues_what_the_recording_holds(name):
    """The pass of scenario `name` on THIS tree's engine against tests/golden/decode_launch_trace.json (recorded from the
    parent commit's): the same launches with the same arguments in the same order, the same replay keys, one host count per
    segment boundary, the same `last_decode`, and the same bytes in every int32 / uint8 workspace."""
    with open(GOLDEN) as f:
        want = json.load(f)["scenarios"][name]
    res, lines, rec = run_scenario(name)
    check_conditions(name, res, lines)
    # narrowest first, so that a failure names what moved before the hash says that something did
    assert res["last_decode"] == want["last_decode"]
    assert res["host_counts"] == want["host_counts"]
    assert res["keys"] == want["keys"]
    assert res["launches"] == want["launches"]
    assert sorted(res["workspaces"]) == sorted(want["workspaces"]), "the set of int32 / uint8 workspaces changed"
    assert res["workspaces"] == want["workspaces"]
    assert (res["entries"], res["trace_sha256"]) == (want["entries"], want["trace_sha256"])


def test_last_decode_is_the_dict_the_loop_updates():
    """`last_decode` is published after the first segment and is the very dict the later segments update: a caller that reads
    it from the idle hook or between segments sees the pass so far."""
    import care_amd
    import care_amd.engine

    seen = []
    res, lines, rec = run_scenario("greedy_bf16_4096")   # (warm path of the module; the check below runs its own pass)
    eng = rec.engines[0]
    host_count = eng._host_count
    rec.script, rec.consumed = [3000, 0], 0
    eng._host_count = lambda cnt: (seen.append((eng.last_decode, dict(eng.last_decode))), host_count(cnt))[1]
    eng.translate_greedy([t for label, t in rec.inputs])
    assert [s[1]["steps"] for s in seen] == [4, 8] and seen[0][0] is seen[1][0] is eng.last_decode


def _main(argv):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="write tests/golden/decode_launch_trace.json")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose care_amd is recorded (the parent commit's)")
    ap.add_argument("--dump", help="directory for the full traces, <scenario>.jsonl")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.tree))
    import care_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(care_amd.__file__))) == os.path.abspath(args.tree)
    out = {}
    for name in SCENARIOS:
        res, lines, rec = run_scenario(name, care_amd)
        check_conditions(name, res, lines)
        out[name] = res
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + ".jsonl"), "w") as f:
                f.write("\n".join(lines) + "\n")
        print("{:32s} {:5d} launches  {}".format(name, sum(res["launches"].values()), res["trace_sha256"][:16]), flush=True)
    if args.record:
        with open(GOLDEN, "w") as f:
            json.dump(dict(scenarios=out), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    _main(sys.argv[1:])

"""The validation epoch, timed (one JSON line):

    python tools/validation_bench.py [--videos 2990] [--refs 20] [--batch 128] [--repeats 3]

A synthetic MSRVTT-test-shaped split (2990 videos x 20 references of 5 .. 14 words + EOS, V = 10547, words drawn from a Zipf-like
law so that n-grams repeat: tools/scst_bench.py's corpus) and the msrvtt_care model with synthetic weights, at batch 128, greedy
and beam 5.  Per decoding mode, wall clock around a synchronised epoch (median of `repeats` after one warm-up):

1. `ValidationEpoch.run`: decode, score and accumulate on the device, one host read at the end;
2. the decode alone: the same engine calls (and care_beam_winner) per batch, nothing scored;
3. the host route: `Translator.translate_batches` (the pipelined hand-back of python lists) and the Python scorer of the tests
   (tests/capmetrics_reference.py, its CIDEr reference weights cached by a warm-up) - what a tree without the kernels runs.

Every batch reuses one set of 128 clips' features (the last batch a slice of it) under its own video ids: the decode costs what
it costs on distinct features, and the device holds one batch instead of the split.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import capmetrics_reference
from care_amd import MetricBank, ValidationEpoch, get_framework, get_translator
from care_amd.configs import feat_shapes, make_opt
from care_amd.synth import synth_state_dict
from scst_bench import synthetic_corpus

V = 10547


def timed(fn, repeats):
    fn()   # warm-up: workspaces, the engine's packed weights, caches of the host scorer
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return res, dict(median_s=round(statistics.median(out), 4), min_s=round(min(out), 4), max_s=round(max(out), 4), n=len(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--refs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validation_bench.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    refs = synthetic_corpus(a.videos, a.refs)
    t0 = time.perf_counter()
    bank = MetricBank(refs, V, device=dev)
    build_s = time.perf_counter() - t0
    corpus = capmetrics_reference.Corpus(refs)
    opt = make_opt("msrvtt_care")
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, a.batch)]
    batches = [{"feats": [f[: min(a.batch, a.videos - lo)] for f in feats], "video_ids": list(range(lo, min(lo + a.batch, a.videos)))}
               for lo in range(0, a.videos, a.batch)]
    res = dict(tool="validation_bench", videos=a.videos, refs_per_video=a.refs, batch=a.batch, batches=len(batches),
               bank_build_s=round(build_s, 2), clip_keys=int(bank.host["clip_keys"].size), reference_tokens=int(bank.host["ref_tok"].size))
    for beam in (1, 5):
        epoch = ValidationEpoch(opt, model, bank, beam_size=beam)
        translator = get_translator(dict(opt, beam_size=beam))

        def device_epoch():
            return epoch.run(batches)

        def decode_alone():
            with torch.no_grad():
                engine = model.engine()
                for b in batches:
                    with engine.lock:
                        epoch._decode(engine, list(b["feats"]))

        def host_route():
            rows = []
            for b, (hyps, _) in zip(batches, translator.translate_batches([model], ({"feats": b["feats"]} for b in batches))):
                rows += [(h[0], len(h[0]), v) for h, v in zip(hyps, b["video_ids"])]
            return corpus.corpus(corpus.records(*zip(*rows)))

        got, t_dev = timed(device_epoch, a.repeats)
        _, t_dec = timed(decode_alone, a.repeats)
        want, t_host = timed(host_route, a.host_repeats)
        res["greedy" if beam == 1 else "beam%d" % beam] = dict(
            device_epoch=t_dev, decode_alone=t_dec, host_route=t_host,
            host_over_device=round(t_host["median_s"] / t_dev["median_s"], 1),
            scoring_share_of_device_epoch=round(1 - t_dec["median_s"] / t_dev["median_s"], 3), scores=got,
            max_deviation_from_host_route=max(abs(got[k] - want[k]) for k in capmetrics_reference.KEYS))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Sampled decoding, timed (one JSON line):

    python tools/sample_bench.py [--clips 128] [--windows 5] [--window-s 0.3] [--config msrvtt_base_ami] [--mode bf16]

Passes (hipGraph replay, encode included, us per decoder step = pass / T), alternating window by window:
  sample_n1 / sample_n5              engine.translate_sample at `clips` x 1 and x 5 rows, temperature 1, no filter;
  sample_n1_filtered / _n5_filtered  the same with temperature 0.7, top_k 20, top_p 0.9;
  greedy_multi_1x / greedy_multi_5x  the fixed-length multi-launch greedy pass at the same row counts (clips and 5 clips):
                                     what a sampled step adds to is this pass's step;
  beam5                              engine.translate_beam, beam 5, at `clips` clips in its default form.
care_sample_logits alone at clips and 5 clips rows x V = 10547 (row stride 10560, Gaussian logits x 2), each filter off and
on, against the bytes it must read - the row once, rows x V x 4 - at the 6.29 TB/s float4-copy rate.

tools/loss_bench.py's method: device events around a window of calls, every variant warmed up, medians of >= 5 windows
of >= 0.3 s.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from care_amd import _lib, get_framework
from care_amd.configs import feat_shapes, make_opt
from care_amd.engine_sample import pack_params
from care_amd.synth import synth_state_dict
from loss_bench import COPY_RATE, summary, windows

V_ALONE, LD_ALONE = 10547, 10560
FILTERED = dict(temperature=0.7, top_k=20, top_p=0.9)


def passes(model, opt, clips, dev, n_windows, window_s):
    eng = model.engine()
    T = eng.T

    def feats_for(B, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        return [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, B)]

    f1, f5 = feats_for(clips, 5), feats_for(5 * clips, 6)
    seeds = iter(range(1, 1 << 30))

    def sample(n, **kw):
        return lambda: eng.translate_sample(f1, n, seed=next(seeds), use_graph=True, **kw)   # (a new seed every call: one graph)

    def greedy(feats):
        def run():
            keep = eng.resident_max_rows
            eng.resident_max_rows = 0   # the multi-launch forms, fixed length: what the sampled pass runs through
            try:
                eng.translate_greedy(feats, use_graph=True, lean=True, early_exit=False)
            finally:
                eng.resident_max_rows = keep
        return run

    variants = {"sample_n1": sample(1), "sample_n5": sample(5), "sample_n1_filtered": sample(1, **FILTERED),
                "sample_n5_filtered": sample(5, **FILTERED), "greedy_multi_1x": greedy(f1), "greedy_multi_5x": greedy(f5),
                "beam5": lambda: eng.translate_beam(f1, 5, 5, use_graph=True, lean=True)}
    with torch.no_grad():
        ts = windows(variants, n_windows, window_s)
    beam_form = "resident" if eng.last_decode.get("resident") else eng.plan.decode
    out = {}
    for name, t in ts.items():
        out[name] = dict(summary(t), us_per_step=round(statistics.median(t) * 1e6 / T, 2))
    out["beam5"]["form"] = beam_form
    out["sample_graphs"] = sum(1 for k in eng._graphs if k[0] == "sample")
    return out


def alone(rows, dev, n_windows, window_s):
    gen = torch.Generator(device=dev).manual_seed(rows)
    logits = torch.randn(rows, LD_ALONE, generator=gen, device=dev) * 2.0
    pmax, psum, logq = (torch.empty(rows, device=dev) for _ in range(3))
    pidx, nkept = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(2))
    settings = {"none": (1.0, 0, 1.0), "top_k_20": (1.0, 20, 1.0), "top_p_0.9": (1.0, 0, 0.9), "top_k_20_top_p_0.9": (0.7, 20, 0.9)}
    blocks = {}
    for name, (temp, k, p) in settings.items():
        blk = torch.zeros(32, dtype=torch.uint8, device=dev)
        blk[:24] = torch.frombuffer(bytearray(pack_params(17, temp, k, p)), dtype=torch.uint8).to(dev)
        blocks[name] = blk

    def run(name):
        return lambda: _lib.call("care_sample_logits", logits.data_ptr(), LD_ALONE, V_ALONE, rows, None, 3, blocks[name].data_ptr(),
                                 pmax.data_ptr(), pidx.data_ptr(), psum.data_ptr(), logq.data_ptr(), nkept.data_ptr())

    ts = windows({name: run(name) for name in settings}, n_windows, window_s)
    bound = rows * V_ALONE * 4 / COPY_RATE
    out = dict(rows=rows, bytes=rows * V_ALONE * 4, bound_us=round(bound * 1e6, 3))
    for name, t in ts.items():
        med = statistics.median(t)
        out[name] = dict(us=round(med * 1e6, 2), min_us=round(min(t) * 1e6, 2), max_us=round(max(t) * 1e6, 2),
                         share_of_bound=round(bound / med, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--config", default="msrvtt_base_ami")
    ap.add_argument("--mode", default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py measures on the MI355X: no GPU, no numbers")
    if a.windows < 5 or a.window_s < 0.3:
        raise SystemExit("at least 5 windows of at least 0.3 s")
    dev = torch.device("cuda:0")
    opt = make_opt(a.config)
    model = get_framework(opt).eval()
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model.set_compute_dtype(a.mode)
    model.to(dev)
    res = dict(tool="sample_bench", config=a.config, mode=a.mode, clips=a.clips, steps=model.engine().T,
               copy_rate_bytes_per_s=COPY_RATE, passes=passes(model, opt, a.clips, dev, a.windows, a.window_s),
               kernel_alone=[alone(rows, dev, a.windows, a.window_s) for rows in (a.clips, 5 * a.clips)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()

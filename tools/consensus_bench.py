"""The consensus among a clip's sampled captions, timed (one JSON line):

    python tools/consensus_bench.py [--windows 5] [--window-s 0.2] [--repeats 5] [--clips 128] [--videos 2990] [--no-model]

1. THE KERNEL ALONE (care_consensus_score into preallocated outputs, no `pairs`) at 128 clips x 5, 128 x 20, 2048 x 5 and - the
   most one launch takes a clip - 128 x 32 candidates: a clip's candidates are one reference of the corpus with 0 - 3 tokens
   substituted (captions of 5 - 14 tokens + EOS), in a `fed`-shaped buffer; the bank is built over 2990 videos x 20 references.
   Device events around a window of calls, medians of >= 5 windows with the spread; `with_pairs` the same with the [n, n]
   table written.
2. THE CALLS, msrvtt_care with synthetic weights, `--clips` clips x 5 draws, wall clock around a synchronised call, the
   variants alternated, medians of `--repeats` after a warm-up:
   `sample_batch`     the sampled pass, its n captions a clip fetched and turned into lists;
   `consensus_batch`  the same pass, care_consensus_score, the gather of the winners, ONE caption a clip fetched;
   `host`             sample_batch, then tests/consensus_reference.py over the lists (what a caller did before).
   `kernel_in_pass`: care_consensus_score alone on that pass's own `fed` / `length`, and its share of consensus_batch.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from care_amd import CiderBank, _lib
from care_amd.constants import EOS
from concept_bench import summary, windows
from scst_bench import V, synthetic_corpus


def candidates(refs, clips, n, dev, seed=1):
    """(fed int32 [clips n, 31] with BOS in column 0, length) - a clip's candidates: one reference, 0 - 3 tokens substituted."""
    rng = np.random.RandomState(seed)
    fed = np.zeros((clips * n, 31), dtype=np.int32)
    fed[:, 0] = 2
    length = np.zeros(clips * n, dtype=np.int32)
    for b in range(clips):
        video = refs[rng.randint(len(refs))]
        base = video[rng.randint(len(video))][:-1]
        for j in range(n):
            cand = list(base)
            for _ in range(rng.randint(0, 4)):
                cand[rng.randint(len(cand))] = int(rng.randint(6, V))
            cand.append(EOS)
            fed[b * n + j, 1:1 + len(cand)] = cand
            length[b * n + j] = len(cand)
    return torch.from_numpy(fed).to(dev), torch.from_numpy(length).to(dev)


def kernel_alone(bank, refs, clips, n, dev, n_windows, window_s):
    fed, length = candidates(refs, clips, n, dev)
    score = torch.empty(clips, n, device=dev)
    pairs = torch.empty(clips, n, n, device=dev)
    winner = torch.empty(clips, dtype=torch.int32, device=dev)
    row = torch.empty(clips, dtype=torch.int32, device=dev)

    def run(p):
        _lib.call("care_consensus_score", fed.data_ptr(), 31, 1, 30, length.data_ptr(), None, clips, n, int(bank.with_eos), EOS,
                  ctypes.addressof(bank.desc), score.data_ptr(), p, winner.data_ptr(), row.data_ptr())

    ts = windows({"kernel": lambda: run(None), "with_pairs": lambda: run(pairs.data_ptr())}, n_windows, window_s)
    out = {name: summary(t) for name, t in ts.items()}
    out["mean_tokens"] = round(float(length.float().mean()), 1)
    out["mean_score"] = round(float(score.mean()), 3)
    return out


def calls(bank, refs, clips, n, dev, repeats, n_windows, window_s):
    import cider_reference as C
    import consensus_reference as R
    from care_amd import get_framework, get_translator
    from care_amd.configs import feat_shapes, make_opt
    from care_amd.synth import synth_state_dict

    opt = make_opt("msrvtt_care")
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(5)
    batch = {"feats": [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, clips)]}
    tr = get_translator(opt)
    corpus = C.Corpus(refs)
    kw = dict(n_samples=n, seed=3)

    def host():
        hyps, scores = tr.sample_batch([model], batch, **kw)
        out = []
        for h, s in zip(hyps, scores):
            j = R.clip(corpus, h)[2]
            out.append((h[j], s[j]))
        return out

    variants = {"sample_batch": lambda: tr.sample_batch([model], batch, **kw),
                "consensus_batch": lambda: tr.consensus_batch([model], batch, bank, **kw), "host": host}
    ts = {name: [] for name in variants}
    for fn in variants.values():
        fn()
        fn()
    for _ in range(repeats):   # alternated
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    res = {name: summary(t, 1e3, "ms") for name, t in ts.items()}
    # the kernel on that pass's own draws
    with torch.no_grad(), model.engine().lock:
        _, fed, length, _, _ = model.engine().translate_sample(batch["feats"], n, seed=3)
        fed, length = fed.clone(), length.clone()
    score = torch.empty(clips, n, device=dev)
    winner = torch.empty(clips, dtype=torch.int32, device=dev)
    T1 = fed.shape[1]

    def run():
        _lib.call("care_consensus_score", fed.data_ptr(), T1, 1, T1 - 1, length.data_ptr(), None, clips, n, int(bank.with_eos), EOS,
                  ctypes.addressof(bank.desc), score.data_ptr(), None, winner.data_ptr(), None)

    res["kernel_in_pass"] = summary(windows({"kernel": run}, n_windows, window_s)["kernel"])
    res["mean_tokens_of_a_draw"] = round(float(length.float().mean()), 1)
    res["kernel_share_of_consensus_batch"] = round(res["kernel_in_pass"]["us"] * 1e-3 / res["consensus_batch"]["ms"], 4)
    res["kernel_over_sampled_pass"] = round(res["kernel_in_pass"]["us"] * 1e-3 / res["sample_batch"]["ms"], 4)
    res["consensus_over_sample_batch"] = round(res["consensus_batch"]["ms"] / res["sample_batch"]["ms"], 3)
    res["host_over_consensus_batch"] = round(res["host"]["ms"] / res["consensus_batch"]["ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consensus_bench.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    refs = synthetic_corpus(a.videos, 20)
    bank = CiderBank(refs, V, device=dev)
    res = dict(tool="consensus_bench", videos=a.videos, corpus_keys=int(bank.host["corpus_keys"].size))
    res["kernel"] = {"%dx%d" % (c, n): kernel_alone(bank, refs, c, n, dev, a.windows, a.window_s)
                     for c, n in ((128, 5), (128, 20), (2048, 5), (128, 32))}
    if not a.no_model:
        res["calls_%dx5" % a.clips] = calls(bank, refs, a.clips, 5, dev, a.repeats, a.windows, a.window_s)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

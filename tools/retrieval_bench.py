"""Caption retrieval, timed per call (one JSON line):

    python tools/retrieval_bench.py [--rows 1,16,128,2048] [--topk 20,100] [--windows 5] [--window-s 0.3]

A bank of M = 130 260 captions (the MSRVTT training captions), D = 512, `unique` with 12 % of the rows repeating an earlier
string (a few strings hundreds of times, most twice; repeated strings carry the same embedding), every clip with an own
range of 20 captions.  Timed: `CaptionBank.search` on unit queries - care_retrieval_topk with its output and scratch
allocations: the scan, the group selection, the re-scoring and the ranking - against the eager form on the same device,
`q @ bank.T` then `topk` (no filter at all, and already kinder than the reference's full sort).  topk = 1 is timed as well: its
re-scoring and ranking are next to nothing, so it shows what the scan and the group selection take.

tools/loss_bench.py's method: device events around a window of calls, every variant warmed up, the variants alternating
window by window, medians of >= 5 windows of >= 0.3 s.  Each figure is set against its bound: the bank's bytes at the 6.29 TB/s
float4-copy rate, or 2 B M D flops at the 157.3 TFLOP/s of the f32 MFMA, whichever is larger.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from care_amd import CaptionBank
from loss_bench import COPY_RATE, summary, windows

M, D = 130260, 512
F32_MFMA_PEAK = 157.3e12


def make_bank(dev):
    rng = np.random.default_rng(0)
    embs = rng.standard_normal((M, D), dtype=np.float32)
    captions = ["caption {}".format(j) for j in range(M)]
    repeats = rng.permutation(np.arange(1000, M))[: int(0.12 * M)]
    heavy = rng.integers(0, 1000, size=8)                                   # eight strings a few hundred times each
    for n, j in enumerate(np.sort(repeats)):
        src = int(heavy[n % 8]) if n % 6 == 0 else int(rng.integers(0, j))
        captions[j], embs[j] = captions[src], embs[src]
    return CaptionBank(embs, captions, unique=True, device=dev), len(set(captions))


def one(bank, B, topk, dev, n_windows, window_s):
    gen = torch.Generator(device=dev).manual_seed(B)
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=gen, device=dev), dim=-1)
    start = (torch.arange(B, dtype=torch.int32) * 20 % (M - 20)).to(dev)
    own = (start, start + 20)                                               # device int32 pairs: no conversion inside the call

    def ours():
        bank.search(q, topk, own)

    def eager():
        torch.topk(q @ bank.unit.t(), topk, dim=-1)

    ts = windows({"care_amd": ours, "eager_torch": eager}, n_windows, window_s)
    ours_s, eager_s = statistics.median(ts["care_amd"]), statistics.median(ts["eager_torch"])
    t_bytes, t_flops = M * D * 4 / COPY_RATE, 2.0 * B * M * D / F32_MFMA_PEAK
    bound = max(t_bytes, t_flops)
    return dict(rows=B, topk=topk, care_amd=summary(ts["care_amd"]), eager_torch=summary(ts["eager_torch"]),
                eager_over_care_amd=round(eager_s / ours_s, 3), bound="bank bytes" if t_bytes >= t_flops else "f32 MFMA",
                bound_ms=round(bound * 1e3, 4), care_amd_share_of_bound=round(bound / ours_s, 3),
                eager_share_of_bound=round(bound / eager_s, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,16,128,2048")
    ap.add_argument("--topk", default="1,20,100")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench.py measures on the MI355X: no GPU, no numbers")
    if a.windows < 5 or a.window_s < 0.3:
        raise SystemExit("at least 5 windows of at least 0.3 s")
    dev = torch.device("cuda:0")
    bank, strings = make_bank(dev)
    res = dict(tool="retrieval_bench", bank=dict(captions=M, dim=D, distinct_strings=strings, groups_exact=bank.groups_exact),
               copy_rate_bytes_per_s=COPY_RATE, f32_mfma_flops_per_s=F32_MFMA_PEAK,
               calls=[one(bank, B, k, dev, a.windows, a.window_s) for B in (int(v) for v in a.rows.split(","))
                      for k in (int(v) for v in a.topk.split(","))])
    print(json.dumps(res))


if __name__ == "__main__":
    main()

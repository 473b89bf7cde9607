"""The device-built batch, timed (one JSON line per part):

    python tools/batch_bench.py [--videos 2990] [--caps 20] [--batches 24] [--steps 6] [--parts 123]

A synthetic corpus in the MSRVTT shapes (a / m / i of 60 frames x 128 / 2048 / 512 floats, `r` of 20 x 512, `--caps` captions of
5 .. 14 words a video: tools/scst_bench.py's corpus) held twice: in a `ClipStore` on the device and as in-memory tables for the
host path this project had before - `data.load_video_feats` + `collate_feats` + `FeaturePrefetcher` - which flatters the host:
the reference reads HDF5.  2990 videos are 2.05 GB of tables, eight times the Infinity Cache; every timed batch holds other
clips than the one before.

1. Time per batch, 128 and 512 clips, and one validation pass over all videos at 128: the store's loader against the host
   path, each a host clock around `--batches` batches that ends in a device synchronise (the host path is counted up to the
   hand-over of its device tensors; it builds no captions, which flatters it again).
2. care_batch_gather alone, device events around each of the distinct batches of part 1 (median): bytes read + written over
   its time, beside a device-to-device copy of as many bytes on the same box.
3. `--steps` training steps of InterplayStep at 512 clips and a validation epoch (ValidationEpoch, greedy, batch 128) fed from
   the store against fed by the host path (which gets its captions as ready device tensors).
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
import numpy as np
import torch

from care_amd import ClipStore, InterplayStep, MetricBank, ValidationEpoch, _lib, get_framework
from care_amd.configs import make_opt
from care_amd.constants import BOS
from care_amd.data import FeaturePrefetcher, collate_feats, load_video_feats
from care_amd.synth import synth_state_dict
from scst_bench import synthetic_corpus

V = 10547
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def corpus(videos, caps):
    gen = torch.Generator().manual_seed(0)
    names = ["video%d" % v for v in range(videos)]
    dbs = {}
    for ch, (n, dim) in {"a": (60, 128), "m": (60, 2048), "i": (60, 512), "r": (20, 512)}.items():
        big = torch.randn(videos, n, dim, generator=gen).numpy()
        dbs[ch] = [{name: big[v] for v, name in enumerate(names)}]
    refs = synthetic_corpus(videos, caps)
    return dbs, names, refs, {name: [[BOS] + c for c in refs[v]] for v, name in enumerate(names)}


def wall(fn, n_batches):
    """Seconds a batch: a host clock around a walk that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = fn()
    torch.cuda.synchronize()
    assert n == n_batches, (n, n_batches)
    return (time.perf_counter() - t0) / n


def host_batches(dbs, names, opt, order, batch_size, n_batches):
    for k in range(n_batches):
        yield collate_feats([load_video_feats(dbs, names[v], opt) for v in order[k * batch_size: (k + 1) * batch_size]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--caps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--parts", default="123")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench.py measures on the MI355X: no GPU, no numbers")
    dev = torch.device("cuda:0")
    opt = make_opt("msrvtt_care", load_feats_type=0, **NO_DROP)
    dbs, names, refs, captions = corpus(a.videos, a.caps)
    t0 = time.perf_counter()
    store = ClipStore(opt, dbs, names, captions=captions, device=dev)
    torch.cuda.synchronize()
    clip_bytes = sum(t.row_bytes * (1 if t.block else store.n_frames) for t in store.tables)
    print(json.dumps(dict(tool="batch_bench", part=0, videos=a.videos, items=store.n_items("train"), store_build_s=round(time.perf_counter() - t0, 2),
                          table_bytes=sum(t.data.numel() * t.data.element_size() for t in store.tables), clip_bytes=clip_bytes,
                          device=torch.cuda.get_device_name(0))), flush=True)
    item_video = store.host_captions["cap_video"]

    def store_walk(mode, bs, epoch, limit):
        n = 0
        for n, _ in enumerate(store.loader(mode=mode, batch_size=bs, epoch=epoch, seed=1), 1):
            if n == limit:
                break
        return n

    def host_walk(order, bs, limit):
        n = 0
        for n, _ in enumerate(FeaturePrefetcher(host_batches(dbs, names, opt, order, bs, limit), dev), 1):
            pass
        return n

    # ---- 1 + 2
    if "1" in a.parts or "2" in a.parts:
        for bs in (128, 512):
            nb = min(a.batches, store.n_items("train") // bs)
            order = item_video[np.random.RandomState(bs).permutation(store.n_items("train"))]
            store_walk("train", bs, 0, 2)
            host_walk(order, bs, 2)                                   # warm-up: slots, pinned buffers, code objects
            t_store = [wall(lambda e=e: store_walk("train", bs, e, nb), nb) for e in (1, 2, 3)]
            t_host = [wall(lambda: host_walk(order, bs, nb), nb) for _ in range(2)]
            _lib.TIMING = {}
            store_walk("train", bs, 4, nb)
            torch.cuda.synchronize()
            ev, _lib.TIMING = _lib.TIMING, None
            us = {tag: sorted(s.elapsed_time(e) * 1e3 for s, e in pairs) for tag, pairs in ev.items()}
            moved = 2 * bs * clip_bytes
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copies = []
            for _ in range(8):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                dst.copy_(src)
                e.record()
                torch.cuda.synchronize()
                copies.append(s.elapsed_time(e) * 1e3)
            g = statistics.median(us["batch_gather"])
            print(json.dumps(dict(part=12, clips=bs, batches=nb, store_ms_per_batch=[round(t * 1e3, 3) for t in t_store],
                                  host_ms_per_batch=[round(t * 1e3, 2) for t in t_host],
                                  host_over_store=round(min(t_host) / statistics.median(t_store), 1),
                                  kernel_us_median={k: round(statistics.median(v), 1) for k, v in us.items()},
                                  gather_us_min_max=[round(us["batch_gather"][0], 1), round(us["batch_gather"][-1], 1)],
                                  gather_bytes=moved, gather_TBps=round(moved / g / 1e6, 3),
                                  d2d_copy_us_median=round(statistics.median(copies), 1),
                                  d2d_copy_TBps=round(moved / statistics.median(copies) / 1e6, 3))), flush=True)
        nb = -(-a.videos // 128)
        order = np.arange(a.videos)
        t_store = [wall(lambda: store_walk("validate", 128, 0, nb), nb) * nb for _ in range(3)]
        t_host = [wall(lambda: host_walk(order, 128, nb), nb) * nb for _ in range(2)]
        print(json.dumps(dict(part=1, what="all videos once, batch 128, features only", store_s=[round(t, 4) for t in t_store],
                              host_s=[round(t, 3) for t in t_host])), flush=True)

    # ---- 3
    if "3" in a.parts:
        model = get_framework(opt)
        model.load_state_dict(synth_state_dict(0, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
        model = model.to(dev).train()
        step = InterplayStep(opt, model)
        bs, n = 512, a.steps
        order = item_video[np.random.RandomState(7).permutation(store.n_items("train"))]
        text = {k: v.clone() for k, v in next(iter(store.loader(mode="train", batch_size=bs, seed=1))).items()
                if k in ("input_ids", "labels", "labels_attr")}

        def train_store(epoch):
            k = 0
            for k, batch in enumerate(store.loader(mode="train", batch_size=bs, epoch=epoch, seed=1), 1):
                step.training_step(batch)
                if k == n:
                    break
            return k

        def train_host():
            k = 0
            for k, feats in enumerate(FeaturePrefetcher(host_batches(dbs, names, opt, order, bs, n), dev), 1):
                step.training_step(dict(text, feats=feats))
            return k

        train_store(0)
        train_host()
        res = dict(part=3, clips=bs, steps=n, step_ms_fed_by_store=[], step_ms_fed_by_host=[])
        for e in (1, 2):      # alternating
            res["step_ms_fed_by_store"].append(round(wall(lambda: train_store(e), n) * 1e3, 2))
            res["step_ms_fed_by_host"].append(round(wall(train_host, n) * 1e3, 2))
        del step
        model.eval()
        bank = MetricBank(refs, V, with_eos=True, device=dev)
        epoch = ValidationEpoch(opt, model, bank, beam_size=1)
        nb = -(-a.videos // 128)

        def val_store():
            epoch.scores(epoch.accumulate(store.loader(mode="validate", batch_size=128)))
            return nb

        def val_host():
            feats = FeaturePrefetcher(host_batches(dbs, names, opt, np.arange(a.videos), 128, nb), dev)
            epoch.scores(epoch.accumulate({"feats": f, "video_ids": list(range(k * 128, min(a.videos, (k + 1) * 128)))} for k, f in enumerate(feats)))
            return nb

        val_store()
        val_host()
        res["validation_epoch_fed_by_store_s"], res["validation_epoch_fed_by_host_s"] = [], []
        for _ in range(2):
            res["validation_epoch_fed_by_store_s"].append(round(wall(val_store, nb) * nb, 4))
            res["validation_epoch_fed_by_host_s"].append(round(wall(val_host, nb) * nb, 3))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""Self-critical training, timed (one JSON line):

    python tools/scst_bench.py [--videos 6513] [--refs 20] [--windows 5] [--window-s 0.3] [--no-step] [--fused-head]

1. THE REWARD ALONE: CiderBank.score (care_cider_score) at 128 and 640 candidates of 30 tokens against a synthetic
   MSRVTT-shaped corpus (6513 videos x 20 references of 5 .. 14 words + EOS, V = 10547, words drawn from a Zipf-like law so that
   n-grams repeat), against the host route a tree without the kernel forces: `fed` / `length` device-to-host, the Python of
   tests/cider_reference.py (its reference weights cached, as a trainer would), the rewards host-to-device.  The host route is
   wall clock around a synchronised call (median of 5 after one warm-up).  Also the bytes a candidate's workgroup must read -
   the keys and weights of its video's references, and ceil(log2 n_corpus) 8-byte probes per unique n-gram - over the time,
   as a share of the float4-copy rate.
2. THE LOSS, forward + backward, on logits [640, 29, 10547]: care_amd.self_critical_loss against eager torch (log_softmax,
   gather, weighted mean) and against care_lang_loss_fwd / _bwd (eps = 0) on the same logits and labels.
3. THE WHOLE STEP at 128 clips x 5 samples (msrvtt_care, greedy baseline): SelfCriticalStep.training_step, the same step with
   the reward computed on the host, and the plain cross-entropy step of tools/train_prof.py at 640 sequences.

With --fused-head (and nothing else measured): the loss WITH the head, forward + backward, on hidden states [640, 29, 512] -
care_amd.self_critical_head_loss against `_Linear` + self_critical_loss - and SelfCriticalStep(fused_head=True) against the
unfused step at 128 clips x 5; each with every position live (the synthetic model never draws EOS) and with the captions cut to
5 .. 14 tokens (about a quarter live), with the peak memory each variant allocates above its starting level.

tools/loss_bench.py's method: device events around a window of calls; every variant warmed up first; the variants ALTERNATE
window by window in one process; medians of >= 5 windows of >= 0.3 s each, with min and max.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cider_reference
from care_amd import CiderBank, SelfCriticalStep, configure_optimizers, get_criterion, get_framework, self_critical_loss
from care_amd.configs import feat_shapes, make_opt
from care_amd.constants import EOS, PAD
from care_amd.criterion import _LangLoss
from care_amd.synth import synth_state_dict
from loss_bench import COPY_RATE, EPS, K, T, V, mixed_labels, summary, windows


def synthetic_corpus(videos, refs_per_video, seed=0):
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, V - 5)
    p /= p.sum()
    words = rng.choice(np.arange(6, V), size=(videos, refs_per_video, 14), p=p)
    lengths = rng.randint(5, 15, size=(videos, refs_per_video))
    return [[words[v, r, :lengths[v, r]].tolist() + [EOS] for r in range(refs_per_video)] for v in range(videos)]


def candidates(refs, rows, dev, seed=1):
    """rows captions of 30 tokens in a `fed`-shaped buffer [rows, 31]: a reference of the row's video, then words of the corpus' law."""
    rng = np.random.RandomState(seed)
    video = rng.randint(0, len(refs), size=rows).astype(np.int32)
    fed = np.full((rows, 31), 2, dtype=np.int32)
    for r in range(rows):
        ref = refs[video[r]][r % len(refs[video[r]])][:-1]
        other = refs[rng.randint(len(refs))][0][:-1]
        toks = (ref + other + ref + other)[:29] + [EOS]
        fed[r, 1:1 + len(toks)] = toks
    length = np.full(rows, 30, dtype=np.int32)
    return torch.from_numpy(fed).to(dev), torch.from_numpy(length).to(dev), torch.from_numpy(video).to(dev)


class HostBank(object):
    """The route without care_cider_score: everything through the host."""

    def __init__(self, bank, corpus):
        self.bank, self.corpus, self.with_eos = bank, corpus, bank.with_eos

    def rows(self, video_ids):
        return self.bank.rows(video_ids)

    def score(self, tokens, length, video, out=None, offset=0, bad=None):
        toks, ln, vd = tokens.cpu().numpy()[:, offset:], length.cpu().numpy(), video.cpu().numpy()
        return torch.tensor(self.corpus.scores(toks.tolist(), ln.tolist(), vd.tolist()), dtype=torch.float32).to(tokens.device)


def reward_alone(bank, corpus, refs, rows, dev, n_windows, window_s):
    fed, length, video = candidates(refs, rows, dev)
    out = torch.empty(rows, device=dev)
    host = HostBank(bank, corpus)

    def ours():
        bank.score(fed[:, 1:], length, video, out=out)

    ts = windows({"care_amd": ours}, n_windows, window_s)
    got = out.cpu().double().numpy()
    want = host.score(fed[:, 1:], length, video).cpu().double().numpy()      # (also the host route's warm-up; rounded to fp32 like the kernel's)
    host_s = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.score(fed[:, 1:], length, video)
        torch.cuda.synchronize()
        host_s.append(time.perf_counter() - t0)
    h = bank.host
    vid = video.cpu().numpy()
    ref_bytes = sum(16 * int(h["ref_start"][h["vid_start"][v + 1]] - h["ref_start"][h["vid_start"][v]]) for v in vid)
    probes = rows * 114 * 8 * int(math.ceil(math.log2(max(2, h["corpus_keys"].size))))   # 30 + 29 + 28 + 27 n-grams at most
    ours_s = statistics.median(ts["care_amd"])
    return dict(rows=rows, care_amd=summary(ts["care_amd"]), host_route=summary(host_s), host_over_care_amd=round(statistics.median(host_s) / ours_s, 1),
                reference_bytes=ref_bytes, probe_bytes=probes, share_of_copy_rate=round((ref_bytes + probes) / ours_s / COPY_RATE, 5),
                mean_reward=float(got.mean()), max_deviation_from_host_route=float(np.abs(got - want).max()))


def loss_alone(seqs, dev, n_windows, window_s):
    gen = torch.Generator(device=dev).manual_seed(seqs)
    logits = (torch.randn(seqs, T, V, generator=gen, device=dev) * 2.0).requires_grad_(True)
    labels = mixed_labels(seqs, 11).to(dev)
    labels32 = labels.to(torch.int32)
    adv = torch.randn(seqs, generator=gen, device=dev)

    def ours():
        logits.grad = None
        self_critical_loss(logits, labels, adv).backward()

    def eager():
        logits.grad = None
        logp = torch.log_softmax(logits, dim=-1).gather(2, labels.unsqueeze(2)).squeeze(2)
        live = labels.ne(PAD)
        (-(adv.view(-1, 1) * logp * live).sum() / live.sum()).backward()

    def lang():
        logits.grad = None
        _LangLoss.apply(logits, labels32, 0.0, None)[0].backward()

    ours()
    g_ours, l_ours = logits.grad.clone(), float(self_critical_loss(logits, labels, adv).detach())
    eager()
    diff = float((g_ours - logits.grad).abs().max() / logits.grad.abs().max())
    del g_ours
    ts = windows({"care_amd": ours, "eager_torch": eager, "care_lang_loss": lang}, n_windows, window_s)
    med = {k: statistics.median(v) for k, v in ts.items()}
    live_rows = int(labels.ne(PAD).sum())
    floor = 4 * V * (2 * live_rows + seqs * T)          # a live row read twice, every row of the gradient written
    return dict(sequences=seqs, live_rows=live_rows, floor_bytes=floor, floor_ms_at_copy_rate=round(floor / COPY_RATE * 1e3, 4),
                **{k: summary(v) for k, v in ts.items()}, eager_over_care_amd=round(med["eager_torch"] / med["care_amd"], 3),
                care_amd_over_lang_loss=round(med["care_amd"] / med["care_lang_loss"], 3),
                care_amd_share_of_copy_rate=round(floor / med["care_amd"] / COPY_RATE, 3), loss=l_ours, max_rel_grad_difference_to_eager=diff)


def _model(opt, seed, dev):
    model = get_framework(opt)
    model.load_state_dict(synth_state_dict(seed, [(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    return model.to(dev).train()


def whole_step(bank, corpus, clips, n, dev, n_windows, window_s):
    opt = make_opt("msrvtt_care", label_smoothing=EPS, gradient_clip_val=5.0)
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, clips)]
    video_ids = np.random.RandomState(2).randint(0, bank.n_videos, size=clips).tolist()
    batch = {"feats": feats, "video_ids": video_ids}
    hip = SelfCriticalStep(opt, _model(opt, 0, dev), bank, n_samples=n, baseline="greedy")
    hst = SelfCriticalStep(opt, _model(opt, 0, dev), bank, n_samples=n, baseline="greedy")
    hst.bank = HostBank(bank, corpus)

    seqs = clips * n
    feats_x = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, seqs)]
    labels = mixed_labels(seqs, 12)
    ids = torch.full_like(labels, PAD)
    ids[:, 0] = 2
    ids[:, 1:] = labels[:, :-1]
    labels_attr = (torch.rand(seqs, K, generator=gen, device=dev) > 0.96).float()
    xe_batch = {"feats": feats_x, "input_ids": ids.to(dev), "labels": labels.to(dev), "labels_attr": labels_attr}
    xe_model = _model(opt, 0, dev)
    xe_crit = get_criterion(opt, override_opt={"calculate_mAP": False})
    xe_optim = configure_optimizers(opt, xe_model)["optimizer"]

    def cross_entropy_step():
        loss = xe_crit.get_loss({**xe_model(xe_batch, current_epoch=0), **xe_batch})
        xe_optim.zero_grad()
        loss.backward()
        xe_optim.step()

    ts = windows({"cross_entropy_step": cross_entropy_step, "scst_care_amd": lambda: hip.training_step(batch),
                  "scst_reward_on_host": lambda: hst.training_step(batch)}, n_windows, window_s)
    xe_crit.reset_loss_recorder()
    live = int((hip.last["labels"] != PAD).sum())
    return dict(clips=clips, n_samples=n, sequences=seqs, live_positions_scst=live, live_positions_cross_entropy=int(labels.ne(PAD).sum()),
                mean_reward=float(hip.last["mean_reward"]), **{k: summary(v) for k, v in ts.items()})


def cut_lengths(rows, seed, dev):
    """int32 [rows]: caption lengths of 5 .. 14 tokens (the corpus' own law) - about a quarter of 29 positions live."""
    return torch.from_numpy(np.random.RandomState(seed).randint(5, 15, size=rows).astype(np.int32)).to(dev)


def peak_rise(fn):
    """Bytes one call of `fn` allocates above its starting level at its peak."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def head_loss_alone(seqs, d, dev, n_windows, window_s, quarter):
    """The loss with the head, forward + backward, on hidden states [seqs, 29, d]: self_critical_head_loss (the live count given,
    as SelfCriticalStep gives it) against `_Linear` + self_critical_loss on the same hidden states.  quarter: captions of 5 .. 14
    tokens; else every position live (what the synthetic model of the whole step samples: it never draws EOS)."""
    from care_amd import self_critical_head_loss
    from care_amd.training import _Linear

    gen = torch.Generator(device=dev).manual_seed(seqs + int(quarter))
    hidden = torch.randn(seqs, T, d, generator=gen, device=dev).requires_grad_(True)
    W = (torch.randn(V, d, generator=gen, device=dev) * (2.0 / math.sqrt(d))).requires_grad_(True)
    labels = torch.randint(6, V, (seqs, T), generator=gen, device=dev)
    if quarter:
        labels = torch.where(torch.arange(T, device=dev).view(1, T) < cut_lengths(seqs, 3, dev).view(-1, 1), labels, torch.zeros_like(labels))
    live = int((labels != PAD).sum())
    adv = torch.randn(seqs, generator=gen, device=dev)

    def fused():
        hidden.grad = W.grad = None
        self_critical_head_loss(hidden, W, labels, adv, live=live).backward()

    def unfused():
        hidden.grad = W.grad = None
        self_critical_loss(_Linear.apply(hidden.view(seqs * T, d), W, None).view(seqs, T, V), labels, adv).backward()

    fused()
    gh, gw, lf = hidden.grad.clone(), W.grad.clone(), float(self_critical_head_loss(hidden, W, labels, adv, live=live).detach())
    unfused()
    diff_h = float((gh - hidden.grad).abs().max() / hidden.grad.abs().max())
    diff_w = float((gw - W.grad).abs().max() / W.grad.abs().max())
    lu = float(self_critical_loss(_Linear.apply(hidden.view(seqs * T, d), W, None).view(seqs, T, V), labels, adv).detach())
    del gh, gw
    peaks = {"fused": peak_rise(fused), "unfused": peak_rise(unfused)}
    ts = windows({"fused": fused, "unfused": unfused}, n_windows, window_s)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return dict(sequences=seqs, positions=seqs * T, live_rows=live, live_share=round(live / (seqs * T), 3), d=d,
                **{k: summary(v) for k, v in ts.items()}, unfused_over_fused=round(med["unfused"] / med["fused"], 3),
                peak_rise_mb={k: round(v / 2 ** 20, 1) for k, v in peaks.items()}, one_logits_tensor_mb=round(seqs * T * V * 4 / 2 ** 20, 1),
                loss_fused=lf, loss_unfused=lu, max_rel_dhidden_difference=diff_h, max_rel_dw_difference=diff_w)


def whole_step_fused(bank, clips, n, dev, n_windows, window_s, quarter):
    """SelfCriticalStep with fused_head=True against the same step without, alternated.  quarter: the sampled captions are cut
    to 5 .. 14 tokens behind the decode (the synthetic model never draws EOS: all 29 positions of every sample are live)."""
    from care_amd import scst

    opt = make_opt("msrvtt_care", label_smoothing=EPS, gradient_clip_val=5.0)
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = [torch.randn(s, generator=gen, device=dev) for s in feat_shapes(opt, clips)]
    batch = {"feats": feats, "video_ids": np.random.RandomState(2).randint(0, bank.n_videos, size=clips).tolist()}
    steps = {"fused": SelfCriticalStep(opt, _model(opt, 0, dev), bank, n_samples=n, baseline="greedy", fused_head=True),
             "unfused": SelfCriticalStep(opt, _model(opt, 0, dev), bank, n_samples=n, baseline="greedy")}
    plain, cut = scst.sample_to_labels, cut_lengths(clips * n, 4, dev)
    if quarter:
        scst.sample_to_labels = lambda fed, length, t: plain(fed, torch.minimum(length, cut), t)
    try:
        peaks = {}
        for k, s in steps.items():
            s.training_step(batch)      # (the first step builds the optimiser's state)
            peaks[k] = peak_rise(lambda: s.training_step(batch))
        ts = windows({k: (lambda s=s: s.training_step(batch)) for k, s in steps.items()}, n_windows, window_s)
    finally:
        scst.sample_to_labels = plain
    med = {k: statistics.median(v) for k, v in ts.items()}
    live = int((steps["fused"].last["labels"] != PAD).sum())
    return dict(clips=clips, n_samples=n, sequences=clips * n, live_positions=live, live_share=round(live / (clips * n * T), 3),
                **{k: summary(v) for k, v in ts.items()}, unfused_over_fused=round(med["unfused"] / med["fused"], 3),
                peak_rise_mb={k: round(v / 2 ** 20, 1) for k, v in peaks.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=6513)
    ap.add_argument("--refs", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    ap.add_argument("--fused-head", action="store_true", help="the fused-head variants of the loss rows and of the whole-step row, "
                    "each against the unfused path, with every position live and with about a quarter live - and nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scst_bench.py measures on the MI355X: no GPU, no numbers")
    if a.windows < 5 or a.window_s < 0.3:
        raise SystemExit("at least 5 windows of at least 0.3 s")
    dev = torch.device("cuda:0")
    refs = synthetic_corpus(a.videos, a.refs)
    t0 = time.perf_counter()
    bank = CiderBank(refs, V, with_eos=True, device=dev)
    build_s = time.perf_counter() - t0
    if a.fused_head:
        res = dict(tool="scst_bench --fused-head", vocab=V,
                   head_loss=[head_loss_alone(640, 512, dev, a.windows, a.window_s, quarter) for quarter in (False, True)])
        if not a.no_step:
            res["whole_step"] = [whole_step_fused(bank, 128, 5, dev, a.windows, a.window_s, quarter) for quarter in (False, True)]
        print(json.dumps(res))
        return
    corpus = cider_reference.Corpus(refs, with_eos=True)
    res = dict(tool="scst_bench", corpus=dict(videos=a.videos, refs_per_video=a.refs, vocab=V, unique_ngrams=int(bank.host["corpus_keys"].size),
                                              reference_keys=int(bank.host["ref_keys"].size), bank_build_s=round(build_s, 2)),
               copy_rate_bytes_per_s=COPY_RATE,
               reward_alone=[reward_alone(bank, corpus, refs, rows, dev, a.windows, a.window_s) for rows in (128, 640)],
               loss_alone=loss_alone(640, dev, a.windows, a.window_s))
    if not a.no_step:
        res["whole_step"] = whole_step(bank, corpus, 128, 5, dev, a.windows, a.window_s)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

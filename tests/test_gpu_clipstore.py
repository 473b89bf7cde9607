"""GPU: `care_amd.ClipStore` end to end - a 40-video synthetic corpus in the msrvtt_care layout (a / m / i of 60 frames, `r` of 20
rows, 1 .. 5 captions a video) against the same batches assembled on the host by tests/batch_reference.py, tensor for tensor
and bit for bit; then the three consumers (InterplayStep, SelfCriticalStep, ValidationEpoch) fed from the store's loader
against the same step / epoch fed with the host-built batches, from the same seeds: identical batches through deterministic
kernels, so the losses and scores must have the same bits.  Nothing here has a tolerance.

The models are freshly initialised: their captions share next to nothing with the random references (rewards and scores near
zero), so the self-critical and validation tests show that the batches are consumed and agree, the interplay test (captioning
loss 89.9, distillation 0.18) that the numbers do.  Measured on one MI355X: this file 6.3 s, the slowest test 2.3 s."""
import gc

import numpy as np
import pytest
import torch

import batch_reference as R
from test_gpu_backward_kernels import DEV

pytestmark = pytest.mark.gpu

N_VIDEOS, MAX_LEN, BATCH = 40, 10, 16
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
MISSING = "video7"            # absent from the motion table: zeros
_state = {}


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    """(tests/test_gpu_interplay_step.py: modules, optimisers and engines are collected right behind the test that built them)"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _opt(**over):
    from care_amd.configs import make_opt

    return make_opt("msrvtt_care", max_len=MAX_LEN, label_smoothing=0.1, learning_rate=1e-3, gradient_clip_val=5.0, load_feats_type=0,
                    **NO_DROP, **over)


def _corpus():
    """(databases, names, captions) and the reference's ingested tables - built once, never changed."""
    if "corpus" not in _state:
        opt = _opt()
        rng = np.random.RandomState(40)
        names = ["video%d" % (100 + 3 * v) for v in range(N_VIDEOS)]
        names[7] = MISSING
        dbs = {"a": [{v: rng.randn(60, 128).astype(np.float32) for v in names}],
               "m": [{v: rng.randn(60, 2048).astype(np.float32) for v in names if v != MISSING}],
               "i": [{v: rng.randn(60, 500).astype(np.float32) for v in names}, {v: rng.randn(12).astype(np.float32) for v in names}],
               "r": [{v: rng.randn(23, 512).astype(np.float32) for v in names}]}
        captions = {}
        for k, v in enumerate(names):   # lengths 2 .. 14 against max_len 10; words over a small range so that concepts repeat
            captions[v] = [[R.BOS] + rng.randint(6, 700, size=rng.randint(0, 13)).tolist() + [R.EOS] for _ in range(1 + k % 5)]
        tables = [R.ingest_modality(dbs["a"], names, 128), R.ingest_modality(dbs["m"], names, 2048),
                  R.ingest_modality(dbs["i"], names, 512), R.ingest_retrieval(dbs["r"][0], names, opt["retrieval_topk"])]
        _state["corpus"] = (dbs, names, captions, tables)
    return _state["corpus"]


def _store(dtype=torch.float32, **over):
    from care_amd import ClipStore

    key = (dtype, tuple(sorted(over.items())))
    if key not in _state:
        dbs, names, captions, _ = _corpus()
        _state[key] = ClipStore(_opt(**over), dbs, names, captions=captions, dtype=dtype, device=DEV)
    return _state[key]


def _host(positions, mode, epoch, seed, items=None, random_type="segment_random", tables=None):
    """The reference's batch of infoset positions `positions`, as numpy arrays."""
    _, names, captions, ref_tables = _corpus()
    items = items if items is not None else R.infoset(captions, names, mode)
    return R.host_batch(tables or ref_tables, [60, 60, 60, 20], captions, names, items, positions, mode, 28, MAX_LEN,
                        random_type=random_type, seed=seed, epoch=epoch, retrieval=(3,))


def _assert_same(batch, want, what):
    assert sorted(batch) == sorted(want), what
    for k, w in want.items():
        got = batch[k]
        for g, x in zip(got if k == "feats" else [got], w if k == "feats" else [w]):
            assert g.device.type == "cuda" and tuple(g.shape) == x.shape, (what, k)
            assert np.array_equal(g.cpu().numpy(), x) and g.cpu().numpy().dtype == x.dtype, (what, k)


def _to_device(want, video_ids_as_list=False):
    out = {k: ([torch.from_numpy(f).to(DEV) for f in v] if k == "feats" else torch.from_numpy(v).to(DEV)) for k, v in want.items()}
    if video_ids_as_list:
        out["video_ids"] = want["video_ids"].tolist()
    return out


def test_a_training_epoch_is_the_reference_s():
    store = _store()
    _, names, captions, _ = _corpus()
    items = R.infoset(captions, names, "train")
    n = len(items)
    assert store.n_items("train") == n == 120 and n % BATCH != 0
    seen, ptrs, vids = [], [], []
    order = R.epoch_order(n, "train", seed=9, epoch=2)
    loader = store.loader(mode="train", batch_size=BATCH, epoch=2, seed=9, depth=2)
    assert len(loader) == 8
    for k, batch in enumerate(loader):
        pos = order[k * BATCH: (k + 1) * BATCH]
        _assert_same(batch, _host(pos, "train", 2, 9), k)
        seen += list(zip(batch["video_ids"].tolist(), batch["caption_ids"].tolist()))
        vids.append(batch["video_ids"].clone())
        ptrs.append([t.data_ptr() for t in batch["feats"]] + [batch[key].data_ptr() for key in sorted(batch) if key != "feats"])
    assert k == 7 and len(pos) == n - 7 * BATCH == 8, "the last batch is short"
    assert sorted(seen) == sorted(items) and len(set(seen)) == n, "every item exactly once"
    assert seen != items, "shuffled"
    for k in range(6):                                     # the ring: period `depth`, and two slots that differ
        assert ptrs[k] == ptrs[k + 2] and all(a != b for a, b in zip(ptrs[k], ptrs[k + 1]))
    # another epoch: another permutation and other frames, the same ring
    other = list(store.loader(mode="train", batch_size=BATCH, epoch=3, seed=9, depth=2))[-1]
    assert [t.data_ptr() for t in other["feats"]] == ptrs[7][:4]
    _assert_same(other, _host(R.epoch_order(n, "train", 9, 3)[7 * BATCH:], "train", 3, 9), "epoch 3")
    assert R.epoch_order(n, "train", 9, 3) != order
    # shard = (rank, world): every world-th batch
    for rank in (0, 1, 2):
        part = [b["video_ids"].clone() for b in store.loader(mode="train", batch_size=BATCH, epoch=2, seed=9, depth=2, shard=(rank, 3))]
        assert len(part) == len(vids[rank::3]) and all(torch.equal(a, b) for a, b in zip(part, vids[rank::3]))
    # an item has the same frames in a batch of another size at another place
    a = store.batch([order[20], order[3]], mode="train", epoch=2, seed=9)
    _assert_same(a, _host([order[20], order[3]], "train", 2, 9), "batch()")


def test_validation_batches_16_bit_tables_a_caption_subset_and_all_random():
    store = _store()
    batches = list(store.loader(mode="validate", batch_size=BATCH, depth=3))       # depth 3 = the number of batches: all alive
    assert [b["video_ids"].shape[0] for b in batches] == [16, 16, 8]
    for k, b in enumerate(batches):
        want = _host(list(range(k * BATCH, min(N_VIDEOS, (k + 1) * BATCH))), "validate", 0, 0)
        _assert_same(b, want, k)
        assert b["caption_ids"].tolist() == [0] * len(b["caption_ids"])
    assert not batches[0]["feats"][1][7].any() and batches[0]["feats"][0][7].any()  # the video missing from `m`
    # bf16 tables: rounded once at ingestion, then copied
    _, _, _, tables = _corpus()
    s16 = _store(torch.bfloat16)
    got = s16.batch([3, 50, 119], mode="train", epoch=1, seed=4)
    want = _host([3, 50, 119], "train", 1, 4, tables=[torch.from_numpy(t).to(torch.bfloat16).view(torch.int16).numpy() for t in tables])
    for g, w in zip(got["feats"], want["feats"]):
        assert g.dtype == torch.bfloat16 and np.array_equal(g.view(torch.int16).cpu().numpy(), w)
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    # two captions a video at the most, frames by all_random
    sub = _store(n_caps_per_video=2, seed=5, random_type="all_random")
    _, names, captions, _ = _corpus()
    items = R.infoset(captions, names, "train", 2, seed=5)
    assert sub.n_items("train") == len(items) == 72
    pos = [0, 71, 33, 33, 8]
    _assert_same(sub.batch(pos, mode="train", epoch=6, seed=1), _host(pos, "train", 6, 1, items=items, random_type="all_random"), "subset")
    # a store without captions serves features alone, by video
    from care_amd import ClipStore
    dbs, names, _, _ = _corpus()
    bare = ClipStore(_opt(modality="ai"), {"a": dbs["a"], "i": dbs["i"]}, names, device=DEV)
    b = bare.batch([5, 0, 39], mode="test")
    assert sorted(b) == ["feats", "frame_ids", "video_ids"] and b["video_ids"].tolist() == [5, 0, 39]
    ids = R.frame_ids(0, 60, 28, "equally_sampling")
    assert np.array_equal(b["feats"][1].cpu().numpy(), tables[2][[5, 0, 39]][:, ids])
    with pytest.raises(IndexError):
        bare.batch([40])


def _fresh_model(opt):
    from care_amd import get_framework

    torch.manual_seed(11)
    return get_framework(opt).to(DEV).train()


def test_interplay_step_on_a_loader_batch():
    from care_amd import InterplayStep

    store, opt = _store(), _opt()
    order = R.epoch_order(120, "train", seed=2, epoch=0)
    losses = []
    for source in ("store", "host"):
        if source == "store":
            batch = next(iter(store.loader(mode="train", batch_size=8, epoch=0, seed=2)))
        else:
            batch = _to_device(_host(order[:8], "train", 0, 2))
        model = _fresh_model(opt)
        torch.manual_seed(12)
        step = InterplayStep(opt, model)
        loss = step.training_step(batch)
        losses.append([loss.detach().cpu()] + [step.last[k].cpu() for k in ("captioning_loss", "distillation_loss", "total_loss")])
        del step, model
    print("interplay losses", [float(x) for x in losses[0]])
    assert all(torch.isfinite(x) for x in losses[0]) and float(losses[0][1]) > 0
    for a, b in zip(*losses):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _refs():
    _, names, captions, _ = _corpus()
    return [[c[1:] for c in captions[v]] for v in names]      # the bank lists its references in the store's video order


def test_self_critical_step_on_a_loader_batch():
    from care_amd import CiderBank, SelfCriticalStep

    store, opt = _store(), _opt()
    order = R.epoch_order(120, "train", seed=2, epoch=1)
    bank = CiderBank(_refs(), opt["vocab_size"], with_eos=True, device=DEV)
    losses = []
    for source in ("store", "host"):
        if source == "store":
            batch = next(iter(store.loader(mode="train", batch_size=4, epoch=1, seed=2)))
        else:
            batch = _to_device(_host(order[:4], "train", 1, 2), video_ids_as_list=True)
        model = _fresh_model(opt)
        step = SelfCriticalStep(opt, model, bank, n_samples=2, baseline="greedy", top_k=3,
                                optimizer=torch.optim.SGD(model.parameters(), lr=1e-3))
        loss = step.training_step(batch, seed=17)
        losses.append([loss.detach().cpu(), step.last["mean_reward"].cpu(), step.last["reward"].cpu(), step.last["tokens"].cpu()])
        del step, model
    print("scst loss", float(losses[0][0]), "mean reward", float(losses[0][1]))
    assert torch.isfinite(losses[0][0])
    for a, b in zip(*losses):
        assert torch.equal(a, b) and a.dtype == b.dtype
    assert torch.equal(losses[0][0].view(torch.int32), losses[1][0].view(torch.int32))


def test_validation_epoch_over_the_store_s_loader():
    from care_amd import MetricBank, ValidationEpoch

    store, opt = _store(), _opt()
    bank = MetricBank(_refs(), opt["vocab_size"], with_eos=True, device=DEV)
    model = _fresh_model(opt)
    epoch = ValidationEpoch(opt, model, bank, beam_size=1)
    got = epoch.run(store.loader(mode="validate", batch_size=BATCH, depth=2))      # three batches through two slots
    host = [_to_device(_host(list(range(lo, min(N_VIDEOS, lo + BATCH))), "validate", 0, 0), video_ids_as_list=True)
            for lo in range(0, N_VIDEOS, BATCH)]
    want = epoch.run(host)
    print("validation", got)
    assert got["n_captions"] == float(N_VIDEOS) and got["n_invalid"] == 0.0
    assert got == want

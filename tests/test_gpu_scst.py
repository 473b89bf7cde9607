"""GPU: one self-critical training step (care_amd/scst.py) on the smallest golden model of the training tests, 2 clips, n_samples
2 and 3, fp32 mode, dropout off: the rewards against the float64 reference on the tokens the step sampled, the teacher-forcing
batch against a host construction, the per-caption log-probabilities against the sampler's own score, the loss against the
float64 formula and every parameter's gradient against torch autograd of the float64-restated loss on the oracle's forward.

Measured on one MI355X (greedy, n = 2 / mean, n = 3): rewards 0.02 .. 0.43, all captions 29 tokens; worst gradient deviation 1.1e-6 /
1.2e-6 of the tensor's largest gradient (bar 1e-4 + 2e-5); sum logp against the sampler's score 1.1e-6 / 1.6e-6 per token (bar
1e-4); the loss at 0.75 / 0.80 of the yardstick rule's bar.  The whole file: 6 s."""
import gc

import numpy as np
import pytest
import torch

import cider_reference as C
from conftest import GoldenCase
from test_gpu_backward_kernels import DEV, _check, _Worst

pytestmark = pytest.mark.gpu

NAME = "msrvtt_base_ami_b2"
NO_DROP = dict(encoder_dropout_prob=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
SAMPLER = dict(temperature=1.0, top_k=3, top_p=1.0)   # the fixture's logits are nearly flat: three tokens a step give captions that share n-grams
BAR = 2e-6                                            # the kernel bar of tests/test_gpu_reward_kernels.py
_state = {}


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    """(tests/test_gpu_interplay_step.py: modules, optimisers and engines are collected right behind the test that built them)"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _model():
    from care_amd import get_framework

    opt, P, feats, _ = GoldenCase(NAME).build()
    opt.update(NO_DROP)
    model = get_framework(opt)
    model.load_state_dict(P, strict=True)
    return opt, P, feats, model.to(DEV).train()


def _refs():
    """The corpus: per clip four captions the model itself samples (another seed than the step's) - so that the step's samples
    earn rewards that differ - and three videos of random captions that only make the corpus larger.  Built once."""
    if "refs" not in _state:
        opt, P, feats, model = _model()
        model.eval()
        with torch.no_grad(), model.engine().lock:
            out = model.engine().translate_sample([f.to(DEV) for f in feats], 4, seed=100, use_graph=False, **SAMPLER)
            fed, length = out[1].cpu().numpy(), out[2].cpu().numpy()
        refs = [[fed[c * 4 + j, 1: length[c * 4 + j] + 1].tolist() for j in range(4)] for c in range(len(feats[0]))]
        rng = np.random.RandomState(1)
        refs += [[rng.randint(6, opt["vocab_size"], size=rng.randint(3, 12)).tolist() + [C.EOS] for _ in range(3)] for _ in range(3)]
        _state["refs"] = refs
    return _state["refs"]


def _step(baseline, n, bank=None, with_eos=False):
    from care_amd import CiderBank, SelfCriticalStep

    opt, P, feats, model = _model()
    bank = bank or CiderBank(_refs(), opt["vocab_size"], with_eos=with_eos, device=DEV)
    step = SelfCriticalStep(opt, model, bank, n_samples=n, baseline=baseline, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3),
                            **SAMPLER)
    batch = {"feats": [f.to(DEV) for f in feats], "video_ids": list(range(len(feats[0])))}
    return opt, P, feats, model, step, batch


def _loss64(logits, labels, adv, dt=torch.float64):
    live = labels > 0
    logp = torch.log_softmax(logits.to(dt), dim=-1).gather(2, labels.unsqueeze(-1)).squeeze(-1)
    logp = torch.where(live, logp, torch.zeros((), dtype=dt))
    return -(adv.to(dt).view(-1, 1) * logp).sum() / live.sum().clamp_min(1).to(dt), logp.sum(dim=1)


@pytest.mark.parametrize("baseline,n,with_eos", [("greedy", 2, False), ("mean", 3, True)])
def test_one_training_step(baseline, n, with_eos):
    from oracle import care_cpu
    from care_amd import self_critical_loss
    from care_amd.constants import BOS, EOS, PAD

    opt, P, feats, model, step, batch = _step(baseline, n, with_eos=with_eos)
    B, T, V = len(feats[0]), opt["max_len"] - 1, opt["vocab_size"]
    before = [p.detach().clone() for p in model.parameters()]
    loss = step.training_step(batch, seed=17)
    last = step.last
    assert model.training and loss.requires_grad and torch.equal(loss.detach(), last["loss"])
    for k in ("loss", "mean_reward", "mean_baseline"):
        assert last[k].device.type == "cuda" and last[k].dim() == 0 and not last[k].requires_grad, k
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters())), "the optimiser must have moved the model"
    fed, length = last["tokens"].cpu().numpy(), last["length"].cpu().numpy()
    N = B * n
    assert fed.shape == (N, T + 1) and (fed[:, 0] == BOS).all() and (length >= 1).all()

    # 1. the rewards: the float64 reference on the tokens and lengths the step used
    corpus = C.Corpus(_refs(), with_eos=with_eos)
    want = np.array(corpus.scores(fed[:, 1:].tolist(), length.tolist(), [r // n for r in range(N)])).reshape(B, n)
    reward = last["reward"].cpu().double().numpy()
    print(baseline, "rewards", reward.tolist(), "lengths", length.tolist())
    assert np.abs(reward - want).max() <= BAR
    assert reward.max() > 0.1 and np.ptp(reward, axis=1).max() > 0.01, "the samples of a clip must earn different rewards"
    if baseline == "greedy":
        gfed, glen = last["greedy_tokens"].cpu().numpy(), last["greedy_length"].cpu().numpy()
        base = np.array(corpus.scores(gfed[:, 1:].tolist(), glen.tolist(), list(range(B)))).reshape(B, 1).repeat(n, axis=1)
    else:
        base = (want.sum(axis=1, keepdims=True) - want) / (n - 1)
    assert abs(float(last["mean_reward"]) - want.mean()) <= BAR and abs(float(last["mean_baseline"]) - base.mean()) <= BAR
    adv = last["advantages"].cpu()
    assert np.abs(adv.double().numpy() - (want - base)).max() <= 2 * BAR and float(adv.abs().max()) > 0.01

    # 2. the teacher-forcing batch: a host construction from fed / length; nothing follows a caption's end but PAD
    ids, labels = last["input_ids"].cpu(), last["labels"].cpu()
    want_ids, want_labels = torch.full((N, T), PAD, dtype=torch.long), torch.full((N, T), PAD, dtype=torch.long)
    for r in range(N):
        L = int(length[r])
        want_ids[r, :L] = torch.from_numpy(fed[r, :L].astype(np.int64))
        want_labels[r, :L] = torch.from_numpy(fed[r, 1: L + 1].astype(np.int64))
        toks = fed[r, 1: L + 1].tolist()
        assert EOS not in toks[:-1] and (toks[-1] == EOS or L == T)
    assert torch.equal(ids, want_ids) and torch.equal(labels, want_labels)
    assert bool(((labels == EOS).sum(dim=1) <= 1).all()) and bool((labels[ids == PAD] == PAD).all())

    # 3. the loss on the step's own logits, labels and advantages: the float64 formula under the yardstick rule
    worst = _Worst("training_step " + baseline)
    logits = last["logits"].cpu()
    assert logits.shape == (N, T, V)
    loss64, _ = _loss64(logits, labels, adv.view(-1))
    loss32, _ = _loss64(logits, labels, adv.view(-1), torch.float32)
    _check(worst, "loss", last["loss"], loss64, loss32)

    # 4. every parameter's gradient: torch autograd of the float64-restated loss on the oracle's training forward
    Pc = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in P.items()}
    ref = care_cpu.feedforward_step(Pc, opt, [f.repeat_interleave(n, dim=0) for f in feats], ids)
    assert (logits - ref["logits"].detach()).abs().max().item() < 2e-4
    _loss64(ref["logits"], labels, adv.view(-1))[0].backward()
    checked, worst_grad = 0, ("", 0.0)
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        gref = Pc[k].grad
        if gref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, "no gradient for " + k
        if k == "decoder.embedding.word_embeddings.weight":
            gref = gref.clone()
            gref[0] = 0.0   # nn.Embedding(padding_idx=PAD): no gradient for the PAD row (tests/test_gpu_training.py)
        scale, diff = float(gref.abs().max()), float((p.grad.cpu() - gref).abs().max())
        worst_grad = max(worst_grad, (k, diff / max(scale, 1e-3)), key=lambda kv: kv[1])
        assert diff < 1e-4 * scale + 2e-5, (k, diff, scale)
        checked += 1
    assert checked >= 20, checked
    print("worst relative gradient error", worst_grad)

    # 5. the model in eval mode: the per-caption sum of log-probabilities of the loss forward is the sampler's own score
    fresh = _model()[3].eval()
    with torch.no_grad():
        out = fresh.feedforward_step({"feats": [f.repeat_interleave(n, dim=0) for f in batch["feats"]], "input_ids": last["input_ids"]},
                                     output_auxiliary=False)
        _, seq_logp, totals = self_critical_loss(out["logits"], last["labels"], last["advantages"].view(-1), return_aux=True)
    err = np.abs(seq_logp.cpu().double().numpy() - last["score"].cpu().double().numpy()) / length
    print("per-token deviation of sum logp from translate_sample's score", err.max())
    assert err.max() <= 1e-4 and float(totals[1]) == float(length.sum())
    worst.report()


def test_zero_advantages_give_a_zero_gradient_in_every_parameter():
    """A corpus of ONE video has ln N = 0: every reward, every baseline and every advantage is exactly 0."""
    from care_amd import CiderBank

    opt = GoldenCase(NAME).build()[0]
    bank = CiderBank([_refs()[0]], opt["vocab_size"], device=DEV)
    for baseline, n in (("greedy", 2), ("mean", 2)):
        opt, P, feats, model, step, batch = _step(baseline, n, bank=bank)
        batch["video_ids"] = [0] * len(feats[0])
        before = [p.detach().clone() for p in model.parameters()]
        loss = step.training_step(batch, seed=3)
        assert float(loss.detach()) == 0.0 and float(step.last["mean_reward"]) == 0.0 and float(step.last["mean_baseline"]) == 0.0
        assert bool((step.last["advantages"] == 0).all())
        grads = [p.grad for p in model.parameters() if p.requires_grad]
        assert len(grads) >= 20 and all(g is not None and bool((g == 0).all()) for g in grads)
        assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


def test_refusals_by_name_and_the_mode_is_restored():
    opt, P, feats, model, step, batch = _step("greedy", 2)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(KeyError, match="video_ids"):
        step.training_step({"feats": batch["feats"]})
    with pytest.raises(ValueError, match="video_ids"):
        step.training_step({"feats": batch["feats"], "video_ids": [0]})
    model.set_fused_head(True)
    with pytest.raises(NotImplementedError, match="fused head"):
        step.training_step(batch)
    model.set_fused_head(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.training_step({"feats": [f.cpu() for f in batch["feats"]], "video_ids": batch["video_ids"]})
    assert model.training and all(torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    model.eval()
    assert torch.isfinite(step.training_step(batch, seed=5).detach()) and not model.training, "the caller's mode comes back"

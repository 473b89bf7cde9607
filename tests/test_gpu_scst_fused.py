"""GPU: the self-critical training step with the fused head (care_amd/scst.py, SelfCriticalStep(fused_head=True)) against the
unfused step on the smallest golden model of the training tests - tests/test_gpu_scst.py's fixture, sampler settings, corpus and
reference construction; dropout off, SGD, both runs under set_train_gemm("fp16x3"), the arithmetic the fused head always uses.

Two training steps in a row, fused and unfused, from the same weights and seeds: tokens, lengths, rewards and advantages bit for
bit, the fused loss under the yardstick rule of tests/test_gpu_backward_kernels.py (float64: the oracle's forward on the float64
weights the step started from, labels rebuilt from last["tokens"]; yardstick: the unfused step's loss), every parameter's
gradient within 1e-4 x scale + 2e-5 of the unfused step's, seq_logp within 1e-4 per token of the sampler's own score."""
import gc

import numpy as np
import pytest
import torch

from conftest import GoldenCase
from test_gpu_backward_kernels import DEV, _check, _Worst
from test_gpu_scst import NAME, SAMPLER, _loss64, _model, _refs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_nothing_to_the_collector():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _step(baseline, n, fused, bank=None, with_eos=False, module_flag=False):
    from care_amd import CiderBank, SelfCriticalStep

    opt, P, feats, model = _model()
    model.set_fused_head(module_flag)
    bank = bank or CiderBank(_refs(), opt["vocab_size"], with_eos=with_eos, device=DEV)
    step = SelfCriticalStep(opt, model, bank, n_samples=n, baseline=baseline, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3),
                            fused_head=fused, **SAMPLER)
    batch = {"feats": [f.to(DEV) for f in feats], "video_ids": list(range(len(feats[0])))}
    return opt, P, feats, model, step, batch


def _labels_of(fed, length, T):
    """input_ids and labels rebuilt on the host from the step's tokens, as tests/test_gpu_scst.py does."""
    N = fed.shape[0]
    ids, labels = torch.zeros(N, T, dtype=torch.long), torch.zeros(N, T, dtype=torch.long)
    for r in range(N):
        L = int(length[r])
        ids[r, :L] = torch.from_numpy(fed[r, :L].astype(np.int64))
        labels[r, :L] = torch.from_numpy(fed[r, 1: L + 1].astype(np.int64))
    return ids, labels


@pytest.mark.parametrize("baseline,n,with_eos", [("greedy", 2, False), ("mean", 3, True)])
def test_fused_against_unfused_step_by_step(baseline, n, with_eos):
    from oracle import care_cpu
    from care_amd import training

    opt, P, feats, model_u, step_u, batch = _step(baseline, n, False, with_eos=with_eos)
    _, _, _, model_f, step_f, _ = _step(baseline, n, True, bank=step_u.bank, with_eos=with_eos)
    T = opt["max_len"] - 1
    worst = _Worst("fused step " + baseline)
    training.set_train_gemm("fp16x3")
    try:
        for it, seed in enumerate((17, 18)):
            start = {k: v.detach().cpu().clone() for k, v in model_f.state_dict().items()}
            loss_u = step_u.training_step(batch, seed=seed)
            loss_f = step_f.training_step(batch, seed=seed)
            lu, lf = step_u.last, step_f.last
            assert model_f.training and model_f.fused_head is False and loss_f.requires_grad and torch.equal(loss_f.detach(), lf["loss"])
            for k in ("tokens", "length", "reward", "advantages", "input_ids", "labels"):
                assert torch.equal(lu[k], lf[k]), (it, k)
            assert "logits" in lu and "logits" not in lf and "seq_logp" in lf and "seq_logp" not in lu
            assert float(lf["advantages"].abs().max()) > 0.01

            # the loss in float64: the oracle's forward on the float64 weights this step started from, labels from the tokens
            fed, length = lf["tokens"].cpu().numpy(), lf["length"].cpu().numpy()
            ids, labels = _labels_of(fed, length, T)
            assert torch.equal(labels, lf["labels"].cpu())
            P64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in start.items()}
            with torch.no_grad():
                ref = care_cpu.feedforward_step(P64, opt, [f.double().repeat_interleave(n, dim=0) for f in feats], ids)
                assert ref["logits"].dtype == torch.float64
                loss64, seq64 = _loss64(ref["logits"], labels, lf["advantages"].cpu().view(-1))
            _check(worst, "loss, step {}".format(it), lf["loss"], loss64, lu["loss"])

            # the per-caption log-probabilities: the sampler's own score (and the float64 sums)
            err = np.abs(lf["seq_logp"].cpu().double().numpy() - lf["score"].cpu().double().numpy()) / length
            print(baseline, "step", it, "per-token deviation of seq_logp from translate_sample's score", err.max())
            assert lf["seq_logp"].shape == (len(length),) and err.max() <= 1e-4
            assert float((lf["seq_logp"].cpu().double() - seq64).abs().max()) <= 1e-4 * length.max()

            # every parameter's gradient: the unfused step's
            checked, worst_grad = 0, ("", 0.0)
            for (k, pu), (kf, pf) in zip(model_u.named_parameters(), model_f.named_parameters()):
                assert k == kf
                if not pu.requires_grad or pu.grad is None:
                    assert pf.grad is None or float(pf.grad.abs().max()) == 0.0, k
                    continue
                assert pf.grad is not None, "no gradient for " + k
                scale, diff = float(pu.grad.abs().max()), float((pf.grad - pu.grad).abs().max())
                worst_grad = max(worst_grad, (k, diff / max(scale, 1e-3)), key=lambda kv: kv[1])
                assert diff < 1e-4 * scale + 2e-5, (it, k, diff, scale)
                checked += 1
            assert checked >= 20, checked
            print(baseline, "step", it, "worst relative gradient deviation from the unfused step", worst_grad)
    finally:
        training.set_train_gemm("auto")
    worst.report()


def test_zero_advantages_give_a_zero_gradient_in_every_parameter():
    """A corpus of ONE video has ln N = 0: every reward, every baseline and every advantage is exactly 0."""
    from care_amd import CiderBank

    opt = GoldenCase(NAME).build()[0]
    bank = CiderBank([_refs()[0]], opt["vocab_size"], device=DEV)
    for baseline, n in (("greedy", 2), ("mean", 2)):
        opt, P, feats, model, step, batch = _step(baseline, n, True, bank=bank)
        batch["video_ids"] = [0] * len(feats[0])
        before = [p.detach().clone() for p in model.parameters()]
        loss = step.training_step(batch, seed=3)
        assert float(loss.detach()) == 0.0 and float(step.last["mean_reward"]) == 0.0 and float(step.last["mean_baseline"]) == 0.0
        assert bool((step.last["advantages"] == 0).all())
        grads = [p.grad for p in model.parameters() if p.requires_grad]
        assert len(grads) >= 20 and all(g is not None and bool((g == 0).all()) for g in grads)
        assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


@pytest.mark.parametrize("module_flag", [False, True])
def test_the_flag_and_the_mode_come_back(module_flag):
    """The module's own fused_head flag and its training mode are the caller's again after a good step and after a step that
    raises - before anything ran (no video_ids) and inside the decodes (a video_ids list of the wrong length)."""
    opt, P, feats, model, step, batch = _step("greedy", 2, True, module_flag=module_flag)
    assert model.fused_head is module_flag
    for training_mode in (True, False):
        model.train(training_mode)
        assert torch.isfinite(step.training_step(batch, seed=5).detach())
        assert model.fused_head is module_flag and model.training is training_mode
        assert "seq_logp" in step.last and "logits" not in step.last
        with pytest.raises(KeyError, match="video_ids"):
            step.training_step({"feats": batch["feats"]})
        assert model.fused_head is module_flag and model.training is training_mode
        with pytest.raises(ValueError, match="video_ids"):
            step.training_step({"feats": batch["feats"], "video_ids": [0]})
        assert model.fused_head is module_flag and model.training is training_mode
    # the module's forward itself still follows its own flag
    model.train()
    from care_amd.criterion import DeferredLogits
    out = model({"feats": batch["feats"], "input_ids": step.last["input_ids"][:len(feats[0])]})["logits"]
    assert isinstance(out, DeferredLogits) is module_flag

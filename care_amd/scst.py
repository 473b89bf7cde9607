"""Self-critical sequence training on the MI355X: a training step on the CIDEr-D of the model's own sampled captions.

    from care_amd.scst import SelfCriticalStep
    step = SelfCriticalStep(opt, captioner, bank, n_samples=5, baseline="greedy")
    loss = step.training_step(batch)          # batch: feats, video_ids

One step: sample n captions per clip (HipEngine.translate_sample, eval mode, no gradient), score them against the clip's
references (CiderBank.score, csrc/reward.hip), subtract a baseline - the reward of the greedy caption, or the mean reward of the
clip's other samples - teacher-force the samples through the training forward and minimise the advantage-weighted
log-likelihood (care_amd.reward.self_critical_loss).  The sampled tokens, their lengths, the rewards, the advantages and the
number of live label positions stay on the device from the first launch to the optimiser step: the host reads nothing of
them, `last` holds device scalars, and reading one is the caller's synchronisation.

`fused_head=True` runs the teacher-forced pass with the vocabulary head inside the loss
(care_amd.reward.self_critical_head_loss): head, loss and backward over the live label positions only, the
[N, t, V] logits and their gradient never in memory.  The unfused step stays free of result reads; the fused one has a single
one - the number of live label positions, 4 bytes, counted on the device and copied to pinned memory without blocking
BEFORE the teacher-forced forward is enqueued, and waited for only when the loss is reached: the read overlaps the forward.

What it does not do: ensembles, a cross-entropy term mixed into the step, and the exchange of gradients between devices.
"""
import torch

from .constants import PAD
from .criterion import DeferredLogits
from .reward import CiderBank, reward_advantage, self_critical_head_loss, self_critical_loss

__all__ = ["SelfCriticalStep", "sample_to_labels"]

BASELINES = ("greedy", "mean")


def sample_to_labels(fed: torch.Tensor, length: torch.Tensor, t: int):
    """The teacher-forcing batch of decoded captions: fed int32 [N, >= t + 1] (column 0 = BOS), length int32 [N] (tokens behind
    BOS, the EOS included) -> input_ids, labels int64 [N, t]: input_ids[r, j] = fed[r, j] and labels[r, j] = fed[r, j + 1] for
    j < length[r], PAD behind (what a frozen row went on drawing is cut here).  Elementwise on the device; `length` is not
    read on the host."""
    live = torch.arange(t, device=fed.device).view(1, t) < length.view(-1, 1)
    pad = torch.full((), PAD, dtype=torch.int64, device=fed.device)
    ids = fed[:, : t + 1].to(torch.int64)
    return torch.where(live, ids[:, :t], pad), torch.where(live, ids[:, 1: t + 1], pad)


class SelfCriticalStep(object):
    """A `captioner`, a `CiderBank` of its training captions, the optimiser and its scheduler (built from `opt` by
    care_amd.optim.configure_optimizers unless given, as InterplayStep does).

    baseline "greedy": advantage = reward - reward of the clip's greedy caption (one more decode per step);
    baseline "mean":   advantage = reward - mean reward of the clip's other n_samples - 1 samples.

    fused_head False (the default): the loss over the [N, t, V] logits; a captioner with set_fused_head(True) is refused.
    fused_head True: the captioner is accepted whatever its own flag says; the step turns the module's fused head on for the
    teacher-forced pass only (the caller's value comes back in a `finally`) and takes the loss with the head inside -
    `last` then holds `seq_logp` (each caption's sum of log-probabilities) and no `logits`.  The unfused step reads no
    result on the host; the fused one reads the live count - 4 bytes, once, overlapped with the forward."""

    def __init__(self, opt, captioner, bank, n_samples=5, baseline="greedy", temperature=1.0, top_k=0, top_p=1.0, optimizer=None,
                 scheduler=None, with_eos=None, fused_head=False):
        from .engine_sample import check_sample_args
        from .optim import configure_optimizers

        if isinstance(captioner, (list, tuple)):
            raise NotImplementedError("an ensemble of {} captioners: self-critical training takes ONE model".format(len(captioner)))
        if not isinstance(bank, CiderBank):
            raise TypeError("`bank` must be a care_amd.CiderBank, got {}".format(type(bank).__name__))
        if baseline not in BASELINES:
            raise ValueError("`baseline` must be one of {}, got {!r}".format(BASELINES, baseline))
        check_sample_args(n_samples, temperature, top_k, top_p)   # n_samples < 1 and the sampler's settings, by name
        if baseline == "mean" and n_samples < 2:
            raise ValueError('baseline="mean" is the mean of a clip\'s OTHER samples: `n_samples` must be >= 2, got {}'.format(n_samples))
        if with_eos is not None and bool(with_eos) != bank.with_eos:
            raise ValueError("`with_eos` = {} but the bank was built with with_eos = {}: candidates and references must "
                             "treat EOS alike".format(bool(with_eos), bank.with_eos))
        self.fused_head = bool(fused_head)
        if not self.fused_head:
            self._refuse_fused_head(captioner)
        self.opt, self.captioner, self.bank = opt, captioner, bank
        self.n_samples, self.baseline = n_samples, baseline
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        if optimizer is None:
            built = configure_optimizers(opt, captioner)
            optimizer = built["optimizer"]
            if scheduler is None:
                scheduler = built["lr_scheduler"]["scheduler"]
        self.optimizer, self.scheduler = optimizer, scheduler
        self.last = {}

    @staticmethod
    def _refuse_fused_head(captioner) -> None:
        if getattr(captioner, "fused_head", False):
            raise NotImplementedError(
                "the captioner runs the fused head (set_fused_head(True)), which never materialises the [N, t, V] logits the "
                "self-critical loss is taken over - call set_fused_head(False) on the module")

    def _baseline_reward(self, engine, feats, video):
        """fp32 [B]: the reward of each clip's greedy caption (baseline "greedy"), with the caption's tokens and length."""
        _, fed, length, _ = engine.translate_greedy(feats, use_graph=False, early_exit=False)
        fed, length = fed.clone(), length.clone()
        return self.bank.score(fed[:, 1: self._T + 1], length, video), fed, length

    def training_step(self, batch, seed=None, current_epoch=0):
        """Returns the loss; `last` holds loss, mean_reward and mean_baseline as detached device scalars, and the device tensors
        the step worked on (tokens, length, reward, advantages, input_ids, labels, logits - with fused_head: seq_logp
        instead of logits -; greedy_tokens / greedy_length with the greedy baseline).  seed None: one from torch's generator."""
        if "video_ids" not in batch:
            raise KeyError("the batch has no `video_ids`: the reward is taken against each clip's own references")
        model, n = self.captioner, self.n_samples
        if not self.fused_head:
            self._refuse_fused_head(model)
        feats = list(batch["feats"])
        if any(f.device.type != "cuda" for f in feats):
            raise RuntimeError("the features are on the CPU: self-critical training runs on the MI355X (no CPU fallback)")
        B = feats[0].shape[0]
        T = self._T = int(self.opt["max_len"]) - 1
        was_training = model.training
        greedy = {}
        model.eval()   # (the decodes run on the inference engine, which re-packs the weights the last step moved)
        try:
            with torch.no_grad(), model._on_device():
                engine = model.engine()
                with engine.lock:
                    video = self.bank.rows(batch["video_ids"])
                    if video.numel() != B:
                        raise ValueError("{} `video_ids` for {} clips".format(video.numel(), B))
                    _, fed, length, score, _ = engine.translate_sample(feats, n, self.temperature, self.top_k, self.top_p, seed=seed,
                                                                       use_graph=False)
                    fed, length, score = fed.clone(), length.clone(), score.clone()   # (workspaces of the engine)
                    reward = self.bank.score(fed[:, 1: T + 1], length, video.repeat_interleave(n)).view(B, n)
                    base = None
                    if self.baseline == "greedy":
                        base, greedy["greedy_tokens"], greedy["greedy_length"] = self._baseline_reward(engine, feats, video)
                    adv, stats = reward_advantage(reward, base)
        except BaseException:
            model.train(was_training)
            raise
        model.train()   # the teacher-forced pass is the TRAINING forward (autograd, dropout as configured)
        input_ids, labels = sample_to_labels(fed, length, T)
        tf_batch = {k: v for k, v in batch.items() if k not in ("feats", "input_ids", "labels", "video_ids")}
        for k, v in tf_batch.items():   # per-clip tensors of the batch (concept labels, retrieval rows) follow their clip
            if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B:
                tf_batch[k] = v.repeat_interleave(n, dim=0)
        tf_batch["feats"] = [f.repeat_interleave(n, dim=0) for f in feats]
        tf_batch["input_ids"], tf_batch["labels"] = input_ids, labels
        try:
            if self.fused_head:
                loss, out = self._fused_loss(model, tf_batch, labels, adv, current_epoch)
            else:
                results = model(tf_batch, current_epoch=current_epoch)
                loss = self_critical_loss(results["logits"], labels, adv.view(-1))
                out = {"logits": results["logits"].detach()}
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
        finally:
            model.train(was_training)
        self.last = {"loss": loss.detach(), "mean_reward": stats[0], "mean_baseline": stats[1],
                     "tokens": fed, "length": length, "score": score, "reward": reward, "advantages": adv,
                     "input_ids": input_ids, "labels": labels, **out, **greedy}
        return loss

    def _fused_loss(self, model, tf_batch, labels, adv, current_epoch):
        """The teacher-forced pass with the module's fused head on and the loss with the head inside.  The live count leaves
        for pinned memory before the forward is enqueued and is waited for behind it: the step's one result read."""
        V = int(self.opt["vocab_size"])
        count = ((labels > 0) & (labels < V)).sum().to(torch.int32)
        host = torch.empty((), dtype=torch.int32, pin_memory=True)
        host.copy_(count, non_blocking=True)
        arrived = torch.cuda.Event()
        arrived.record(torch.cuda.current_stream(labels.device))
        was_fused = bool(getattr(model, "fused_head", False))
        model.set_fused_head(True)
        try:
            results = model(tf_batch, current_epoch=current_epoch)
        finally:
            model.set_fused_head(was_fused)
        deferred = results["logits"]
        if not isinstance(deferred, DeferredLogits):
            raise RuntimeError("the training forward under set_fused_head(True) returned {} under `logits`, not a "
                               "DeferredLogits".format(type(deferred).__name__))
        if deferred.weight.shape[0] != V:
            raise ValueError("opt['vocab_size'] = {} but the head has {} rows".format(V, deferred.weight.shape[0]))
        arrived.synchronize()
        loss, seq_logp, _ = self_critical_head_loss(deferred.hidden, deferred.weight, labels, adv.view(-1), return_aux=True,
                                                    live=int(host))
        return loss, {"seq_logp": seq_logp}

    def training_epoch_end(self) -> None:
        """The scheduler is stepped by hand, as InterplayStep does (manual optimisation)."""
        if self.scheduler is not None:
            self.scheduler.step()

"""care_amd - MI355X-native captioning forward path of yangbang18/CARE.

Public seam (mirrors the reference's two factories):
    from care_amd import get_framework, get_translator
and, for training, the reference's criteria behind `misc.Crit`'s interface (care_amd/criterion.py):
    from care_amd import get_criterion
and the optimiser step behind `Wrapper.configure_optimizers`' interface (care_amd/optim.py):
    from care_amd import configure_optimizers, Adam
and the mean-teacher step of `--wrapper InterplayModel` (models/Wrapper.py:550-614; care_amd/interplay.py):
    from care_amd import InterplayStep, distillation_mse, ema_update
and the `r` modality retrieved on device from a bank of caption embeddings (pretreatment/clip_retrieval.py; care_amd/retrieval.py):
    from care_amd import CaptionBank, attach_retrieval
and self-critical sequence training on the CIDEr-D of sampled captions (care_amd/reward.py, care_amd/scst.py):
    from care_amd import CiderBank, self_critical_loss, self_critical_head_loss, SelfCriticalStep
(`self_critical_head_loss`, `SelfCriticalStep(..., fused_head=True)`: the vocabulary head inside the loss, no [N, t, V] logits)
and the validation epoch scored on device - corpus BLEU, ROUGE-L and CIDEr over token ids (care_amd/capmetrics.py, care_amd/validation.py):
    from care_amd import MetricBank, ValidationEpoch
and the data set resident in HBM, every training / validation batch built on the device (care_amd/clipstore.py):
    from care_amd import ClipStore
and the test epoch - per-video scores, the predictions and the caption analysis `ave_length` / `novel` / `unique` / `usage`
against the training captions, all kept on the device (care_amd/corpusstats.py, care_amd/testepoch.py):
    from care_amd import CorpusBank, EpochCaptions, TestEpoch
and the consensus among a clip's sampled captions - the candidate that agrees most with the others under CIDEr-D, chosen on
the device (care_amd/consensus.py; Translator_ARFormer.consensus_batch):
    from care_amd import consensus_select
"""
from .framework import get_framework  # noqa: F401
from .translator import get_translator  # noqa: F401
from .criterion import Criterion, LanguageGeneration, NoisyOrMIL, get_criterion  # noqa: F401
from .optim import Adam, configure_optimizers, filter_weight_decay  # noqa: F401
from .interplay import InterplayStep, distillation_mse, ema_update  # noqa: F401
from .retrieval import CaptionBank, attach_retrieval  # noqa: F401
from .reward import CiderBank, self_critical_head_loss, self_critical_loss  # noqa: F401
from .scst import SelfCriticalStep  # noqa: F401
from .capmetrics import MetricBank  # noqa: F401
from .validation import ValidationEpoch  # noqa: F401
from .clipstore import ClipStore  # noqa: F401
from .corpusstats import CorpusBank, EpochCaptions  # noqa: F401
from .testepoch import TestEpoch  # noqa: F401
from .consensus import consensus_select  # noqa: F401

__all__ = ["consensus_select", "CorpusBank", "EpochCaptions", "TestEpoch", "ClipStore", "MetricBank", "ValidationEpoch", "CiderBank", "self_critical_loss", "self_critical_head_loss", "SelfCriticalStep", "get_framework", "get_translator", "get_criterion", "Criterion", "LanguageGeneration", "NoisyOrMIL",
           "Adam", "configure_optimizers", "filter_weight_decay", "InterplayStep", "distillation_mse", "ema_update",
           "CaptionBank", "attach_retrieval"]

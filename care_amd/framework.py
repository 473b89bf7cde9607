"""Drop-in for the reference's `models.Framework.get_framework` (models/Framework.py:14-51).

`get_framework(opt)` returns an nn.Module with the attribute surface the reference's
callers touch (`backbone, encoder, predictor, decoder, cls_head, pointer,
input_keys_for_decoder, opt`; `encoding_phase / prepare_inputs_for_decoder /
decoding_phase / feedforward_step / forward / get_keys_to_device`) and a
`state_dict()` whose keys and shapes equal the reference's, so its checkpoints load with
strict=True.  The sub-modules below are *parameter containers* that reproduce the
reference's parameter naming; the arithmetic is done by `HipEngine` (care_amd/engine.py)
through the C ABI of libcare_hip.so.  There is no eager/CPU fallback: a forward call
without the HIP library or a GPU raises.

Training mode (`model.train()`; models/Wrapper.py:423-435 -> Framework.py:215-237 under autograd): `forward` /
`feedforward_step` route to care_amd/training.py - the same forward with dropout active, as torch.autograd.Functions
whose forward AND backward are HIP kernels (csrc/backward.hip).  The eval-only entry points (`encoding_phase`,
`decoding_phase`, the Translator) raise NotImplementedError in training mode instead of silently running without
dropout; configurations training.py does not cover (other encoders, concept heads without mean pooling + channel
concat, several captions per clip) raise too.
"""
import math
import contextlib
import os
import threading
from typing import Any, Dict, List, Optional

import torch
import torch.nn as nn

from .constants import PAD
from .engine import HipEngine


# --------------------------------------------------------------------------- parameter containers
class _SDPA(nn.Module):
    """Parameters of ScaledDotProductAttention (models/components/Attention.py:11-61)."""

    def __init__(self, d, heads, bias=True, hybrid_length=0):
        super().__init__()
        if hybrid_length:
            self.hybrid_bias = nn.Parameter(torch.zeros(heads, hybrid_length))
        self.query = nn.Linear(d, d, bias=bias)
        self.key = nn.Linear(d, d, bias=bias)
        self.value = nn.Linear(d, d, bias=bias)


class _MHA(nn.Module):
    """Parameters of MultiHeadAttention (models/components/SubLayers.py:11-38)."""

    def __init__(self, opt, hybrid_length=0):
        super().__init__()
        d = opt["dim_hidden"]
        self.SDPA = _SDPA(d, opt["num_attention_heads"], not opt.get("mha_exclude_bias", False), hybrid_length)
        self.dense = nn.Linear(d, d)
        self.LayerNorm = nn.LayerNorm(d, eps=opt["layer_norm_eps"])


class _FFN(nn.Module):
    """Parameters of PositionwiseFeedForward (SubLayers.py:108-135)."""

    def __init__(self, opt):
        super().__init__()
        d, ff = opt["dim_hidden"], opt["intermediate_size"]
        self.dense1 = nn.Linear(d, ff)
        self.dense2 = nn.Linear(ff, d)
        self.LayerNorm = nn.LayerNorm(d, eps=opt["layer_norm_eps"])


class _FixedPE(nn.Module):
    """Sinusoidal table stored as a frozen parameter `pe` (Embeddings.py:11-27)."""

    def __init__(self, max_len, d):
        super().__init__()
        pe = torch.zeros(max_len, d)
        position = torch.arange(0, max_len).float().unsqueeze(1)
        div = (torch.arange(0, d, 2).float() * -(math.log(10000.0) / d)).exp()
        pe[:, 0::2] = torch.sin(position * div)
        pe[:, 1::2] = torch.cos(position * div)
        self.pe = nn.Parameter(pe.unsqueeze(0), requires_grad=False)


def _position_table(opt, n):
    return nn.Embedding(n, opt["dim_hidden"]) if opt.get("trainable_pe", False) else _FixedPE(n, opt["dim_hidden"])


class _EncoderLayer(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.intra_attention = _MHA(opt)
        self.ffn = _FFN(opt)


class _TransformerEncoderBase(nn.Module):
    """Parameters of TransformerEncoderBase (models/Encoder.py:244-262)."""

    def __init__(self, opt):
        super().__init__()
        self.position_embeddings = _position_table(opt, opt["n_frames"])
        self.LayerNorm = nn.LayerNorm(opt["dim_hidden"], eps=opt["layer_norm_eps"])
        self.layers = nn.ModuleList([_EncoderLayer(opt) for _ in range(opt["num_hidden_layers_encoder"])])


class Embedder(nn.Module):
    """MultipleStreams with per-modality Linear->LayerNorm->Dropout (Encoder.py:51-83,165-168)."""

    def __init__(self, opt):
        super().__init__()
        for ch in opt["modality"].lower():
            dim = opt.get("dim_" + ch)
            if dim is None:
                raise AssertionError("The modality is {}, but dim_{} can not be found in opt".format(opt["modality"], ch))
            self.add_module("Encoder_%s" % ch.upper(), self._stream(dim, opt))

    @staticmethod
    def _stream(dim, opt):
        return nn.Sequential(nn.Linear(dim, opt["dim_hidden"]), nn.LayerNorm(opt["dim_hidden"], eps=opt["layer_norm_eps"]),
                             nn.Dropout(opt.get("encoder_dropout_prob", 0.5)))


class MultiTransformerEncoder(Embedder):
    """Per-modality Linear -> TransformerEncoderBase (Encoder.py:190-193)."""

    @staticmethod
    def _stream(dim, opt):
        return nn.Sequential(nn.Linear(dim, opt["dim_hidden"]), _TransformerEncoderBase(opt))


_ENCODERS = {"Embedder": Embedder, "MultiTransformerEncoder": MultiTransformerEncoder}


class Predictor_attribute(nn.Module):
    """Concept-detection head parameters (models/Predictor/pred_attribute.py:49-76)."""

    def __init__(self, opt):
        super().__init__()
        modality = opt.get("modality_for_predictor", None) or opt["modality"]
        if not (opt.get("attribute_prediction_share_prj", False) or len(opt["attribute_prediction_flags"]) == 1):
            raise ValueError("per-flag concept projections are outside the hot path (pred_attribute.py:66-70)")
        n = len(modality) if opt.get("attribute_prediction_channel_concat", False) else 1
        self.prj = nn.Linear(opt["dim_hidden"] * n, opt["attribute_prediction_k"])


class _NaiveEmbeddings(nn.Module):
    def __init__(self, n_words, n_positions, d, eps, padding_idx=None):
        super().__init__()
        self.word_embeddings = nn.Embedding(n_words, d, padding_idx=padding_idx)
        self.position_embeddings = nn.Embedding(n_positions, d)
        self.LayerNorm = nn.LayerNorm(d, eps=eps)


class SemanticContainer(nn.Module):
    """Concept embedding + global guidance parameters (pred_attribute.py:239-261)."""

    def __init__(self, opt):
        super().__init__()
        # pred_attribute.py:243-252: no concept embeddings without local guidance (`use_attr_flags` ..L0; the ablation rows of
        # scripts/exp_ablation_main.sh:34,63 - G1L0 keeps the global guidance `semantic2hidden` alone)
        if "L0" not in opt.get("use_attr_flags", ""):
            self.attr_embs = _NaiveEmbeddings(opt["attribute_prediction_k"], opt["use_attr_topk"], opt["dim_hidden"],
                                              opt["layer_norm_eps"])
        if "emb" in opt.get("use_attr_type", ""):
            self.semantic2hidden = nn.Linear(opt["attribute_prediction_k"], opt["dim_hidden"],
                                             bias="pp_emb" in opt.get("use_attr_type", ""))


class Predictor(nn.Module):
    def __init__(self, nets):
        super().__init__()
        self.nets = nn.ModuleList(nets)


def _get_predictor(opt) -> Optional[nn.Module]:
    """`get_predictor` (models/Predictor/__init__.py:26-60) for the in-scope predictors."""
    table = {"Predictor_attribute": Predictor_attribute, "SemanticContainer": SemanticContainer}
    nets = []
    for crit in opt["crits"]:
        if crit == "lang":
            continue
        name = "Predictor_{}".format(crit)
        if name not in table:
            raise ValueError("We can not find the class `{}` in {}".format(name, __file__))
        nets.append(table[name](opt))
    for name in opt.get("predictors_to_be_added", []):
        if name not in table:
            raise ValueError("We can not find the class `{}` in {}".format(name, __file__))
        nets.append(table[name](opt))
    return Predictor(nets) if nets else None


class _DecoderEmbeddings(nn.Module):
    """Parameters of Embeddings (models/components/Embeddings.py:90-132)."""

    def __init__(self, opt):
        super().__init__()
        self.word_embeddings = nn.Embedding(opt["vocab_size"], opt["dim_hidden"], padding_idx=PAD)
        self.position_embeddings = _position_table(opt, opt["max_len"])
        if not opt.get("transformer_pre_ln", False):  # Embeddings.py:130-131: a pre-LN decoder has no LayerNorm here
            self.LayerNorm = nn.LayerNorm(opt["dim_hidden"], eps=opt["layer_norm_eps"])


class _DecoderLayer(nn.Module):
    """Parameters of DecoderLayer (models/components/Layers.py:55-135), CARE / Base variants."""

    def __init__(self, opt):
        super().__init__()
        self.intra_attention = _MHA(opt)
        modality = opt["modality"] if opt.get("modality_for_decoder", None) is None else opt["modality_for_decoder"]
        hybrid_length = opt["n_frames"] * len(modality) + opt.get("use_attr_topk", 30)
        if "r" in modality:
            hybrid_length += opt["retrieval_topk"] - opt["n_frames"]
        hb = hybrid_length if opt.get("add_hybrid_attention_bias", False) else 0
        self.inter_attention = _MHA(opt, hb)
        if opt.get("use_attr", False) and "att" in opt.get("use_attr_type", "att"):
            # Layers.py:117-119: attr_attention = deepcopy(inter_attention) -> same parameter tree
            if opt.get("attr_layer_pos", "cross2attr") != "cross2attr":
                raise ValueError("only attr_layer_pos='cross2attr' (tasks.yaml:58) is on the path")
            self.attr_attention = _MHA(opt, hb)
        self.ffn = _FFN(opt)


class TransformerDecoder(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.embedding = _DecoderEmbeddings(opt)
        self.layers = nn.ModuleList([_DecoderLayer(opt) for _ in range(opt["num_hidden_layers_decoder"])])
        if opt.get("transformer_pre_ln", False):  # Decoder/Transformer.py:80-81: the final LayerNorm of a pre-LN decoder
            if opt["encoder"] != "Embedder":
                raise ValueError("transformer_pre_ln with a self-attention encoder is outside the hot path")
            self.LayerNorm = nn.LayerNorm(opt["dim_hidden"], eps=opt["layer_norm_eps"])

    def get_word_embeddings(self):
        return self.embedding.word_embeddings

    def get_embeddings(self):
        return self.embedding


class NaiveHead(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.tgt_word_prj = nn.Linear(opt["dim_hidden"], opt["vocab_size"], bias=False)

    def get_word_embeddings(self):
        return self.tgt_word_prj


# --------------------------------------------------------------------------- framework
def get_framework(opt: Dict[str, Any]) -> nn.Module:
    """Same contract as models/Framework.py:14-51 for the Transformer branch."""
    if "rnn" in opt["decoder"].lower():
        raise ValueError("RNN decoders are outside the hot path (SURVEY.md section 2, row 14)")
    for key, table in (("encoder", _ENCODERS), ("decoder", {"TransformerDecoder": TransformerDecoder}),
                       ("cls_head", {"NaiveHead": NaiveHead})):
        if opt[key] not in table:
            raise ValueError("We can not find the class `{}` in {}".format(opt[key], __file__))
    if opt.get("with_backbones") or opt.get("pointer") or opt.get("with_category"):
        raise ValueError("backbones / pointer / category inputs are outside the hot path")
    # options that change the layout of the modules on the path (other parameters, other shapes: a checkpoint of such a model
    # would not load) or its decoding scheme - named here rather than ignored
    if opt.get("decoding_type", "ARFormer") != "ARFormer":
        raise ValueError("decoding_type {!r}: only the autoregressive decoder is on the hot path".format(opt.get("decoding_type")))
    if opt.get("fusion", "temporal_concat") != "temporal_concat":
        raise ValueError("fusion {!r}: only temporal_concat (opts.py:36) is on the hot path".format(opt.get("fusion")))
    for key in ("RPE", "compositional_intra", "compositional_inter", "compositional_ffn"):
        if opt.get(key, False):
            raise ValueError("{} is outside the hot path".format(key))
    if opt.get("use_attr", False) and ("pp_emb" in opt.get("use_attr_type", "") or "prefix" in opt.get("use_attr_type", "")):
        # `use_attr_flags` Gp.. / use_attr_type 'prefix': the guidance vector / the concept rows PREPENDED to the decoder's input
        # sequence under a mask of their own (Embeddings.py:155-157, Decoder/Transformer.py:131-160) - another decoder layout,
        # used by no shipped script; refused rather than decoded as the additive form
        raise ValueError("use_attr_type {!r} (prefix guidance) is outside the hot path".format(opt.get("use_attr_type")))
    keys = ["encoder_hidden_states"]
    if opt.get("use_attr", False) and ("prefix" in opt["use_attr_type"] or "att" in opt["use_attr_type"].lower()):
        keys += ["semantic_embs"]
    if "emb" in opt.get("use_attr_type", ""):
        keys += ["semantic_hidden_states"]
    return TransformerSeq2Seq(opt, keys)


_ENGINE_BUILD_LOCK = threading.Lock()


class TransformerSeq2Seq(nn.Module):
    """`Seq2SeqBase` + `TransformerSeq2Seq` (models/Framework.py:54-269) on the HIP engine."""

    def __init__(self, opt: Dict[str, Any], input_keys_for_decoder: List[str]):
        super().__init__()
        self.backbone = None
        self.encoder = _ENCODERS[opt["encoder"]](opt)
        self.predictor = _get_predictor(opt)
        self.decoder = TransformerDecoder(opt)
        self.pointer = None
        self.cls_head = NaiveHead(opt)
        self.input_keys_for_decoder = input_keys_for_decoder
        self.opt = opt
        self._init_weights()
        self._engine: Optional[HipEngine] = None
        self._engine_stamp = None
        self._compute_dtype = opt.get("care_compute_dtype") or os.environ.get("CARE_AMD_DTYPE", "fp32")
        self._compute_dtype = {"half": "fp16", "16bit": "fp16"}.get(self._compute_dtype, self._compute_dtype)
        self._fused_head = os.environ.get("CARE_TRAIN_FUSED_HEAD", "0").strip().lower() in ("1", "true", "on", "yes")

    # -- initialisation: same distributions as models/Framework.py:115-134
    def _init_weights(self):
        for module in self.modules():
            if isinstance(module, nn.Linear):
                nn.init.xavier_uniform_(module.weight)
                if module.bias is not None:
                    module.bias.data.zero_()
            elif isinstance(module, nn.Embedding):
                nn.init.xavier_uniform_(module.weight)
                if module.padding_idx is not None:
                    module.weight.data[module.padding_idx].zero_()
            elif isinstance(module, nn.LayerNorm):
                module.weight.data.fill_(1.0)
                module.bias.data.zero_()

    # -- engine management
    def __getstate__(self):
        """Pickling / copy.deepcopy of the module (torch.save(model), DDP's spawn, ModelEnsemble-style copies): the inference
        engine - device workspaces, captured hipGraphs, the loaded library - is not part of the module's state; a copy
        builds its own on first use."""
        state = dict(self.__dict__)
        state["_engine"], state["_engine_stamp"] = None, None
        return state

    def set_compute_dtype(self, dtype: str) -> "TransformerSeq2Seq":
        """'fp32' (exact f32 MFMA, parity mode), 'bf16' (bf16 MFMA, fp32 accumulation: throughput mode), 'fp16' (the same
        kernels compiled for IEEE half, libcare_hip_f16.so: bf16's bytes and MFMA rate with 11 significand bits instead
        of 8 - the 16-bit mode nearest the reference) or 'fp16x3' (fp32 storage, every GEMM as three fp16 MFMA passes
        over hi/lo pieces: fp32-grade results at about twice fp32 mode's rate - the mode that meets the reference's
        fp32 tolerances without the exact-f32 MFMA).
        'half' (= '16bit') names the DEFAULT 16-bit mode: `fp16` - at bf16's throughput (98 - 99 %) it is 8 x closer to the
        reference (hidden states: max 1.9e-3 / mean 2.6e-4 against 1.5e-2 / 2.1e-3; tests/test_gpu_scale.py counts the
        captions that differ at MSRVTT-test scale).  Its one condition is the range of the raw features, |x| < 65504
        (care_amd.data.fp16_range_ok checks a loader's batches); `bf16` stays available by name for features without a bound."""
        dtype = {"half": "fp16", "16bit": "fp16"}.get(dtype, dtype)
        if dtype != self._compute_dtype:
            self._compute_dtype = dtype
            self._engine = None
        return self

    @property
    def compute_dtype(self) -> str:
        return self._compute_dtype

    def set_fused_head(self, on: bool) -> "TransformerSeq2Seq":
        """Training mode only (care_amd/training.py reads it): True - the vocabulary head is not run by forward(); `logits` is a
        care_amd.criterion.DeferredLogits (the hidden states + the head's weight) and LanguageGeneration runs the head fused
        with its loss over the live label positions, the [N, t, V] logits and their gradient never in memory.
        Default: off (the environment variable CARE_TRAIN_FUSED_HEAD=1 turns it on for models built afterwards); with it off
        every launch and result of training mode is what it was.  Eval mode does not read it."""
        self._fused_head = bool(on)
        return self

    @property
    def fused_head(self) -> bool:
        return bool(getattr(self, "_fused_head", False))

    def engine(self) -> HipEngine:
        if self.training:
            raise NotImplementedError(
                "the inference engine (encoding_phase / decoding_phase / translate) runs in eval mode: call .eval(); "
                "in training mode use forward() / feedforward_step(), which run under autograd (care_amd/training.py)")
        params = list(self.parameters())
        device = params[0].device
        stamp = (device, self._compute_dtype, tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
        if self._engine is not None and self._engine_stamp == stamp:
            return self._engine
        with _ENGINE_BUILD_LOCK:   # (threads sharing a module: one of them builds / re-packs, the others find it done)
            return self._engine_locked(stamp, device)

    def _engine_locked(self, stamp, device) -> HipEngine:
        if self._engine is None or self._engine_stamp != stamp:
            if device.type != "cuda":
                raise RuntimeError("the model is on `{}`: move it to the MI355X (model.to('cuda')); "
                                   "there is no CPU fallback".format(device))
            if self._engine is None or self._engine.dtype != self._compute_dtype:
                self._engine = HipEngine(self.opt, self._compute_dtype)
            self._engine.load_weights(self.state_dict(), device)
            self._engine_stamp = stamp
        return self._engine

    # -- reference API
    def get_keys_to_device(self, teacher_forcing=False, **kwargs):
        keys = ["feats", "input_ids"]
        for k in self.input_keys_for_decoder:
            if "hidden_states" not in k:
                keys.append(k)
        return keys

    def _on_device(self):
        """The module's device as the current device of what follows (kernels go to the CURRENT device with this module's
        pointers; a process that drives several GPUs need not have set it) - a no-op when it already is, or on the CPU."""
        p = next(self.parameters(), None)
        return torch.cuda.device(p.device) if p is not None and p.is_cuda else contextlib.nullcontext()

    def encoding_phase(self, feats: List[torch.Tensor], **kwargs) -> Dict[str, torch.Tensor]:
        n_mod = len(self.opt["modality"])
        with torch.no_grad(), self._on_device(), self.engine().lock:
            eng = self.engine()
            eng._begin_pass(eng.plan_for(feats[0].shape[0]))
            out = eng.encode(list(feats[:n_mod]))
        if self.predictor is not None:
            out["attribute_prediction_prj"] = self.predictor.nets[0].prj
        return out

    def prepare_inputs_for_decoder(self, encoding_phase_outputs, batch) -> Dict[str, torch.Tensor]:
        inputs = {}
        for key in self.input_keys_for_decoder:
            if key not in encoding_phase_outputs.keys() and key not in batch.keys():
                raise KeyError("the input key `{}` can not be found in `encoding_phase_outputs` {} nor `batch` {}".format(
                    key, encoding_phase_outputs.keys(), batch.keys()))
            src = batch if key not in encoding_phase_outputs.keys() else encoding_phase_outputs
            inputs[key] = src[key]
        return inputs

    def decoding_phase(self, input_ids, inputs_for_decoder, last_time_step_logits: bool = False, **kwargs):
        """Stateless decoder call on a full prefix (Framework.py:240-269)."""
        mem = inputs_for_decoder["encoder_hidden_states"]
        if isinstance(mem, list):
            assert len(mem) == 1
            mem = mem[0]
        # The auxiliary entries of the reference's decoder dict (attention probabilities, contexts,
        # intermediate embeddings: Decoder/Transformer.py:239-252; read by regularisers and notebooks,
        # never by decoding) come with every full-sequence call, like there; the per-step calls of a
        # decode loop (last_time_step_logits) skip them unless asked (`output_auxiliary=True`).
        aux = kwargs.get("output_auxiliary", not last_time_step_logits)
        with torch.no_grad(), self._on_device(), self.engine().lock:
            eng = self.engine()
            plan = eng._begin_pass(eng.plan_for(mem.shape[0], rows=input_ids.numel()))
            return eng.decode_full(input_ids, mem, inputs_for_decoder.get("semantic_hidden_states"),
                                             want_logits="last" if last_time_step_logits else "all",
                                             sem_embs=inputs_for_decoder.get("semantic_embs"), want_aux=bool(aux), plan=plan)

    def feedforward_step(self, batch: Dict[str, Any], **kwargs) -> Dict[str, Any]:
        if self.training:
            # models/Wrapper.py:423-435 -> Framework.py:215-237 with dropout active, under autograd: every op's
            # forward and backward is a HIP kernel behind the C ABI (care_amd/training.py)
            from .training import training_forward
            with self._on_device():
                return training_forward(self, batch, **kwargs)
        enc = self.encoding_phase(batch["feats"], **kwargs)
        inputs = self.prepare_inputs_for_decoder(enc, batch)
        dec = self.decoding_phase(batch["input_ids"], inputs, **kwargs)
        return {**enc, **dec, "schedule_sampling_prob": 0}

    def forward(self, batch: Dict[str, Any], **kwargs) -> Dict[str, Any]:
        return self.feedforward_step(batch, **kwargs)

"""ASRModel on MI355X: drop-in for the training path of ``tiny_audio/asr_modeling.py``.

Same constructor argument (an ASRConfig), same ``forward(input_ids, input_features, audio_attention_mask,
attention_mask, labels, audio_token_counts, ...)`` -> object with ``.loss`` / ``.logits``, same sub-module
names (``audio_tower``, ``projector``, ``language_model``), projector-only ``state_dict()`` with the
reference's key names (asr_modeling.py:398-422).  Encoder and LM are frozen; ``loss.backward()`` produces
gradients for the projector parameters only, through two HIP composites (LM dX backward, projector backward).

There is no CPU path: without libta355.so / a GPU every entry point raises.
"""
from __future__ import annotations

import contextlib
from collections.abc import Mapping
from typing import Iterator, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from .asr_config import ASRConfig, WhisperEncoderConfig, compute_encoder_output_length
from .decoding import check_decay_window
from .encoder import GlmAsrEncoderMI355X
from .whisper_encoder import WhisperEncoderMI355X
from .language_model import NO_NORM_FULL_FT, FrozenLMLoss, Qwen3MI355X, check_loss_options
from .ops import F32
from .projectors import PROJECTOR_CLASSES


@contextlib.contextmanager
def _eval_mode(model):
    """``model.eval()`` inside the block; the mode it had comes back on every way out (a generator closed early included)."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


class CausalLMOutput(dict):
    """What ``ASRModel.forward`` returns.  Like transformers' ``ModelOutput`` (``CausalLMOutputWithPast``): the dict holds only
    the fields that are not None, in order -- ``loss``, ``logits`` -- with attribute, key, index and slice access (HF
    ``Trainer.compute_loss`` reads ``outputs["loss"]`` / ``outputs[0]``; ``Trainer.prediction_step`` builds
    ``tuple(v for k, v in outputs.items() if k != "loss")`` and concatenates it over batches, so no None and no Python scalar
    may sit among the items).  This path's extras are plain attributes, not items: ``nll`` (per label token),
    ``n_label_tokens`` (int), ``aux_loss``, ``loss_ce`` (the LM's cross-entropy alone: loss = loss_ce + aux_loss)."""

    _items = ("loss", "logits")
    _extras = ("nll", "n_label_tokens", "aux_loss", "loss_ce")

    def __init__(self, loss=None, logits=None, nll=None, n_label_tokens=None, aux_loss=None, loss_ce=None):
        super().__init__()
        if isinstance(loss, Mapping):                 # ModelOutput.__init__ accepts a mapping as its first argument, and library code
            src = loss                                # rebuilds outputs that way: accelerate's convert_to_fp32 / send_to_device do
            loss, logits = src.get("loss"), src.get("logits")     # type(data)({k: f(v) ...}) around model.forward under bf16=True
            unknown = [k for k in src if k not in self._items]
            if unknown:
                raise KeyError(f"CausalLMOutput has no item {unknown[0]!r}")
            if isinstance(src, CausalLMOutput):       # (a rebuild from a plain dict cannot carry the attribute extras: they become None)
                nll, n_label_tokens, aux_loss, loss_ce = src.nll, src.n_label_tokens, src.aux_loss, src.loss_ce
        for k, v in (("loss", loss), ("logits", logits)):
            if v is not None:
                dict.__setitem__(self, k, v)
        for k, v in (("nll", nll), ("n_label_tokens", n_label_tokens), ("aux_loss", aux_loss), ("loss_ce", loss_ce)):
            object.__setattr__(self, k, v)

    def __getattr__(self, k):                     # reached only when the normal lookup fails: an item, or an absent item
        if k in CausalLMOutput._items:
            return dict.get(self, k)
        raise AttributeError(k)

    def __getitem__(self, k):
        if isinstance(k, (int, slice)):
            return tuple(self.values())[k]
        return dict.__getitem__(self, k)

    def to_tuple(self):
        return tuple(self.values())

    def __reduce__(self):                             # copy / pickle keep the extras
        return (CausalLMOutput, (dict.get(self, "loss"), dict.get(self, "logits"), self.nll, self.n_label_tokens, self.aux_loss, self.loss_ce))


class GenerationOutput(dict):
    """What ``ASRModel.generate`` returns when decoding scores are asked for (``return_token_scores`` / ``top_logprobs``); like
    ``CausalLMOutput`` the dict holds the fields that are not None, in order, with attribute, key, index and slice access:
    ``sequences`` int64 [B, n_new], ``token_logprobs`` f32 [B, n_new] (log-probability of every emitted token under the processed
    distribution it was chosen from: HF's ``compute_transition_scores(..., normalize_logits=True)``), ``token_entropy`` f32
    [B, n_new] (nats), and with ``top_logprobs`` = k > 0 ``top_token_ids`` int64 [B, n_new, k] / ``top_logprobs`` f32 [B, n_new, k]
    (descending; slots beyond the finite entries are -1 / -inf).  Positions after a clip's first eos hold 0 / 0 / -1 / -inf.
    HF's ``scores`` (the full [B, V] row of every step) is deliberately not kept, so that name is not used.
    ``ASRModel.generate_beams`` returns ``sequences`` int64 [B * num_return_sequences, n_new] with ``sequences_scores`` f32
    [B * num_return_sequences] (HF's name: the length-penalised sum of log-probabilities of every returned hypothesis)."""

    _items = ("sequences", "token_logprobs", "token_entropy", "top_token_ids", "top_logprobs", "sequences_scores")

    def __init__(self, sequences=None, token_logprobs=None, token_entropy=None, top_token_ids=None, top_logprobs=None,
                 sequences_scores=None):
        super().__init__()
        if isinstance(sequences, Mapping):            # rebuilt from a mapping, as library code does with ModelOutput
            src = sequences
            unknown = [k for k in src if k not in self._items]
            if unknown:
                raise KeyError(f"GenerationOutput has no item {unknown[0]!r}")
            sequences, token_logprobs, token_entropy, top_token_ids, top_logprobs, sequences_scores = (src.get(k) for k in self._items)
        for k, v in zip(self._items, (sequences, token_logprobs, token_entropy, top_token_ids, top_logprobs, sequences_scores)):
            if v is not None:
                dict.__setitem__(self, k, v)

    def __getattr__(self, k):                     # reached only when the normal lookup fails: an item, or an absent item
        if k in GenerationOutput._items:
            return dict.get(self, k)
        raise AttributeError(k)

    def __getitem__(self, k):
        if isinstance(k, (int, slice)):
            return tuple(self.values())[k]
        return dict.__getitem__(self, k)

    def to_tuple(self):
        return tuple(self.values())

    def __reduce__(self):
        return (GenerationOutput, tuple(dict.get(self, k) for k in self._items))


class ScoreOutput(dict):
    """What ``ASRModel.score`` returns; a dict in the style of ``GenerationOutput`` (the fields that are not None, in order, with
    attribute, key, index and slice access): ``scores`` f32 [R] (sum of the candidate's token log-probabilities), ``candidate_clip``
    int64 [R] and ``n_tokens`` int64 [R], rows clip-major in the order the candidates were given; with ``return_token_scores`` also
    ``token_ids`` int64 [R, T] and ``token_logprobs`` f32 [R, T] (exact 0 behind a candidate's end).  ``per_clip()`` regroups them."""

    _items = ("scores", "candidate_clip", "n_tokens", "token_ids", "token_logprobs")

    def __init__(self, scores=None, candidate_clip=None, n_tokens=None, token_ids=None, token_logprobs=None, n_clips=None):
        super().__init__()
        for k, v in zip(self._items, (scores, candidate_clip, n_tokens, token_ids, token_logprobs)):
            if v is not None:
                dict.__setitem__(self, k, v)
        self.n_clips = n_clips

    def __getattr__(self, k):                     # reached only when the normal lookup fails: an item, or an absent item
        if k in ScoreOutput._items:
            return dict.get(self, k)
        raise AttributeError(k)

    def __getitem__(self, k):
        if isinstance(k, (int, slice)):
            return tuple(self.values())[k]
        return dict.__getitem__(self, k)

    def to_tuple(self):
        return tuple(self.values())

    def __reduce__(self):
        return (ScoreOutput, tuple(dict.get(self, k) for k in self._items) + (self.n_clips,))

    def per_clip(self):
        """One list per clip, in the order given: a dict(score, n_tokens[, token_ids, token_logprobs cut to the candidate's length])
        per candidate; an empty list for a clip without candidates."""
        clip = self["candidate_clip"].tolist()
        n = self["n_tokens"].tolist()
        s = self["scores"].detach().cpu().tolist()
        B = self.n_clips if self.n_clips is not None else (max(clip) + 1 if clip else 0)
        out = [[] for _ in range(B)]
        for r, b in enumerate(clip):
            item = dict(score=s[r], n_tokens=n[r])
            if "token_logprobs" in self:
                item["token_ids"] = self["token_ids"][r, :n[r]].tolist()
                item["token_logprobs"] = self["token_logprobs"][r, :n[r]].detach().cpu().tolist()
            out[b].append(item)
        return out


def _is_cjk(ch: str) -> bool:
    """CJK ideograph blocks (a streamer releases such characters one by one: they carry no spaces)."""
    cp = ord(ch)
    return any(lo <= cp <= hi for lo, hi in ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F),
                                             (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F)))


class _TextPieces:
    """Incremental detokeniser with the release rule of transformers' TextStreamer (generation/streamers.py
    ``put``/``end``): decode the tokens of the current line, release a finished line whole, a trailing CJK character at
    once, otherwise everything up to the last space; ``flush`` releases the rest."""

    def __init__(self, tokenizer):
        self.tok, self.ids, self.shown = tokenizer, [], 0

    def push(self, token_id: int) -> str:
        self.ids.append(int(token_id))
        text = self.tok.decode(self.ids, skip_special_tokens=True)
        if text.endswith("\n"):
            out, self.ids, self.shown = text[self.shown:], [], 0
        elif text and _is_cjk(text[-1]):
            out, self.shown = text[self.shown:], len(text)
        else:
            cut = text.rfind(" ") + 1
            out = text[self.shown:cut] if cut > self.shown else ""
            self.shown = max(self.shown, cut)
        return out

    def flush(self) -> str:
        out = self.tok.decode(self.ids, skip_special_tokens=True)[self.shown:] if self.ids else ""
        self.ids, self.shown = [], 0
        return out


class _ThinkGate:
    """Drops ``<think>...</think>`` spans from a stream of text pieces (tiny_audio/asr_modeling.py:737-757)."""

    def __init__(self):
        self.buf, self.inside = "", False

    def feed(self, text: str):
        self.buf += text
        while "<think>" in self.buf:
            self.inside = True
            before, self.buf = self.buf.split("<think>", 1)
            if before:
                yield before
        while self.inside and "</think>" in self.buf:
            self.inside = False
            self.buf = self.buf.split("</think>", 1)[1]
        if not self.inside and self.buf:
            out, self.buf = self.buf, ""
            yield out

    def flush(self) -> str:
        out = "" if self.inside else self.buf
        self.buf = ""
        return out


class ASRModel(nn.Module):
    config_class = ASRConfig
    main_input_name = "input_features"
    TRANSCRIBE_PROMPT = "Transcribe the speech to text"

    def __init__(self, config: ASRConfig, device="cuda", init="random", seed=0, ragged_encoder=False, **kwargs):
        super().__init__()
        self.config = config
        self.device_ = torch.device(device)
        self._ragged_encoder = False
        # asr_modeling.py:203-237: a Whisper encoder for every "whisper" audio_model_id, GLM-ASR's audio tower otherwise
        if isinstance(config.audio_config, WhisperEncoderConfig):
            self.audio_tower = WhisperEncoderMI355X(config.audio_config, device=device)
        else:
            self.audio_tower = GlmAsrEncoderMI355X(config.audio_config, device=device)
        tc = config.text_config
        if tc.model_type != "qwen3":
            # ASRConfig's token-id defaults are Qwen3's (151669 / 151643 / 151645): beyond a SmolLM3 / Llama vocabulary they would index
            # the embedding table out of range
            for name in ("audio_token_id", "pad_token_id", "eos_token_id"):
                tid = getattr(config, name, None)
                if tid is not None and int(tid) >= tc.vocab_size:
                    raise ValueError(f"{name} = {tid} lies outside the {tc.model_type} vocabulary (vocab_size = {tc.vocab_size}): "
                                     f"pass the tokenizer's own id")
            if not getattr(config, "freeze_language_model", True):
                raise NotImplementedError(NO_NORM_FULL_FT)
        self.language_model = Qwen3MI355X(config.text_config, device=device)              # :143
        self.audio_token_id = config.audio_token_id
        self.projector = self._create_projector(config).to(device=device, dtype=F32)      # :163
        if not getattr(config, "freeze_language_model", True):
            # full decoder fine-tuning (asr_modeling.py:251-253; embedded.yaml:23): the LM's fp32 masters become Parameters
            # as soon as its weights exist (now for init="random", at load_state_dict_hf otherwise)
            self.language_model.keep_fp32 = self.language_model.want_train_base = True
        if init == "random":
            self.audio_tower.random_init(seed)
            self.language_model.random_init(seed + 1)
        if getattr(config, "use_lora", False):
            self._setup_lora(config, seed)
        if getattr(config, "freeze_projector", False):
            self.projector.requires_grad_(False)
        self._drop_seed = 0x5EED + seed
        self.tokenizer = kwargs.get("tokenizer")        # optional: only needed when generate() must build the prompt
        if self.tokenizer is not None and hasattr(self.tokenizer, "convert_tokens_to_ids"):
            # the reference reads the placeholder's id from the tokenizer (tiny_audio/asr_modeling.py:160-171), config.json
            # does not carry it
            tid = self.tokenizer.convert_tokens_to_ids("<audio>")
            if tid is not None and int(tid) >= 0:
                self.audio_token_id = config.audio_token_id = int(tid)
        self.system_prompt = getattr(config, "system_prompt", None)
        # the reference builds its WhisperFeatureExtractor here (tiny_audio/asr_modeling.py:146, :190-201; padding disabled for
        # GLM-ASR); this one computes the log-mel on the device.  ``feature_extractor=`` hands in another one.
        self.feature_extractor = kwargs.get("feature_extractor") or self._create_feature_extractor(config)
        self.ragged_encoder = ragged_encoder

    @property
    def ragged_encoder(self) -> bool:
        """True: the frozen GLM-ASR tower encodes every clip at its OWN mel length (``audio_attention_mask.sum(-1)``) -- what the
        reference computes for a clip at inference, where it is encoded alone without padding (tiny_audio/asr_modeling.py:198-200)
        -- instead of padded to the longest clip of the batch with the padding attended to, as the reference's training forward
        does (:448-450).  A deliberate, opt-in difference from the reference's training arithmetic, in the
        class of sequence packing; a run-time attribute, not an ``ASRConfig`` / ``config.json`` field.  ``forward``, ``generate``
        and ``generate_streaming`` then need ``audio_attention_mask``; the lengths are taken on the host, which costs one
        device sync per call when the mask lives on the device (the collators emit it on the host).  Whisper towers refuse it:
        their contract is a fixed 30 s window with attention over the padding (TF:models/whisper/modeling_whisper.py:612-616)."""
        return self._ragged_encoder

    @ragged_encoder.setter
    def ragged_encoder(self, on):
        if on and isinstance(self.audio_tower, WhisperEncoderMI355X):
            raise ValueError(f"ragged_encoder is not available for the Whisper audio tower ({type(self.audio_tower).__name__}): Whisper "
                             "encodes a fixed 30 s window and attends to its padding (TF:models/whisper/modeling_whisper.py:612-616); "
                             "only the GLM-ASR tower encodes clips at their own lengths")
        self._ragged_encoder = bool(on)

    def _mel_lengths(self, audio_features, audio_attention_mask):
        """The ragged encoder's per-clip mel lengths as host ints (None with the switch off); ValueError on a missing mask or a
        length outside [1, T]."""
        if not self._ragged_encoder:
            return None
        if audio_attention_mask is None:
            raise ValueError("ragged_encoder=True needs audio_attention_mask: the clips' mel lengths are its row sums")
        B, _, T = audio_features.shape
        mask = torch.as_tensor(audio_attention_mask)
        if mask.dim() != 2 or mask.shape[0] != B or mask.shape[1] != T:
            raise ValueError(f"audio_attention_mask must be [{B}, {T}] like input_features' clips and frames; got {tuple(mask.shape)}")
        return self.audio_tower.check_mel_lengths(mask.sum(dim=-1), B, T)        # one sync if the mask is on the device

    def _apply_stream_modes(self):
        """``config.model_dtype`` decides where the residual streams are STORED, as it does in the reference: "bfloat16" (the
        reference ASRConfig's default, tiny_audio/asr_config.py:41: bf16 modules) -> bf16 streams; "float32" (the training
        recipe, configs/config.yaml:14-18 with bf16 autocast) -> fp32 streams.  Compute is bf16 MFMA with fp32 accumulation in
        both (the reference's ``bf16: true``); the trainable masters are fp32 in both.  ``config.residual_dtype`` overrides."""
        rd = getattr(self.config, "residual_dtype", None) or getattr(self.config, "model_dtype", "bfloat16")
        f32 = str(rd).replace("torch.", "") in ("float32", "fp32", "float")
        # per-model state since round 6 (fields of the two weights handles, include/ta355.h ABI 4): another ASRModel of another
        # model_dtype in the same process, or a decoding thread, is not affected
        if self.audio_tower.res_f32 != f32:
            self.audio_tower.res_f32 = f32
        lm = self.language_model
        if lm.res_f32 != f32 or lm.dx_f32 != f32:
            lm.res_f32 = lm.dx_f32 = f32

    def _setup_lora(self, config, seed=0):
        """Stage-2 adapters on the LM (tiny_audio/asr_modeling.py:289-301: LoraConfig(r, lora_alpha,
        target_modules, lora_dropout, bias="none", task_type="CAUSAL_LM"))."""
        self.language_model.enable_lora(rank=config.lora_rank, alpha=config.lora_alpha, dropout=config.lora_dropout,
                                        target_modules=config.lora_target_modules, seed=seed + 2)

    def _create_feature_extractor(self, config):
        from .asr_processing import LogMelFeatureExtractor
        fe = LogMelFeatureExtractor(int(getattr(config.audio_config, "num_mel_bins", 128)), self.device_)
        if isinstance(config.audio_config, WhisperEncoderConfig):
            # the reference disables the 30 s padding for GLM-ASR only (tiny_audio/asr_modeling.py:190-201): Whisper's encoder
            # takes exactly 3000 frames
            fe.padding = "max_length"
        return fe

    def get_processor(self):
        """tiny_audio/asr_modeling.py:384-396: the processor that pairs with this model (its feature extractor, its tokenizer, its
        projector's length rule, its encoder's conv geometry)."""
        from .asr_processing import ASRProcessor
        if self.tokenizer is None:
            raise ValueError("get_processor needs a tokenizer: construct ASRModel(..., tokenizer=tok) or set model.tokenizer")
        return ASRProcessor(feature_extractor=self.feature_extractor, tokenizer=self.tokenizer, projector=self.projector,
                            encoder_conv_layers=self.config.encoder_conv_layers)

    # ---- the PreTrainedModel surface HF tooling touches (tiny_audio/asr_modeling.py:359-382, :535-546)
    def get_input_embeddings(self):
        """A frozen ``nn.Embedding`` VIEW of the LM's fp32 lookup table (no copy); the training forward does not go through it
        (the lookup is fused with the <audio> scatter, ``ta_embed_scatter``)."""
        w = self.language_model.ft_embed if self.language_model.train_base else self.language_model.get_input_embeddings_weight()
        emb = nn.Embedding(w.shape[0], w.shape[1], _weight=w.detach(), _freeze=True)
        return emb

    def set_input_embeddings(self, value):
        """Replace the (tied) token embedding: the lookup table and both lm_head images are rebuilt from ``value.weight``."""
        self.language_model.set_embedding_weight(value.weight if hasattr(value, "weight") else value)

    def get_output_embeddings(self):
        """The tied lm_head as a bias-free ``nn.Linear`` VIEW of the same table (Qwen3 ties them: SURVEY section 8)."""
        w = self.language_model.ft_embed if self.language_model.train_base else self.language_model.get_input_embeddings_weight()
        head = nn.Linear(w.shape[1], w.shape[0], bias=False, device="meta")
        head.weight = nn.Parameter(w.detach(), requires_grad=False)
        return head

    def set_output_embeddings(self, value):
        self.set_input_embeddings(value)

    def _set_gradient_checkpointing(self, enable: bool = True, gradient_checkpointing_func=None):
        """The reference forwards this to the LM so that its activations are recomputed in the backward (:359-370).  Here the LM
        keeps a 40 KB-per-token tape (7.4 GB at B = 32) out of 288 GB and nothing is recomputed: accepted and
        recorded, so ``TrainingArguments(gradient_checkpointing=True)`` runs unchanged; results are identical either way."""
        self.gradient_checkpointing = bool(enable)

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        self._set_gradient_checkpointing(True)

    def gradient_checkpointing_disable(self):
        self._set_gradient_checkpointing(False)

    def prepare_inputs_for_generation(self, *args, **kwargs):
        """HF's ``GenerationMixin`` protocol (:535-546: audio features only on the step with ``cache_position[0] == 0``).  This
        model owns its KV cache and decode loop (``generate`` / ``generate_streaming``), so there is no per-step ``forward`` for
        the protocol to feed -- raising beats silently returning inputs that ``forward`` would refuse."""
        raise NotImplementedError("ASRModel on MI355X decodes with its own device-resident loop: call generate() / "
                                  "generate_streaming(); HF's step-wise GenerationMixin protocol is not spoken")

    def _create_projector(self, config):
        projector_type = getattr(config, "projector_type", "mlp")
        cls = PROJECTOR_CLASSES.get(projector_type)
        if cls is None:
            raise ValueError(f"Unknown projector_type: {projector_type}. Valid options: {list(PROJECTOR_CLASSES.keys())}")
        return cls(config)

    # frozen sub-models hold plain device buffers, not Parameters: parameters()/state_dict() cover the projector, the LoRA
    # adapters and -- with freeze_language_model=False -- the LM's fp32 masters
    def state_dict(self, *args, **kwargs):
        sd = {f"projector.{k}": v for k, v in self.projector.state_dict().items()}
        if self.language_model.lora_rank:       # peft adapter naming under the reference's attribute name
            sd.update(self.language_model.export_lora_state_dict(prefix="language_model.base_model.model.model."))
        if self.language_model.train_base:      # fine-tuned LM: saved with the projector (asr_modeling.py:409-421)
            sd.update({"language_model." + k: v for k, v in self.language_model.ft_state_dict_hf().items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        sub = {k[len("projector."):]: v for k, v in sd.items() if k.startswith("projector.")}
        out = self.projector.load_state_dict(sub, strict=strict)
        if self.language_model.lora_rank and any(".lora_A" in k for k in sd):
            self.language_model.load_lora_state_dict(sd)
        if self.language_model.train_base and "language_model.model.embed_tokens.weight" in sd:
            self.language_model.load_ft_state_dict_hf(sd)
        if hasattr(self.projector, "_pack_versions"):
            self.projector._pack_versions = None
        return out

    def train(self, mode: bool = True):
        """Frozen sub-modules never enter train mode (asr_modeling.py:344-357)."""
        super().train(mode)
        self.audio_tower.train(False)
        self.language_model.train(False)
        return self

    def _compute_encoder_output_lengths(self, audio_attention_mask):
        return compute_encoder_output_length(audio_attention_mask.sum(dim=-1), self.config.encoder_conv_layers)

    def _frame_keep_mask(self, B, S, frame_keep=None):
        """Whole-frame Bernoulli keep mask of _maybe_drop_audio_tokens (asr_modeling.py:458-479); applied inside
        the encoder's final LayerNorm kernel.  ``frame_keep`` injects a mask (parity tests)."""
        if frame_keep is not None:
            return frame_keep
        p = float(getattr(self.config, "audio_token_dropout", 0.0))
        if not self.training or p <= 0.0:
            return None
        self._drop_seed += 1
        return ops.bernoulli_keep(B * S, 1.0 - p, self._drop_seed, self.device_)

    def _encode_audio(self, audio_features, frame_keep=None, after_encoder=None, audio_attention_mask=None):
        """-> projector output [B, N, llm_dim] fp32 (packing into <audio> rows happens in the LM op).
        ``after_encoder``: called between the frozen encoder and the projector -- the last point of a step that has not
        read a trainable weight yet (ASRTrainer applies a deferred optimizer update there).
        ``audio_attention_mask``: read only with ``ragged_encoder`` on (the clips' own lengths)."""
        B, _, T = audio_features.shape
        S = self.audio_tower.output_length(T)
        mel_lengths = self._mel_lengths(audio_features, audio_attention_mask)
        keep = self._frame_keep_mask(B, S, frame_keep)
        if mel_lengths is not None:
            hidden = self.audio_tower(audio_features, frame_keep=keep, mel_lengths=mel_lengths).last_hidden_state
        else:
            hidden = self.audio_tower(audio_features, frame_keep=keep).last_hidden_state      # no_grad inside
        if after_encoder is not None:
            after_encoder()
        return self.projector(hidden)

    def forward(self, input_ids: Optional[torch.Tensor] = None, input_features: Optional[torch.Tensor] = None,
                audio_attention_mask: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None, audio_token_counts: Optional[torch.Tensor] = None,
                num_items_in_batch=None, return_logits: bool = True, frame_keep=None, after_encoder=None,
                position_ids: Optional[torch.Tensor] = None, past_key_values=None, inputs_embeds=None,
                use_cache: Optional[bool] = None, cache_position=None, segment_ids: Optional[torch.Tensor] = None,
                z_loss_coef: Optional[float] = None, **kwargs):
        """Training/eval forward (tiny_audio/asr_modeling.py:481-533).

        ``segment_ids`` [R, L] (sequence packing, ``DataCollator(pack_to=...)``; not in the reference): a row holds several clips'
        chat sequences back to back -- 0 on the right padding, 1, 2, ... on the tokens of the row's clips.  Attention stays inside a
        clip (same id, causal), RoPE positions restart at 0 in every clip unless ``position_ids`` is given, the label at the first
        token of a clip is never a target, and the <audio> placeholders of the c-th clip (row-major over (row, clip)) take the projector
        rows of clip c: ``input_features`` / ``audio_token_counts`` stay per clip, [C, ...].  One host check per call validates the
        layout.  ``None``: one clip per row, nothing changes.

        ``position_ids`` [B, L] (or [1, L] / [L], broadcast over the batch): the RoPE position of every token, handed to the LM
        as the reference does (asr_modeling.py:517-526 -> TF:models/qwen3/modeling_qwen3.py:386-389, default arange(L)).
        A collator that LEFT-pads (trl's DataCollatorForChatML) must pass the positions it wants: nothing is inferred from the
        attention mask, exactly as in the reference.  ``inputs_embeds`` / ``past_key_values`` / ``use_cache=True`` /
        ``cache_position`` belong to HF's incremental-decoding protocol, which this forward does not speak (``generate`` owns
        the KV cache here): they raise instead of being ignored.

        ``num_items_in_batch``: as in HF Trainer -- loss = sum(nll) / num_items_in_batch (default: the number of
        label tokens in this batch, i.e. the mean).  ``return_logits=False`` skips materialising the [B, L, V]
        logits (the HF Trainer discards them on the training path).  ``label_meta=(rows, targets, n)`` (through ``**kwargs``:
        a NAMED parameter containing "label" would enter HF Trainer's ``label_names`` -- find_labels scans the signature -- and
        Trainer.predict would then treat every batch as unlabelled) lets a
        collator that already knows the label positions on the host avoid one device->host sync.

        ``label_smoothing`` (through ``**kwargs`` for the same reason) and ``z_loss_coef``: the LM loss options for this call;
        ``None`` takes ``config.label_smoothing`` / ``config.lm_z_loss_coef`` (default 0).  As in HF they apply whenever labels are
        given, in ``eval()`` too: ``loss`` / ``loss_ce`` are then loss_scale * sum of
        (1 - eps) nll + eps (lse - mean(logits)) + z_loss_coef lse^2 over the label tokens (LabelSmoother /
        cross_entropy(label_smoothing=eps), plus the z-loss), computed with its gradient inside the cross-entropy launch; ``nll``
        stays the plain per-token NLL.
        """
        dev = self.device_
        if inputs_embeds is not None or past_key_values is not None or use_cache or cache_position is not None:
            bad = [n for n, v in (("inputs_embeds", inputs_embeds), ("past_key_values", past_key_values), ("use_cache", use_cache or None),
                                  ("cache_position", cache_position)) if v is not None]
            raise NotImplementedError(f"ASRModel.forward on MI355X does not take {', '.join(bad)}: the training / eval forward "
                                      "runs from input_ids (+ input_features) without a KV cache; use generate() for decoding")
        if input_ids is None:
            raise ValueError("input_ids is required")
        eps, zc = kwargs.pop("label_smoothing", None), z_loss_coef
        eps, zc = check_loss_options(getattr(self.config, "label_smoothing", 0.0) if eps is None else eps,
                                     getattr(self.config, "lm_z_loss_coef", 0.0) if zc is None else zc)
        self._apply_stream_modes()
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        B, L = ids.shape
        pos = None
        if position_ids is not None:
            pos = torch.as_tensor(position_ids).to(device=dev, dtype=torch.int32)
            if pos.dim() == 1:
                pos = pos[None, :]
            if pos.dim() != 2 or pos.shape[1] != L or pos.shape[0] not in (1, B):
                raise ValueError(f"position_ids must be [B, L] (or [1, L] / [L]); got {tuple(pos.shape)} for input_ids {tuple(ids.shape)}")
            # the RoPE kernels index the cos / sin tables with these: a position outside [0, max_position_embeddings) would read past
            # them (the reference raises an index error there).  One host check on this opt-in path; the default arange needs none.
            max_pos = int(self.config.text_config.max_position_embeddings)
            lo, hi = (int(v) for v in torch.aminmax(pos)) if pos.numel() else (0, 0)
            if lo < 0 or hi >= max_pos:
                raise ValueError(f"position_ids must lie in [0, {max_pos}) (max_position_embeddings); got [{lo}, {hi}]")
            pos = pos.expand(B, L).contiguous().reshape(-1)
        seg, sid = None, None
        if segment_ids is not None:
            sid, n_clips = self._check_segment_ids(segment_ids, attention_mask, B, L)
            sid = sid.to(dev).contiguous()
            seg, seg_pos = ops.segment_table(sid)
            if pos is None:
                pos = seg_pos
            if attention_mask is None:
                attention_mask = sid != 0
            if labels is not None:                        # the last token of one clip never predicts the first token of the next
                if kwargs.get("label_meta") is not None:
                    raise ValueError("label_meta cannot be combined with segment_ids: the labels at segment starts are masked here")
                first = torch.ones_like(sid, dtype=torch.bool)
                first[:, 1:] = sid[:, 1:] != sid[:, :-1]
                labels = labels.to(device=dev, dtype=torch.int64).masked_fill(first, -100)
        audio, src_row = None, None
        if input_features is None and after_encoder is not None:
            after_encoder()
        if input_features is not None:
            y = self._encode_audio(input_features.to(dev), frame_keep, after_encoder, audio_attention_mask)     # [B, N, D]
            N = y.shape[1]
            if sid is not None:
                placed = self._segment_placeholder_counts(ids, sid, n_clips)
                if audio_token_counts is None:
                    audio_token_counts = placed
                counts = audio_token_counts.to(device=dev, dtype=torch.int64).contiguous()
                if y.shape[0] != n_clips or counts.numel() != n_clips or not bool((placed == counts).all()):
                    raise ValueError(f"segment_ids holds {n_clips} clips with {placed.tolist()} <audio> placeholders; input_features has "
                                     f"{y.shape[0]} clips and audio_token_counts is {counts.tolist()}")
                src_row = ops.audio_index_seg(ids, sid, counts, N, self.audio_token_id)
            else:
                if audio_token_counts is None:
                    audio_token_counts = (ids == self.audio_token_id).sum(dim=-1)
                counts = audio_token_counts.to(device=dev, dtype=torch.int64).contiguous()
                src_row = ops.audio_index(ids, counts, N, self.audio_token_id)
            audio = y.reshape(y.shape[0] * N, -1)
        kmask = None if attention_mask is None else attention_mask.to(device=dev, dtype=torch.int32).contiguous()
        n_lab, rows, targets = 0, None, None
        if labels is not None:
            label_meta = kwargs.pop("label_meta", None)
            if label_meta is not None:
                rows, targets, n_lab = label_meta
            else:
                rows, targets, n = ops.label_rows(labels.to(device=dev, dtype=torch.int64).contiguous())
                n_lab = int(n.item())                                                      # one host sync
        scale = 1.0 / float(num_items_in_batch if num_items_in_batch is not None else max(n_lab, 1))
        if labels is None:                                    # (validated above; without labels there is no loss to apply them to)
            eps, zc = 0.0, 0.0
        if audio is None:
            audio = torch.zeros((1, self.config.llm_dim), device=dev, dtype=F32)
        loss, nll, logits = FrozenLMLoss.apply(audio, self.language_model, ids, src_row, kmask, rows, targets, n_lab,
                                               scale, bool(return_logits),
                                               *(self.language_model.lora_parameters() or self.language_model.ft_parameters()), pos=pos,
                                               **({} if seg is None else {"seg": seg}),
                                               **({"label_smoothing": eps, "z_loss": zc} if (eps > 0.0 or zc > 0.0) else {}))
        V = self.config.text_config.vocab_size
        logits = logits.reshape(B, L, -1)[:, :, :V] if return_logits else None
        aux, loss_ce = None, loss
        if labels is None:
            loss = loss_ce = None
        elif hasattr(self.projector, "get_aux_loss"):
            aux = self.projector.get_aux_loss()
            if aux is not None and aux.numel() > 0:
                loss = loss + aux.to(loss.device)                                          # asr_modeling.py:528-531
        return CausalLMOutput(loss=loss, logits=logits, nll=nll[:n_lab] if labels is not None else None,
                              n_label_tokens=n_lab, aux_loss=aux, loss_ce=loss_ce)

    # ------------------------------------------------------------------ sequence packing
    @staticmethod
    def _check_segment_ids(segment_ids, attention_mask, B, L):
        """-> (int32 [B, L] on the host, number of clips).  ValueError unless every row is 1, 2, ..., S (non-decreasing, no gaps, at
        least one clip) followed by zeros only, and -- when an attention mask is given -- the mask is exactly ``segment_ids != 0``."""
        sid = torch.as_tensor(segment_ids).detach().to("cpu")
        if sid.dim() != 2 or tuple(sid.shape) != (B, L) or sid.dtype.is_floating_point:
            raise ValueError(f"segment_ids must be an integer tensor [{B}, {L}] like input_ids; got {sid.dtype} {tuple(sid.shape)}")
        sid = sid.to(torch.int32)
        real = sid != 0
        step = sid[:, 1:] - sid[:, :-1]
        ok = bool((sid >= 0).all()) and bool((sid[:, 0] == 1).all())
        # inside the tokens the id stays or grows by one; after the first 0 everything is 0 (right padding only)
        ok = ok and bool(((step == 0) | (step == 1))[real[:, 1:]].all()) and bool((~real[:, 1:] | real[:, :-1]).all())
        if not ok:
            raise ValueError("segment_ids must be 1, 2, ..., S along every row (non-decreasing, no gaps), then 0 on the right padding")
        if attention_mask is not None:
            att = torch.as_tensor(attention_mask).detach().to("cpu")
            if tuple(att.shape) != (B, L) or not bool(((att != 0) == real).all()):
                raise ValueError("attention_mask disagrees with segment_ids: it must be 1 exactly where segment_ids != 0")
        return sid, int(sid.max(dim=1).values.sum())

    def _segment_placeholder_counts(self, ids, sid, n_clips):
        """<audio> placeholders of every clip of a packed batch, in clip order (row-major over (row, segment)) -> int64 [C], device."""
        per_row = sid.max(dim=1).values.to(torch.int64)
        clip = (torch.cumsum(per_row, 0) - per_row)[:, None] + sid.to(torch.int64) - 1          # clip index of every token (junk on padding)
        m = (ids == self.audio_token_id) & (sid != 0)
        return torch.bincount(clip[m], minlength=n_clips)[:n_clips]

    # ------------------------------------------------------------------ checkpoints
    def save_pretrained(self, save_directory, **kwargs):
        """model.safetensors (projector.*) + config.json (+ PEFT adapter files with LoRA), the reference's layout
        (tiny_audio/asr_modeling.py:769-852)."""
        from .checkpoint import save_pretrained
        save_pretrained(self, str(save_directory))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, **kwargs):
        """tiny_audio/asr_modeling.py:59-131 for a local directory."""
        from .checkpoint import load_pretrained
        return load_pretrained(cls, str(pretrained_model_name_or_path), **kwargs)

    # ------------------------------------------------------------------ generation
    def _generation_setting(self, name, default, overrides):
        v = overrides.pop(name, None)
        if v is None:
            v = getattr(self.config, name, None)
        return default if v is None else v

    def _get_num_audio_tokens(self, audio_attention_mask):
        """tiny_audio/asr_modeling.py:548-560"""
        lens = self._compute_encoder_output_lengths(audio_attention_mask)
        return int(self.projector.get_output_length(int(lens.max().item())))

    def _prepare_generation(self, input_ids, input_features, audio_attention_mask, attention_mask, system_prompt, kw, beams=False):
        """Everything ``generate``, ``generate_streaming`` and ``generate_beams`` share (tiny_audio/asr_modeling.py:580-640, :669-716):
        generation settings, audio -> encoder -> projector, the chat prompt with one <audio> placeholder per projected
        frame, and the placeholder -> audio-row index.  -> kwargs of ``Qwen3MI355X.greedy_decode_iter``; with ``beams`` (the caller
        has taken the beam settings out of ``kw``) those of ``Qwen3MI355X.beam_decode``, which takes no ``sampling``."""
        if input_features is None:
            raise ValueError("input_features required for generation")
        if audio_attention_mask is None:
            raise ValueError("audio_attention_mask required for generation")
        self._apply_stream_modes()
        max_new = int(self._generation_setting("max_new_tokens", 128, kw))
        if not beams and int(self._generation_setting("num_beams", 1, kw)) != 1:
            raise NotImplementedError("generate() is greedy search or sampling (num_beams 1, the reference's generation config, "
                                      "asr_config.py:103-111); beam search is ASRModel.generate_beams(...)")
        # do_sample / temperature / top_k / top_p (asr_config.py:78-81; round 4): HF's warpers on the device, one multinomial draw per
        # clip and step from a Philox stream keyed by ``seed`` (a generate() keyword here).  Without one every call draws a FRESH key
        # from torch's global generator, so repeated calls on the same audio give different samples and torch.manual_seed() makes a
        # run reproducible -- the behaviour of HF's sampling, which advances the global RNG
        sampling = None
        if bool(self._generation_setting("do_sample", False, kw)):
            if beams:
                raise ValueError("do_sample=True with beams: beam sampling is not built")
            temp = self._generation_setting("temperature", None, kw)
            top_k = self._generation_setting("top_k", None, kw)
            top_p = self._generation_setting("top_p", None, kw)
            seed = kw.pop("seed", None)
            sampling = (1.0 if temp is None else float(temp), 0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p),
                        int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed))
            if not sampling[0] > 0 or sampling[1] < 0 or not 0 < sampling[2] <= 1:
                raise ValueError("temperature must be > 0, top_k >= 0, 0 < top_p <= 1")
        else:
            for k_ in ("temperature", "top_k", "top_p", "seed"):
                kw.pop(k_, None)
        min_new = int(self._generation_setting("min_new_tokens", 0, kw) or 0)   # HF MinNewTokensLengthLogitsProcessor (round 4)
        # the reference's other two knobs (asr_config.py:84-86): HF logits processors on the device, in front of the argmax
        rep = float(self._generation_setting("repetition_penalty", 1.0, kw))
        ngram = int(self._generation_setting("no_repeat_ngram_size", 0, kw))
        if not beams:
            kw.pop("length_penalty", None)                              # beam-search only: no effect on greedy search
        eos_ids = kw.pop("eos_token_id", None)
        if eos_ids is None:       # <|im_end|> and <|endoftext|> (asr_modeling.py:163-167); the latter is Qwen's pad token
            eos_ids = [self.config.eos_token_id, self.config.pad_token_id]
        eos_ids = [int(e) for e in (eos_ids if isinstance(eos_ids, (list, tuple)) else [eos_ids]) if e is not None]
        pad_id = int(kw.pop("pad_token_id", self.config.pad_token_id))
        options = self._decoding_options(kw, eos_ids, min_new, sampling is not None)
        dev = self.device_
        feats = input_features.to(dev)
        B = feats.shape[0]
        amask = audio_attention_mask.to(dev)
        enc_len = self._compute_encoder_output_lengths(amask)
        counts = self.projector.get_output_length(enc_len).to(device=dev, dtype=torch.int64).contiguous()
        y = self._encode_audio(feats, audio_attention_mask=audio_attention_mask)        # [B, N, D]
        N = y.shape[1]
        if input_ids is None:
            if self.tokenizer is None:
                raise ValueError("input_ids required: no tokenizer is attached to build the chat prompt")
            from .asr_processing import ASRProcessor
            messages = ASRProcessor.build_messages(self._get_num_audio_tokens(amask), None, system_prompt or self.system_prompt)
            input_ids = ASRProcessor.tokenize_messages(self.tokenizer, messages, add_generation_prompt=True)
            if input_ids.shape[0] == 1 and B > 1:
                input_ids = input_ids.expand(B, -1)
            attention_mask = torch.ones_like(input_ids)
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        src_row = ops.audio_index(ids, counts, N, self.audio_token_id)
        return dict(input_ids=ids, src_row=src_row, audio=y.reshape(B * N, -1), attention_mask=attention_mask,
                    max_new_tokens=max_new, eos_ids=eos_ids, pad_id=pad_id, repetition_penalty=rep, no_repeat_ngram_size=ngram,
                    min_new_tokens=min_new, **({} if beams else {"sampling": sampling}), **options)

    def _decoding_options(self, kw, eos_ids, min_new, do_sample):
        """HF's remaining single-hypothesis options, each read from the call's keywords, then from ``self.config``
        (``_generation_setting``), validated with HF's wording -> the decoding-option keywords of ``greedy_decode_iter`` (only those
        that are set: with none, the decode loop gets nothing new).  ``bad_words_ids``, ``sequence_bias`` (both HF forms),
        ``suppress_tokens``, ``begin_suppress_tokens``, ``forced_eos_token_id``, ``exponential_decay_length_penalty``; under
        ``do_sample`` also ``min_p``, ``typical_p``, ``epsilon_cutoff``, ``eta_cutoff`` (HF builds no warper otherwise; neither do we).
        ``renormalize_logits=True`` is accepted and launches nothing: the selection (argmax, or a draw from the softmax) is invariant
        under a per-row shift, and ``ta_token_scores_f32`` already reports normalised log-probabilities."""
        V = int(self.language_model.config.vocab_size)
        get = lambda name: self._generation_setting(name, None, kw)  # noqa: E731
        out = {}
        sb = get("sequence_bias")
        if sb is not None:
            out["sequence_bias"] = ops.normalize_sequence_bias(sb)
            ops.build_sequence_table(out["sequence_bias"], V, "cpu", "sequence_bias")       # the id and limit checks, before any device work
        bw = get("bad_words_ids")
        if bw is not None:
            bad = ops.normalize_bad_words(bw, eos_ids)
            ops.build_sequence_table(bad, V, "cpu", "bad_words_ids")
            if bad:
                out["bad_words"] = bad
        forced = get("forced_eos_token_id")
        if forced is not None:
            out["forced_eos_ids"] = ops.id_list(forced, V, "forced_eos_token_id")
        decay = get("exponential_decay_length_penalty")
        if decay is not None and eos_ids:
            if not isinstance(decay, (tuple, list)) or len(decay) != 2:
                raise ValueError(f"`exponential_decay_length_penalty` has to be a (start_index, decay_factor) pair, but is {decay}")
            check_decay_window(min_new, decay)
            ops.id_list(eos_ids, V, "eos_token_id")
            out["exponential_decay_length_penalty"] = (int(decay[0]), float(decay[1]))
        for name in ("suppress_tokens", "begin_suppress_tokens"):
            v = get(name)
            if v is not None and len(v):
                out[name] = ops.id_list(list(v), V, name)
        wx = ops.check_warp_ext(get("min_p"), get("typical_p"), get("epsilon_cutoff"), get("eta_cutoff"))
        if do_sample and wx != (0.0, 1.0, 0.0, 0.0):
            out["warp_ext"] = wx
        kw.pop("renormalize_logits", None)
        return out

    @staticmethod
    def _check_top_logprobs(top_logprobs) -> int:
        k = int(top_logprobs or 0)
        if not 0 <= k <= ops.MAX_TOP_LOGPROBS:
            raise ValueError(f"top_logprobs must be within [0, {ops.MAX_TOP_LOGPROBS}]; got {top_logprobs}")
        return k

    @torch.no_grad()
    def generate(self, input_ids: Optional[torch.Tensor] = None, input_features: Optional[torch.Tensor] = None,
                 audio_attention_mask: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                 system_prompt: Optional[str] = None, return_token_scores: bool = False, top_logprobs: int = 0, **generate_kwargs):
        """Transcription token ids [B, n_new] (prompt stripped), as ASRModel.generate of the reference
        (tiny_audio/asr_modeling.py:562-646): audio -> encoder -> projector -> <audio> rows of the prompt embeddings ->
        greedy search on the LM (num_beams 1, do_sample False: asr_config.py:103-111), with the
        reference's ``repetition_penalty`` / ``no_repeat_ngram_size`` settings as device-side logits processors.

        ``return_token_scores=True`` and / or ``top_logprobs=k`` (1..8) return a ``GenerationOutput`` instead: the same tokens as
        ``sequences`` plus every token's log-probability and the entropy of the distribution it was chosen from (after the
        processors and warpers), and the k most probable alternatives of every step -- computed by one more row kernel inside the
        decode step; the [B, V] rows themselves are never kept."""
        top_k = self._check_top_logprobs(top_logprobs)
        with _eval_mode(self):
            args = self._prepare_generation(input_ids, input_features, audio_attention_mask, attention_mask, system_prompt,
                                            dict(generate_kwargs))
            if not (return_token_scores or top_k):
                return self.language_model.greedy_decode(**args)
            seq, sc = self.language_model.greedy_decode(**args, token_scores=True, top_logprobs=top_k)
            return GenerationOutput(sequences=seq, **sc)

    @torch.no_grad()
    def generate_beams(self, input_ids: Optional[torch.Tensor] = None, input_features: Optional[torch.Tensor] = None,
                       audio_attention_mask: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                       system_prompt: Optional[str] = None, num_beams: Optional[int] = None, length_penalty: Optional[float] = None,
                       early_stopping=None, num_return_sequences: int = 1, return_beam_trace: bool = False, **generate_kwargs):
        """Beam search: what the reference gets from ``language_model.generate(num_beams=K, ...)`` (``num_beams`` / ``length_penalty``
        of asr_config.py:42,85 and any ``**generate_kwargs``; HF ``GenerationMixin._beam_search``, do_sample False) -- the n-best
        transcripts of every clip with their scores.  ``generate`` keeps raising for ``num_beams > 1`` (its callers rely on one row per
        clip); this is the entry point.

        ``num_beams`` (1..8), ``length_penalty`` and ``early_stopping`` (False, True or "never") are read from the call, then from
        ``self.config``; defaults 1, 1.0, False.  Every logits-processor option of ``generate`` works here (HF applies them to the
        log-probabilities of every beam).  -> ``GenerationOutput(sequences int64 [B * num_return_sequences, n_new], sequences_scores
        f32 [B * num_return_sequences])``: per clip its best ``num_return_sequences <= num_beams`` finished hypotheses, best first,
        padded with ``pad_token_id`` and cropped to the longest.  ``return_beam_trace=True`` -> ``(that output, trace)`` with the
        trace dict of ``Qwen3MI355X.beam_decode`` (every step's candidates, running beams and parents, the final pool and cache).
        ``use_graph=False`` (a keyword) runs every step eagerly instead of replaying the captured one."""
        kw = dict(generate_kwargs)
        K = int(self._generation_setting("num_beams", 1, {"num_beams": num_beams}))
        lp = float(self._generation_setting("length_penalty", 1.0, {"length_penalty": length_penalty}))
        es = self._generation_setting("early_stopping", False, {"early_stopping": early_stopping})
        nrs = int(num_return_sequences)
        if not 1 <= K <= ops.MAX_BEAMS:
            raise ValueError(f"num_beams must be within [1, {ops.MAX_BEAMS}] (the per-clip candidate lists of csrc/beam.hip); got {K}")
        if not 1 <= nrs <= K:
            raise ValueError(f"`num_return_sequences` ({nrs}) has to be smaller or equal to `num_beams` ({K})")
        if es not in (False, True, "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es!r}")
        if kw.pop("return_token_scores", False) or kw.pop("top_logprobs", 0):
            raise ValueError("return_token_scores / top_logprobs are per-token scores of one hypothesis per clip: generate() only; "
                             "generate_beams returns sequences_scores")
        for name in ("num_beam_groups", "constraints", "force_words_ids"):
            v = kw.pop(name, None)
            if v is not None and v != 1:
                raise ValueError(f"{name}: group and constrained beam search are not built")
        with _eval_mode(self):
            args = self._prepare_generation(input_ids, input_features, audio_attention_mask, attention_mask, system_prompt, kw, beams=True)
            if len(args["eos_ids"]) > ops.MAX_BEAM_EOS:
                raise ValueError(f"beam search takes at most {ops.MAX_BEAM_EOS} eos ids; got {args['eos_ids']}")
            use_graph = bool(kw.pop("use_graph", True))
            out = self.language_model.beam_decode(**args, num_beams=K, length_penalty=lp, early_stopping=es, num_return_sequences=nrs,
                                                  use_graph=use_graph, return_trace=bool(return_beam_trace))
            res = GenerationOutput(sequences=out[0], sequences_scores=out[1])
            return (res, out[2]) if return_beam_trace else res

    @torch.no_grad()
    def score(self, input_features: Optional[torch.Tensor] = None, audio_attention_mask: Optional[torch.Tensor] = None, candidates=None, *,
              input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
              system_prompt: Optional[str] = None, append_eos: bool = True, return_token_scores: bool = False):
        """How probable is each given text under the model, given the audio: for clip b and candidate c = (c_0 .. c_{n-1}) the sum over
        t of log_softmax(z(P_b, c_<t))[c_t] -- minus the summed cross-entropy the reference's ``forward(labels=...)`` computes for those
        label positions (tiny_audio/asr_modeling.py:481-533), with P_b exactly the prompt ``generate`` builds (system prompt, user turn
        with the audio placeholders, assistant header) and raw logits (no processor, no temperature).  The audio and the prompt are
        encoded once per clip; the candidates of a clip share its KV cache.

        ``candidates``: one list per clip; an entry is a ``str`` (tokenised with ``add_special_tokens=False``) or a list of token ids;
        the lists are ragged and a clip may have none.  ``append_eos`` appends ``config.eos_token_id`` (``<|im_end|>``: what training
        labels end with).  ValueError: a candidate empty after tokenisation, ids outside the vocabulary, prompt + candidate beyond
        ``max_position_embeddings``.  -> ``ScoreOutput``."""
        from . import scoring
        if candidates is None:
            raise ValueError("candidates required: one list of texts or token-id lists per clip")
        B = int(input_features.shape[0]) if input_features is not None else len(candidates)
        if len(candidates) != B:
            raise ValueError(f"{len(candidates)} candidate lists for {B} clips")
        V = int(self.language_model.config.vocab_size)
        tab = scoring.build_candidate_table(candidates, self.tokenizer, self.config.eos_token_id, append_eos, vocab_size=V)
        with _eval_mode(self):
            args = self._prepare_generation(input_ids, input_features, audio_attention_mask, attention_mask, system_prompt, {})
            L, T = args["input_ids"].shape[1], tab["token_ids"].shape[1]
            if L + T > self.language_model.config.max_position_embeddings:
                raise ValueError(f"prompt ({L}) + candidate tokens ({T}) exceeds max_position_embeddings")
            lp, scores = self.language_model.score_candidates(args["input_ids"], args["src_row"], args["audio"], args["attention_mask"],
                                                              tab["token_ids"], tab["n_tokens"], tab["candidate_clip"], tab["chunks"])
        return ScoreOutput(scores=scores, candidate_clip=tab["candidate_clip"], n_tokens=tab["n_tokens"],
                           token_ids=tab["token_ids"] if return_token_scores else None,
                           token_logprobs=lp if return_token_scores else None, n_clips=B)

    @torch.no_grad()
    def transcribe_long(self, audio, sample_rate: int = 16000, *, max_window_s: float = 28.0, min_window_s: float = 10.0,
                        batch_size: int = 32, return_timestamps: bool = False, acoustic_model=None,
                        system_prompt: Optional[str] = None, vad=None, min_speech_s: float = 0.0, return_speakers: bool = False,
                        speaker_model=None, num_speakers: Optional[int] = None, min_speakers: Optional[int] = None,
                        max_speakers: Optional[int] = None, cluster_device=None, **generate_kwargs):
        """A whole 16 kHz recording -> ``{"text", "chunks": [{"text", "timestamp": (start_s, end_s)}]}`` (``audio``: a 1-D array or
        tensor; a list of them returns a list of results).  The reference keeps a long recording's first chunk only
        (tiny_audio/asr_pipeline.py:243-245); this transcribes all of it, up to 2.9 h per recording (``tiny_audio_amd/longform.py``).

        The recordings are uploaded once.  On the device every 10 ms position is priced as a cut (smoothed short-time power) and the
        cheapest cuts that keep every window within ``min_window_s`` .. ``max_window_s`` are chosen: cuts fall into pauses and never
        beyond the encoder's window (``longform.plan_windows`` returns the plan alone).  The windows are ordered by length, longest
        first (ties in time order), grouped ``batch_size`` at a time, gathered on the device into the feature extractor's padded batch
        and decoded by ``generate``; every window gets its OWN chat prompt with its own ``<audio>`` placeholder count, left-padded
        (with ``input_ids=None`` ``generate`` would build one prompt from the batch maximum).  Every ``generate`` keyword passes
        through (decoding options, ``repetition_penalty``, sampling, ``max_new_tokens``).  Tokens become text through
        ``eval_text.postprocess_tokens``; ``chunks`` are in time order and ``text`` joins the non-empty ones with one space.

        ``return_timestamps=True`` adds ``"words"`` [{'word', 'start', 'end'}]: ``ForcedAligner.align_audio_batch`` with
        ``acoustic_model`` (a ``wav2vec2.Wav2Vec2CtcMI355X``, required) on the same windows in the same groups, shifted by each
        window's start; a window shorter than one acoustic frame (400 samples) or with no text has no words.

        ``vad=`` (a ``vad.DeviceVAD``; opt-in, None changes nothing): the detector runs on the uploaded buffer, the diarizer's hysteresis
        turns its flags into speech segments, every chunk gains ``"speech_s"`` (the seconds of those segments inside the window), and a
        window with ``speech_s <= min_speech_s`` is neither gathered nor decoded nor aligned: its text is ``""`` and it has no words.

        ``return_speakers=True`` (implies ``return_timestamps=True``, as tiny_audio/asr_pipeline.py:100-101; needs ``acoustic_model``,
        ``speaker_model`` -- an ``ecapa.EcapaTdnnMI355X`` -- and ``vad``, each a ``ValueError`` when missing): the same flags feed the
        diarizer on the uploaded buffer (``num_speakers`` / ``min_speakers`` / ``max_speakers`` / ``cluster_device`` as
        ``SpeakerDiarizer.diarize`` takes them), every result gains ``"speaker_segments"`` [{'speaker', 'start', 'end'}] (``[]`` for a
        recording without speech) and every word ``"speaker"`` (None without segments); voting, merging and the words' speakers are one
        launch each for all recordings (``spk_vote``, ``spk_merge``, ``spk_words``)."""
        from .longform import transcribe_long
        with _eval_mode(self):
            return transcribe_long(self, audio, sample_rate, max_window_s=max_window_s, min_window_s=min_window_s, batch_size=batch_size,
                                   return_timestamps=return_timestamps, acoustic_model=acoustic_model, system_prompt=system_prompt,
                                   vad=vad, min_speech_s=min_speech_s, return_speakers=return_speakers, speaker_model=speaker_model,
                                   num_speakers=num_speakers, min_speakers=min_speakers, max_speakers=max_speakers,
                                   cluster_device=cluster_device, **generate_kwargs)

    def generate_streaming(self, input_features: torch.Tensor, audio_attention_mask: torch.Tensor,
                           system_prompt: Optional[str] = None, input_ids: Optional[torch.Tensor] = None,
                           return_token_ids: bool = False, return_token_scores: bool = False, **generate_kwargs) -> Iterator:
        """Partial transcript text, piece by piece, while the clip is still being decoded (ASRModel.generate_streaming,
        tiny_audio/asr_modeling.py:648-760).  The reference runs ``language_model.generate`` on a thread feeding a
        ``TextIteratorStreamer``; here the decode loop itself is a generator (one device sync per token), so no thread
        is needed.  Text is released at word boundaries the way that streamer does (complete lines at once, otherwise
        up to the last space; CJK characters immediately), special tokens are skipped and ``<think>...</think>`` spans
        are dropped (:737-757).  One clip at a time, like the reference's streamer.

        ``return_token_ids=True`` yields the raw int token id of every step instead (no tokenizer needed); with
        ``return_token_scores=True`` as well, ``(token_id, logprob)`` pairs: the id and its log-probability under the processed
        distribution of its step (a float).  The text mode carries no scores."""
        if return_token_scores and not return_token_ids:
            raise ValueError("return_token_scores needs return_token_ids=True: text pieces do not map to single tokens")
        if input_features.shape[0] != 1:
            raise ValueError("generate_streaming handles one clip at a time (TextIteratorStreamer: batch size 1 only)")
        if not return_token_ids and self.tokenizer is None:
            raise ValueError("generate_streaming needs a tokenizer to produce text (or return_token_ids=True)")
        if int(self._generation_setting("num_beams", 1, {"num_beams": generate_kwargs.get("num_beams")})) != 1:
            raise ValueError("generate_streaming does not take num_beams > 1 (HF: a streamer cannot follow beam search); use generate_beams")
        with _eval_mode(self):
            with torch.no_grad():
                args = self._prepare_generation(input_ids, input_features, audio_attention_mask, None, system_prompt,
                                                dict(generate_kwargs))
            eos = set(args["eos_ids"])
            pieces = _TextPieces(self.tokenizer) if not return_token_ids else None
            gate = _ThinkGate()
            # (the reference's streaming call passes inputs_embeds only, so HF's repetition / n-gram processors start from an empty
            # input_ids there and see the generated tokens alone -- generate() passes the prompt ids as well)
            for col in self.language_model.greedy_decode_iter(per_token=True, processors_see_prompt=False,
                                                              token_scores=bool(return_token_scores), **args):
                lp = None
                if return_token_scores:                  # (tokens [1], logprob [1]) per step; the closing item holds a dict
                    col, lp = col
                    if isinstance(lp, dict):
                        break
                if col.dim() != 1:                       # the closing full [B, n_new] tensor
                    break
                tok = int(col[0])
                if return_token_ids:
                    yield (tok, float(lp[0])) if return_token_scores else tok
                    if tok in eos:
                        break
                    continue
                for out in gate.feed(pieces.push(tok)):
                    yield out
                if tok in eos:
                    break
            if pieces is not None:
                for out in gate.feed(pieces.flush()):
                    yield out
                tail = gate.flush()
                if tail:
                    yield tail

"""Configuration of the MI355X-native ASR training path.

Mirrors ``tiny_audio/asr_config.py`` (field names, defaults, the conv length formula at :9-19) without
depending on ``transformers``: sub-configs are plain objects carrying the shape fields the kernels need.
An HF ``GlmAsrEncoderConfig`` / ``WhisperConfig`` / ``Qwen3Config`` / ``SmolLM3Config`` / ``LlamaConfig`` (or a dict) can be passed wherever a sub-config is expected.
"""
from __future__ import annotations

from typing import Optional

# [(padding, kernel, stride), ...]  tiny_audio/asr_config.py:6
DEFAULT_ENCODER_CONV_LAYERS = [(1, 3, 1), (1, 3, 2)]


def compute_encoder_output_length(mel_length, conv_layers=None):
    """tiny_audio/asr_config.py:9-19: (L + 2p - (k-1) - 1) // s + 1 per conv; ints or tensors."""
    layers = conv_layers if conv_layers is not None else DEFAULT_ENCODER_CONV_LAYERS
    length = mel_length
    for padding, kernel_size, stride in layers:
        length = (length + 2 * padding - (kernel_size - 1) - 1) // stride + 1
    return length


def _get(src, names, default=None):
    for n in names:
        if isinstance(src, dict):
            if n in src and src[n] is not None:
                return src[n]
        elif src is not None and getattr(src, n, None) is not None:
            return getattr(src, n)
    return default


class EncoderConfig:
    """GlmAsrEncoderConfig fields (TF:models/glmasr/configuration_glmasr.py:44-61)."""

    def __init__(self, src=None, **kw):
        src = {**(src if isinstance(src, dict) else {}), **kw} if (isinstance(src, dict) or src is None) else src
        self.hidden_size = int(_get(src, ["hidden_size", "hidden"], 1280))
        self.intermediate_size = int(_get(src, ["intermediate_size", "ffn"], 5120))
        self.num_hidden_layers = int(_get(src, ["num_hidden_layers", "layers"], 32))
        self.num_attention_heads = int(_get(src, ["num_attention_heads", "heads"], 20))
        self.num_mel_bins = int(_get(src, ["num_mel_bins", "n_mels"], 128))
        self.max_position_embeddings = int(_get(src, ["max_position_embeddings"], 1500))
        rp = _get(src, ["rope_parameters"], None) or {}
        self.rope_theta = float(_get(src, ["rope_theta"], None) or rp.get("rope_theta", 10000.0))
        self.partial_rotary_factor = float(_get(src, ["partial_rotary_factor", "partial_rotary"], None)
                                           or rp.get("partial_rotary_factor", 0.5))
        self.layer_norm_eps = float(_get(src, ["layer_norm_eps", "ln_eps"], 1e-5))
        if self.hidden_size // self.num_attention_heads != 64 or self.partial_rotary_factor != 0.5:
            raise ValueError("ta355 encoder kernels are built for head_dim 64 with partial rotary 0.5 (GLM-ASR)")


class WhisperEncoderConfig:
    """The encoder half of a WhisperConfig (TF:models/whisper/configuration_whisper.py: d_model, encoder_layers,
    encoder_attention_heads, encoder_ffn_dim, num_mel_bins, max_source_positions), under the attribute names the rest of the
    package reads from ``EncoderConfig``.  ``WhisperEncoder`` uses nn.LayerNorm's default eps (1e-5)."""

    model_type = "whisper"

    def __init__(self, src=None, **kw):
        src = {**(src if isinstance(src, dict) else {}), **kw} if (isinstance(src, dict) or src is None) else src
        self.model_type = "whisper"
        self.hidden_size = int(_get(src, ["d_model", "hidden_size", "hidden"], 384))
        self.intermediate_size = int(_get(src, ["encoder_ffn_dim", "intermediate_size", "ffn"], 4 * self.hidden_size))
        self.num_hidden_layers = int(_get(src, ["encoder_layers", "num_hidden_layers", "layers"], 4))
        self.num_attention_heads = int(_get(src, ["encoder_attention_heads", "num_attention_heads", "heads"], self.hidden_size // 64))
        self.num_mel_bins = int(_get(src, ["num_mel_bins", "n_mels"], 80))
        self.max_source_positions = int(_get(src, ["max_source_positions", "max_position_embeddings"], 1500))
        self.layer_norm_eps = float(_get(src, ["layer_norm_eps", "ln_eps"], 1e-5))
        if self.num_attention_heads <= 0 or self.hidden_size != 64 * self.num_attention_heads:
            raise ValueError("ta355 encoder kernels are built for head_dim 64 (every openai/whisper-* encoder)")

    # the names WhisperConfig itself uses
    d_model = property(lambda self: self.hidden_size)
    encoder_ffn_dim = property(lambda self: self.intermediate_size)
    encoder_layers = property(lambda self: self.num_hidden_layers)
    encoder_attention_heads = property(lambda self: self.num_attention_heads)
    max_position_embeddings = property(lambda self: self.max_source_positions)


# encoder geometry of the public openai/whisper-* checkpoints: (d_model, heads, ffn, layers, mel bins); head_dim is 64 in all of them
WHISPER_GEOMETRY = {"tiny": (384, 6, 1536, 4, 80), "base": (512, 8, 2048, 6, 80), "small": (768, 12, 3072, 12, 80),
                    "medium": (1024, 16, 4096, 24, 80), "large-v3": (1280, 20, 5120, 32, 128), "large": (1280, 20, 5120, 32, 80)}


def whisper_geometry(audio_model_id) -> dict:
    """Shape fields for an ``openai/whisper-<size>[.en|-v2|-v3|-v3-turbo]`` id when no sub-config is passed ({} for an unknown name:
    the class defaults, whisper-tiny, apply)."""
    name = str(audio_model_id or "").lower()
    for key in ("large-v3", "large", "medium", "small", "base", "tiny"):
        if key in name:
            h, nh, f, n, m = WHISPER_GEOMETRY[key]
            return dict(d_model=h, encoder_attention_heads=nh, encoder_ffn_dim=f, encoder_layers=n, num_mel_bins=m)
    return {}


def is_whisper(audio_model_id, audio_config=None) -> bool:
    """The reference's tower rule (tiny_audio/asr_modeling.py:203-237: ``"whisper" in config.audio_model_id.lower()``), extended to a
    passed sub-config that says so itself (``model_type == "whisper"``)."""
    if isinstance(audio_config, WhisperEncoderConfig):
        return True
    if isinstance(audio_config, EncoderConfig):
        return False
    if audio_config is not None:
        return _get(audio_config, ["model_type"], None) == "whisper"
    return "whisper" in str(audio_model_id or "").lower()


# what each supported decoder family fixes: (q/k-norm, defaults vocab / hidden / ffn / layers / heads / kv heads / rope theta / max positions)
LM_FAMILIES = {"qwen3": (True, (151670, 1024, 3072, 28, 16, 8, 1e6, 4096)),            # Qwen3-0.6B (SURVEY.md section 8 preamble)
               "smollm3": (False, (128256, 2048, 11008, 36, 16, 4, 2e6, 32768)),        # SmolLM3Config() = SmolLM3-3B
               "llama": (False, (128256, 2048, 8192, 16, 16, 4, 5e5, 4096))}
MAX_LM_LAYERS = 64      # csrc/api.hip; also the width of ta_lm_weights.nope_layers


def _has(src, name):
    """True when ``src`` (dict or object) carries ``name`` and it is truthy."""
    return bool(_get(src, [name], False))


class LMConfig:
    """The decoder's shape fields, from a Qwen3Config / SmolLM3Config / LlamaConfig (or a dict, or keyword arguments); defaults =
    Qwen3-0.6B (SURVEY.md section 8 preamble).  ``model_type`` picks the family:

    * ``qwen3``: per-head q_norm / k_norm before RoPE (``qk_norm``), every layer rotates;
    * ``smollm3``: no q/k-norm; ``no_rope_layers[i] == 0`` switches RoPE off in layer i ("NoPE"), from the source or derived from
      ``no_rope_layer_interval`` as TF:models/smollm3/configuration_smollm3.py derives it; defaults = ``SmolLM3Config()``;
    * ``llama``: no q/k-norm, every layer rotates.

    What the kernels do not do is refused here with a ValueError that names the field."""

    def __init__(self, src=None, **kw):
        src = {**(src if isinstance(src, dict) else {}), **kw} if (isinstance(src, dict) or src is None) else src
        self.model_type = str(_get(src, ["model_type"], "qwen3"))
        if self.model_type not in LM_FAMILIES:
            raise ValueError(f"model_type {self.model_type!r}: the text tower is one of {sorted(LM_FAMILIES)}")
        qk_norm, (V, D, F, NL, NH, NKV, theta, max_pos) = LM_FAMILIES[self.model_type]
        self.vocab_size = int(_get(src, ["vocab_size", "vocab"], V))
        self.hidden_size = int(_get(src, ["hidden_size", "hidden"], D))
        self.intermediate_size = int(_get(src, ["intermediate_size", "ffn"], F))
        self.num_hidden_layers = int(_get(src, ["num_hidden_layers", "layers"], NL))
        self.num_attention_heads = int(_get(src, ["num_attention_heads", "heads"], NH))
        self.num_key_value_heads = int(_get(src, ["num_key_value_heads", "kv_heads"], NKV))
        # Qwen3Config always carries head_dim (128 in every published size); SmolLM3 / Llama configs derive it
        self.head_dim = int(_get(src, ["head_dim"], 128 if self.model_type == "qwen3" else self.hidden_size // self.num_attention_heads))
        self.rms_norm_eps = float(_get(src, ["rms_norm_eps", "rms_eps"], 1e-6))
        rp = _get(src, ["rope_parameters"], None) or {}
        self.rope_theta = float(_get(src, ["rope_theta"], None) or rp.get("rope_theta", theta))
        self.max_position_embeddings = int(_get(src, ["max_position_embeddings"], max_pos))
        self.qk_norm = qk_norm
        nrl = _get(src, ["no_rope_layers"], None) if self.model_type == "smollm3" else None
        if nrl is None:
            every = int(_get(src, ["no_rope_layer_interval"], 4)) if self.model_type == "smollm3" else 0
            nrl = [int(every == 0 or (i + 1) % every != 0) for i in range(self.num_hidden_layers)]   # configuration_smollm3.py __post_init__
        self.no_rope_layers = [int(bool(v)) for v in list(nrl)[: self.num_hidden_layers]]
        if len(self.no_rope_layers) != self.num_hidden_layers:
            raise ValueError(f"no_rope_layers has {len(self.no_rope_layers)} entries for num_hidden_layers = {self.num_hidden_layers}")
        if self.head_dim != 128:
            raise ValueError(f"head_dim = {self.head_dim}: ta355 LM kernels are built for head_dim 128 (Qwen3, SmolLM3-3B)")
        if self.num_hidden_layers > MAX_LM_LAYERS:
            raise ValueError(f"num_hidden_layers = {self.num_hidden_layers}: at most {MAX_LM_LAYERS} decoder layers")
        if self.model_type != "qwen3":          # (a Qwen3 source is read exactly as before: its extra fields are not looked at)
            for name in ("attention_bias", "mlp_bias", "use_sliding_window"):
                if _has(src, name):
                    raise ValueError(f"{name} = True is not built (the LM linears carry no bias, every layer attends to the whole prefix)")
            rope_type = rp.get("rope_type", rp.get("type", "default")) if isinstance(rp, dict) else "default"
            rs = _get(src, ["rope_scaling"], None)
            if isinstance(rs, dict):
                rope_type = rs.get("rope_type", rs.get("type", rope_type))
            if rope_type not in (None, "default"):
                raise ValueError(f"rope_type = {rope_type!r}: only the default rotary embedding is built (no llama3 / yarn scaling)")
            if _get(src, ["tie_word_embeddings"], True) is False:
                raise ValueError("tie_word_embeddings = False is not built (lm_head is the embedding matrix)")

    @property
    def nope_mask(self) -> int:
        """ta_lm_weights.nope_layers: bit l set = layer l does not rotate."""
        return sum(1 << i for i, v in enumerate(self.no_rope_layers) if not v)


def smollm3_geometry(text_model_id) -> dict:
    """Sub-config fields for a ``HuggingFaceTB/SmolLM3-*`` id when no ``text_config`` is passed ({} for any other name: Qwen3)."""
    return {"model_type": "smollm3"} if "smollm3" in str(text_model_id or "").lower() else {}


class ASRConfig:
    """Same knobs as the reference ASRConfig (tiny_audio/asr_config.py:36-220); unknown kwargs are kept as
    attributes (the reference lets e.g. ``router_z_loss_coef`` / ``router_jitter_noise`` ride along that way)."""

    model_type = "asr_model"

    def __init__(self, audio_model_id: str = "zai-org/GLM-ASR-Nano-2512", text_model_id: str = "Qwen/Qwen3-0.6B",
                 attn_implementation: str = "ta355", model_dtype: str = "bfloat16",
                 system_prompt: str = "You are a helpful assistant.", encoder_dim: Optional[int] = None,
                 llm_dim: Optional[int] = None, encoder_conv_layers: Optional[list] = None,
                 audio_sample_rate: int = 16000, projector_pool_stride: int = 4, downsample_rate: int = 5,
                 projector_hidden_dim: Optional[int] = None, projector_type: str = "mlp",
                 audio_token_dropout: float = 0.0, num_experts: int = 4, num_experts_per_tok: int = 2,
                 router_aux_loss_coef: float = 0.01, use_lora: bool = False, lora_rank: int = 8, lora_alpha: int = 32,
                 lora_dropout: float = 0.0, lora_target_modules: Optional[list] = None, freeze_projector: bool = False,
                 freeze_language_model: bool = True, max_new_tokens: int = 128, audio_config=None, text_config=None,
                 audio_token_id: int = 151669, pad_token_id: int = 151643, eos_token_id: int = 151645,
                 label_smoothing: float = 0.0, lm_z_loss_coef: float = 0.0, **kwargs):
        self.audio_model_id = audio_model_id
        self.text_model_id = text_model_id
        self.attn_implementation = attn_implementation
        self.model_dtype = model_dtype
        self.system_prompt = system_prompt
        self.encoder_conv_layers = encoder_conv_layers or DEFAULT_ENCODER_CONV_LAYERS
        self.audio_sample_rate = audio_sample_rate
        self.projector_pool_stride = projector_pool_stride
        self.downsample_rate = downsample_rate
        self.projector_hidden_dim = projector_hidden_dim
        self.projector_type = projector_type
        self.audio_token_dropout = audio_token_dropout
        self.num_experts = num_experts
        self.num_experts_per_tok = num_experts_per_tok
        self.router_aux_loss_coef = router_aux_loss_coef
        self.use_lora = use_lora
        self.lora_rank = lora_rank
        self.lora_alpha = lora_alpha
        self.lora_dropout = lora_dropout
        self.lora_target_modules = lora_target_modules or ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj",
                                                            "up_proj", "down_proj"]
        self.freeze_projector = freeze_projector
        self.freeze_language_model = freeze_language_model
        self.max_new_tokens = max_new_tokens
        # LM loss options (not in the reference's config: HF has label_smoothing_factor on TrainingArguments, where a stock Trainer
        # smooths on the full logits): label smoothing and the coefficient of logsumexp^2, both inside the cross-entropy launch
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1); got {label_smoothing}")
        if not float(lm_z_loss_coef) >= 0.0:
            raise ValueError(f"lm_z_loss_coef must be >= 0; got {lm_z_loss_coef}")
        self.label_smoothing = float(label_smoothing)
        self.lm_z_loss_coef = float(lm_z_loss_coef)
        if isinstance(audio_config, (EncoderConfig, WhisperEncoderConfig)):
            self.audio_config = audio_config
        elif is_whisper(audio_model_id, audio_config):
            self.audio_config = WhisperEncoderConfig(audio_config if audio_config is not None else whisper_geometry(audio_model_id))
        else:
            self.audio_config = EncoderConfig(audio_config)
        if isinstance(text_config, LMConfig):
            self.text_config = text_config
        else:       # an explicit sub-config decides by its own model_type; without one the model id does (the whisper_geometry pattern)
            self.text_config = LMConfig(text_config if text_config is not None else smollm3_geometry(text_model_id))
        self.encoder_dim = encoder_dim or self.audio_config.hidden_size      # asr_modeling.py:259-265
        self.llm_dim = llm_dim or self.text_config.hidden_size               # asr_modeling.py:267-273
        self.audio_token_id = audio_token_id
        self.pad_token_id = pad_token_id
        self.eos_token_id = eos_token_id
        for k, v in kwargs.items():
            setattr(self, k, v)

    def to_dict(self):
        d = {k: v for k, v in self.__dict__.items() if k not in ("audio_config", "text_config")}
        d["audio_config"] = dict(self.audio_config.__dict__)
        d["text_config"] = dict(self.text_config.__dict__)
        return d

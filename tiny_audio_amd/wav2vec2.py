"""Frozen wav2vec2-base CTC acoustic model on MI355X: waveforms -> log-softmax emissions, the front half of forced alignment.

The reference's ``ForcedAligner.align`` (tiny_audio/alignment.py:182-211) runs torchaudio's ``WAV2VEC2_ASR_BASE_960H`` bundle through
PyTorch, one clip at a time, and takes ``log_softmax`` of its output.  ``Wav2Vec2CtcMI355X`` computes the same emissions for a ragged
batch in one call (``ta_wav2vec2_forward``, csrc/wav2vec2.hip), every clip as if alone, and leaves them on the device in the layout
``torch.ops.ta355.ctc_align`` takes.

Reference module: ``Wav2Vec2ForCTC`` (TF:models/wav2vec2/modeling_wav2vec2.py:1597-1700) with ``feat_extract_norm="group"``,
``conv_bias=False``, ``do_stable_layer_norm=False`` -- the settings of ``facebook/wav2vec2-base-960h`` and of torchaudio's bundle --
no attention mask and no input normalisation.  Inference only.  tests/wav2vec2_ref.py is the float64 definition.

The second family -- ``feat_extract_norm="layer"``, ``conv_bias=True``, ``do_stable_layer_norm=True``: wav2vec2-large-960h-lv60(-self),
the XLSR-53 / XLS-R 300M fine-tunes, MMS 300M and torchaudio's ``MMS_FA`` -- is the same class with those three config fields set
(``Wav2Vec2CtcConfig.from_hf`` reads them from a ``Wav2Vec2Config`` dict): ``ta_wav2vec2_sln_forward``, defined by
tests/wav2vec2_sln_ref.py, with the optional zero-mean / unit-variance input (``normalize_input``).  ``set_vocab`` gives the model the
checkpoint's own alphabet, which ``ForcedAligner`` then tokenises against instead of the English ``LABELS``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .ops import BF16, F32, ptr, stream

CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
POS_KERNEL, POS_GROUPS = 128, 16
SLN_CONV_DIMS = (64, 128, 256, 512)               # ta_w2v_conv0_ln_gelu: a lane owns conv_dim / 64 in {1, 2, 4, 8} channels
INPUT_NORM_EPS = {"hf": 1e-7, "torchaudio": 1e-5}  # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm / torchaudio's layer_norm(waveform, waveform.shape)
HEAD_PAD = 64                                    # TA_W2V_HEAD_PAD
MIN_SAMPLES = 400                                # the receptive field of one frame
Q_SCALE = (64 ** -0.5) * math.log2(math.e)       # softmax scale and log2(e), folded into the q rows (the attention kernel runs in base 2)
TORCHAUDIO_DROPPED = (1, 2, 3)                   # <s>, </s>, <unk> of the HF vocabulary: torchaudio's bundle removes these head rows

_HF_PREFIX = "wav2vec2."
# ta_enc_layer field <- Wav2Vec2EncoderLayer parameter (TF:models/wav2vec2/modeling_wav2vec2.py:575-608)
_LAYER_NAMES = (("ln1_w", "layer_norm.weight"), ("ln1_b", "layer_norm.bias"), ("ln2_w", "final_layer_norm.weight"),
                ("ln2_b", "final_layer_norm.bias"), ("bo", "attention.out_proj.bias"), ("b1", "feed_forward.intermediate_dense.bias"),
                ("b2", "feed_forward.output_dense.bias"))


@dataclass
class Wav2Vec2CtcConfig:
    """Geometry of the model; the defaults are wav2vec2-base-960h with torchaudio's 29 labels."""
    hidden_size: int = 768
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    conv_dim: int = 512
    n_classes: int = 29
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"             # "group" (base) | "layer" (large-lv60 / XLSR / XLS-R / MMS)
    conv_bias: bool = False
    do_stable_layer_norm: bool = False
    normalize_input: str | None = None           # None | "hf" (eps 1e-7) | "torchaudio" (eps 1e-5): zero mean / unit variance per clip

    @property
    def sln(self) -> bool:
        """The layer-norm / stable family (``ta_wav2vec2_sln_forward``) instead of the base model (``ta_wav2vec2_forward``)."""
        return self.feat_extract_norm == "layer"

    @classmethod
    def from_hf(cls, config, n_classes: int | None = None, normalize_input="auto"):
        """A ``Wav2Vec2Config``-style dict (``config.json``, or ``config.to_dict()``) -> the config, refusing by name what is not
        built.  ``n_classes`` defaults to ``vocab_size``.  ``normalize_input="auto"``: "hf" for the layer-norm family (whose
        checkpoints are published with ``do_normalize=true`` in their preprocessor config), None for the base model; the
        preprocessor config is not part of this dict, so pass the value when a checkpoint differs."""
        c = dict(config)
        if c.get("adapter_attn_dim") is not None:
            raise ValueError("adapter_attn_dim is set: MMS adapter layers are not built")
        fen = c.get("feat_extract_norm", "group")
        conv_dim = tuple(c.get("conv_dim", (512,) * 7))
        if len(set(conv_dim)) != 1 or len(conv_dim) != 7:
            raise ValueError(f"conv_dim {conv_dim}: seven conv layers of one width are built")
        if tuple(c.get("conv_kernel", CONV_KERNEL)) != CONV_KERNEL or tuple(c.get("conv_stride", CONV_STRIDE)) != CONV_STRIDE:
            raise ValueError(f"conv_kernel / conv_stride other than {CONV_KERNEL} / {CONV_STRIDE} are not built")
        if c.get("num_conv_pos_embeddings", POS_KERNEL) != POS_KERNEL or c.get("num_conv_pos_embedding_groups", POS_GROUPS) != POS_GROUPS:
            raise ValueError(f"the positional conv is built for {POS_KERNEL} taps in {POS_GROUPS} groups")
        for k in ("hidden_act", "feat_extract_activation"):
            if c.get(k, "gelu") != "gelu":
                raise ValueError(f"{k}={c[k]!r}: only gelu is built")
        if c.get("add_adapter"):
            raise ValueError("add_adapter is set: the convolutional adapter is not built")
        if normalize_input == "auto":
            normalize_input = "hf" if fen == "layer" else None
        return cls(hidden_size=int(c.get("hidden_size", 768)), num_attention_heads=int(c.get("num_attention_heads", 12)),
                   intermediate_size=int(c.get("intermediate_size", 3072)), num_hidden_layers=int(c.get("num_hidden_layers", 12)),
                   conv_dim=int(conv_dim[0]), n_classes=int(n_classes if n_classes is not None else c.get("vocab_size", 32)),
                   layer_norm_eps=float(c.get("layer_norm_eps", 1e-5)), feat_extract_norm=fen, conv_bias=bool(c.get("conv_bias", False)),
                   do_stable_layer_norm=bool(c.get("do_stable_layer_norm", False)), normalize_input=normalize_input)

    def __post_init__(self):
        if self.feat_extract_norm not in ("group", "layer"):
            raise ValueError(f'feat_extract_norm must be "group" or "layer", not {self.feat_extract_norm!r}')
        if self.sln != bool(self.do_stable_layer_norm):
            raise ValueError(f'feat_extract_norm="{self.feat_extract_norm}" with do_stable_layer_norm={bool(self.do_stable_layer_norm)}: '
                             'this mixed configuration is not built (no published checkpoint has it)')
        if self.sln != bool(self.conv_bias):
            raise ValueError(f'feat_extract_norm="{self.feat_extract_norm}" with conv_bias={bool(self.conv_bias)} is not built')
        if self.normalize_input not in (None, "hf", "torchaudio"):
            raise ValueError(f'normalize_input must be None, "hf" or "torchaudio", not {self.normalize_input!r}')
        if self.normalize_input is not None and not self.sln:
            raise ValueError('normalize_input is built for feat_extract_norm="layer" models only')
        if self.sln and self.conv_dim not in SLN_CONV_DIMS:
            raise ValueError(f'feat_extract_norm="layer": conv_dim must be one of {SLN_CONV_DIMS}')
        H, cg = self.hidden_size, self.hidden_size // POS_GROUPS
        if self.num_attention_heads <= 0 or H != 64 * self.num_attention_heads:
            raise ValueError("ta355 encoder kernels are built for head_dim 64 (XLS-R 1B / 2B have 80 and 120)")
        if H % 128 or self.intermediate_size % 128:
            raise ValueError("hidden_size and intermediate_size must be multiples of 128")
        if H % POS_GROUPS or cg % 8 or cg > 64:
            raise ValueError(f"{cg} channels per positional-conv group: the kernel takes multiples of 8 up to 64")
        if self.conv_dim <= 0 or self.conv_dim % 64:
            raise ValueError("conv_dim must be a multiple of 64")
        if not 1 <= self.n_classes <= HEAD_PAD:
            raise ValueError(f"n_classes must be in 1 .. {HEAD_PAD}: vocabularies above {HEAD_PAD} classes are not built")


def frames_of(num_samples: int) -> int:
    """Emission frames of a clip: ``(T - k) // s + 1`` through the seven convolutions, ((L - 400) // 320) + 1 for L >= 400, else 0."""
    T = int(num_samples)
    for k, s in zip(CONV_KERNEL, CONV_STRIDE):
        T = (T - k) // s + 1 if T >= k else 0
    return T


FRAME_HOP = 320                                  # samples between two emission frames: the product of CONV_STRIDE
SAMPLE_RATE = 16000


def long_windows(n_samples: int, window: int, context: int) -> list[tuple[int, int, int, int]]:
    """The window table of ``emissions_long``, in samples: -> [(s0, s1, f0, f1)], window i being the slice ``wave[s0:s1]`` that is
    run through the model and whose frames with GLOBAL index in [f0, f1) are kept.  Pure host arithmetic.

    * Global frame f reads samples [320 f, 320 f + 400); a recording has T = (n_samples - 400) // 320 + 1 of them.
    * ``window`` is rounded down to a multiple of 320 (at least 320), so window i owns the samples from i * window on and the frames
      [i * window / 320, (i + 1) * window / 320) that start inside it, cut at T: the spans tile [0, T) exactly once.
    * The slice is the window's own frames' samples extended by ``context`` (rounded down to a multiple of 320) on both sides where
      audio exists.  s0 is a multiple of 320, so the slice's frame grid is the global one: its local frame f - s0 / 320 is global f.
    * A last window with fewer than 400 samples of its own holds no whole frame: it is merged into the window before it, whose right
      context reaches over its samples as far as ``context`` allows.
    * A recording of at most one window gives the one entry (0, n_samples, 0, T): the whole recording, no context arithmetic.
    A recording shorter than 400 samples has no frame and gives no window."""
    n, T = int(n_samples), frames_of(int(n_samples))
    if T <= 0:
        return []
    wf = max(int(window) // FRAME_HOP, 1)
    ctx = max(int(context), 0) // FRAME_HOP * FRAME_HOP
    if T <= wf:
        return [(0, n, 0, T)]
    out = []
    for f0 in range(0, T, wf):
        f1 = min(f0 + wf, T)
        out.append((max(0, f0 * FRAME_HOP - ctx), min(n, (f1 - 1) * FRAME_HOP + MIN_SAMPLES + ctx), f0, f1))
    return out


def fold_weight_norm(g, v) -> torch.Tensor:
    """``weight_norm(conv, dim=2)``: w[:, :, tap] = g[tap] * v[:, :, tap] / ||v[:, :, tap]||_F  (g is [1, 1, k])."""
    g, v = torch.as_tensor(g).to(torch.float64), torch.as_tensor(v).to(torch.float64)
    return (v * (g.reshape(1, 1, -1) / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())).to(F32)


def rename_torchaudio(sd) -> dict:
    """torchaudio ``Wav2Vec2Model.state_dict()`` names -> transformers' ``Wav2Vec2ForCTC`` names.  The torchaudio side is written
    from torchaudio's published module layout (``feature_extractor.conv_layers.N.conv.weight``, ``encoder.feature_projection.*``,
    ``encoder.transformer.pos_conv_embed.conv.weight_g|weight_v``, ``encoder.transformer.layers.N.*``, ``aux.*``); torchaudio is not
    installed where this package is tested, so these names have NOT been checked against a real bundle.  The layer-norm family's extra
    parameters (``feature_extractor.conv_layers.N.layer_norm.*``, ``feature_extractor.conv_layers.N.conv.bias``,
    ``encoder.transformer.layer_norm.*``) go through the same prefix rules and are just as unchecked."""
    out = {}
    for k, v in sd.items():
        if k.startswith("aux."):
            out["lm_head." + k[4:]] = v
        elif k.startswith("feature_extractor."):
            out[_HF_PREFIX + k] = v
        elif k.startswith("encoder.feature_projection."):
            out[_HF_PREFIX + k[len("encoder."):]] = v
        elif k.startswith("encoder.transformer."):
            out[_HF_PREFIX + "encoder." + k[len("encoder.transformer."):]] = v
        else:
            raise KeyError(f"unexpected torchaudio wav2vec2 parameter {k!r}")
    return out


def _strip(sd) -> dict:
    return {(k[len(_HF_PREFIX):] if k.startswith(_HF_PREFIX) else k): v for k, v in sd.items()}


def head_rows(n_rows: int, labels: str):
    """Rows of ``lm_head`` that are kept, in order: all of them (``"hf"``) or all but 1, 2, 3 (``"torchaudio"``: the 29 classes of
    ``alignment.LABELS`` out of the 32-entry HF vocabulary, blank staying at 0)."""
    if labels == "hf":
        return list(range(n_rows))
    if labels == "torchaudio":
        if n_rows != 32:
            raise ValueError(f'labels="torchaudio" maps the 32-class HF head, this one has {n_rows} classes')
        return [i for i in range(n_rows) if i not in TORCHAUDIO_DROPPED]
    raise ValueError(f'labels must be "hf" or "torchaudio", not {labels!r}')


def pack_pos_conv(w: torch.Tensor) -> torch.Tensor:
    """Plain positional-conv weight [H, cg, 128] -> the image ``ta_w2v_pos_conv`` reads: bf16 [16][NB * 16][128 * cg], row = output
    channel inside its group (rows >= cg zero), column = tap * cg + cin."""
    H, cg, K = w.shape
    nb = (cg + 15) // 16
    img = torch.zeros(POS_GROUPS, nb * 16, K * cg, dtype=F32)
    img[:, :cg] = w.reshape(POS_GROUPS, cg, cg, K).permute(0, 1, 3, 2).reshape(POS_GROUPS, cg, K * cg)
    return img.to(BF16).contiguous()


def pack_state_dict(sd, config: Wav2Vec2CtcConfig, labels: str = "hf"):
    """``Wav2Vec2ForCTC.state_dict()`` -> the images ``ta_wav2vec2_weights`` / ``ta_enc_layer`` point to, as CPU tensors (matrices
    bf16, vectors and conv 0 fp32).  Pure tensor arithmetic: no device, no library."""
    sd = _strip(sd)
    H, L, Cd, F = config.hidden_size, config.num_hidden_layers, config.conv_dim, config.intermediate_size
    g = lambda k: torch.as_tensor(sd[k]).detach().to(F32).cpu()
    b = {}
    fe = "feature_extractor.conv_layers."
    c0 = g(fe + "0.conv.weight")
    if tuple(c0.shape) != (Cd, 1, CONV_KERNEL[0]):
        raise ValueError(f"conv_layers.0.conv.weight is {tuple(c0.shape)}, the config says {(Cd, 1, CONV_KERNEL[0])}")
    if not config.sln and any((fe + f"{i}.conv.bias") in sd for i in range(7)):
        raise ValueError("conv_bias=True checkpoints are not supported (wav2vec2-base has none)")
    b["conv0_w"] = c0.reshape(Cd, CONV_KERNEL[0]).contiguous()
    if config.sln:
        for i in range(7):                                           # Wav2Vec2LayerNormConvLayer: bias, LayerNorm(C) on every layer
            for f, k in (("b", "conv.bias"), ("ln_w", "layer_norm.weight"), ("ln_b", "layer_norm.bias")):
                if fe + f"{i}.{k}" not in sd:
                    raise ValueError(f'feat_extract_norm="layer" needs conv_layers.{i}.{k}')
                b[f"conv{i}_{f}"] = g(fe + f"{i}.{k}").contiguous()
                if tuple(b[f"conv{i}_{f}"].shape) != (Cd,):
                    raise ValueError(f"conv_layers.{i}.{k} is {tuple(b[f'conv{i}_{f}'].shape)}, the config says {(Cd,)}")
    else:
        b["gn_w"], b["gn_b"] = g(fe + "0.layer_norm.weight"), g(fe + "0.layer_norm.bias")
    for i in range(1, 7):
        w = g(fe + f"{i}.conv.weight")
        if tuple(w.shape) != (Cd, Cd, CONV_KERNEL[i]):
            raise ValueError(f"conv_layers.{i}.conv.weight is {tuple(w.shape)}, the config says {(Cd, Cd, CONV_KERNEL[i])}")
        b[f"conv{i}_w"] = w.permute(0, 2, 1).reshape(Cd, CONV_KERNEL[i] * Cd).to(BF16).contiguous()      # col = tap * C + cin
    b["fp_ln_w"], b["fp_ln_b"] = g("feature_projection.layer_norm.weight"), g("feature_projection.layer_norm.bias")
    b["fp_w"], b["fp_b"] = g("feature_projection.projection.weight").to(BF16).contiguous(), g("feature_projection.projection.bias")
    pc = "encoder.pos_conv_embed.conv."
    if pc + "parametrizations.weight.original0" in sd:
        pw = fold_weight_norm(g(pc + "parametrizations.weight.original0"), g(pc + "parametrizations.weight.original1"))
    elif pc + "weight_g" in sd:
        pw = fold_weight_norm(g(pc + "weight_g"), g(pc + "weight_v"))
    else:
        pw = g(pc + "weight")
    if tuple(pw.shape) != (H, H // POS_GROUPS, POS_KERNEL):
        raise ValueError(f"pos_conv_embed weight is {tuple(pw.shape)}, the config says {(H, H // POS_GROUPS, POS_KERNEL)}")
    b["pos_w_plain"] = pw.to(BF16).contiguous()                     # kept for export_state_dict_hf (never read by the kernels)
    b["pos_w"] = pack_pos_conv(pw)
    b["pos_b"] = g(pc + "bias")
    b["enc_ln_w"], b["enc_ln_b"] = g("encoder.layer_norm.weight"), g("encoder.layer_norm.bias")
    for i in range(L):
        p, a = f"layers.{i}.", f"encoder.layers.{i}.attention."
        wq, wk, wv = g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight")
        bq, bk, bv = g(a + "q_proj.bias"), g(a + "k_proj.bias"), g(a + "v_proj.bias")
        b[p + "wqkv"] = torch.cat([wq, wk, wv], 0).to(BF16).contiguous()              # kept for export (never read by the kernels)
        b[p + "bqkv"] = torch.cat([bq, bk, bv], 0).contiguous()
        # scaled from the fp32 master: one rounding to bf16
        b[p + "wqkv_fa"] = torch.cat([(wq * Q_SCALE).to(BF16), wk.to(BF16), wv.to(BF16)], 0).contiguous()
        b[p + "bqkv_fa"] = torch.cat([bq * Q_SCALE, bk, bv], 0).contiguous()
        b[p + "wo"] = g(a + "out_proj.weight").to(BF16).contiguous()
        b[p + "w1"] = g(f"encoder.layers.{i}.feed_forward.intermediate_dense.weight").to(BF16).contiguous()
        b[p + "w2"] = g(f"encoder.layers.{i}.feed_forward.output_dense.weight").to(BF16).contiguous()
        if tuple(b[p + "w1"].shape) != (F, H):
            raise ValueError(f"intermediate_dense.weight is {tuple(b[p + 'w1'].shape)}, the config says {(F, H)}")
        for f, k in _LAYER_NAMES:
            b[p + f] = g(f"encoder.layers.{i}." + k).contiguous()
    hw, hb = g("lm_head.weight"), g("lm_head.bias")
    rows = head_rows(hw.shape[0], labels)
    if len(rows) != config.n_classes:
        raise ValueError(f"lm_head gives {len(rows)} classes with labels={labels!r}, the config says {config.n_classes}")
    img = torch.zeros(HEAD_PAD, H, dtype=F32)
    img[:len(rows)] = hw[rows]
    b["head_w"] = img.to(BF16).contiguous()
    b["head_b"] = hb[rows].contiguous()
    return b


def random_state_dict(config: Wav2Vec2CtcConfig, seed: int = 0) -> dict:
    """A seeded ``Wav2Vec2ForCTC``-named state dict at the configured shapes (O(1 / sqrt(fan_in)) matrices, perturbed norm gains)."""
    gen = torch.Generator().manual_seed(seed)
    H, F, Cd, NC = config.hidden_size, config.intermediate_size, config.conv_dim, config.n_classes
    cg = H // POS_GROUPS
    rn = lambda *s, std=1.0: torch.randn(*s, generator=gen, dtype=F32) * std
    sd = {}
    fe = "wav2vec2.feature_extractor.conv_layers."
    sd[fe + "0.conv.weight"] = rn(Cd, 1, 10, std=1 / math.sqrt(10))
    sd[fe + "0.layer_norm.weight"], sd[fe + "0.layer_norm.bias"] = 1 + rn(Cd, std=0.1), rn(Cd, std=0.02)
    for i in range(1, 7):
        sd[fe + f"{i}.conv.weight"] = rn(Cd, Cd, CONV_KERNEL[i], std=math.sqrt(2.0 / (CONV_KERNEL[i] * Cd)))
    if config.sln:                                                   # (drawn only here: the base model's draws keep their order)
        for i in range(7):
            sd[fe + f"{i}.conv.bias"] = rn(Cd, std=0.05)
            if i:
                sd[fe + f"{i}.layer_norm.weight"], sd[fe + f"{i}.layer_norm.bias"] = 1 + rn(Cd, std=0.1), rn(Cd, std=0.02)
    fp = "wav2vec2.feature_projection."
    sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"] = 1 + rn(Cd, std=0.1), rn(Cd, std=0.02)
    sd[fp + "projection.weight"], sd[fp + "projection.bias"] = rn(H, Cd, std=1 / math.sqrt(Cd)), rn(H, std=0.02)
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    v = rn(H, cg, POS_KERNEL, std=1 / math.sqrt(cg * POS_KERNEL))
    sd[pc + "parametrizations.weight.original1"] = v
    sd[pc + "parametrizations.weight.original0"] = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1 + rn(1, 1, POS_KERNEL, std=0.1))
    sd[pc + "bias"] = rn(H, std=0.02)
    sd["wav2vec2.encoder.layer_norm.weight"], sd["wav2vec2.encoder.layer_norm.bias"] = 1 + rn(H, std=0.1), rn(H, std=0.02)
    for i in range(config.num_hidden_layers):
        p = f"wav2vec2.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj"):
            sd[p + f"attention.{n}.weight"], sd[p + f"attention.{n}.bias"] = rn(H, H, std=1 / math.sqrt(H)), rn(H, std=0.02)
        sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"] = rn(H, H, std=0.5 / math.sqrt(H)), rn(H, std=0.02)
        sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"] = rn(F, H, std=1 / math.sqrt(H)), rn(F, std=0.02)
        sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"] = rn(H, F, std=0.5 / math.sqrt(F)), rn(H, std=0.02)
        for n in ("layer_norm", "final_layer_norm"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + rn(H, std=0.1), rn(H, std=0.02)
    sd["lm_head.weight"], sd["lm_head.bias"] = rn(NC, H, std=4 / math.sqrt(H)), rn(NC, std=0.1)
    return sd


def _as_clips(waveforms, lengths):
    """-> (list of 1-D float32 CPU/device tensors or None, padded [B, Ls] tensor or None, lengths list)."""
    if isinstance(waveforms, (list, tuple)):
        if lengths is not None:
            raise ValueError("lengths is for a padded [B, Ls] tensor; a list of clips carries its own lengths")
        clips = [torch.as_tensor(np.ascontiguousarray(w)) if isinstance(w, np.ndarray) else w for w in waveforms]
        for w in clips:
            if w.dim() != 1:
                raise ValueError(f"every clip must be 1-D, got {tuple(w.shape)}")
        return clips, None, [int(w.shape[0]) for w in clips]
    w = torch.as_tensor(np.ascontiguousarray(waveforms)) if isinstance(waveforms, np.ndarray) else waveforms
    if w.dim() == 1:
        if lengths is not None:
            raise ValueError("lengths is for a padded [B, Ls] tensor")
        return [w], None, [int(w.shape[0])]
    if w.dim() != 2:
        raise ValueError(f"waveforms must be a list of 1-D clips or a padded [B, Ls] tensor, got {tuple(w.shape)}")
    if lengths is None:
        lens = [int(w.shape[1])] * int(w.shape[0])
    else:
        lens = [int(x) for x in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        if len(lens) != w.shape[0]:
            raise ValueError(f"{len(lens)} lengths for {w.shape[0]} clips")
        if any(n > w.shape[1] for n in lens):
            raise ValueError(f"a length exceeds the padded width {w.shape[1]}")
    return None, w, lens


class Wav2Vec2CtcMI355X(torch.nn.Module):
    """``model(waveforms) -> (emissions f32 [sum T, n_classes] on the device, frames per clip)``: log-softmax CTC emissions of
    16 kHz clips, clip b at rows ``sum(frames[:b]) .. sum(frames[:b + 1])``."""

    def __init__(self, config: Wav2Vec2CtcConfig | None = None, device="cuda"):
        super().__init__()
        self.config = config if config is not None else Wav2Vec2CtcConfig()
        self.device_ = torch.device(device)
        self._bufs = {}
        self._layers_arr = None
        self._w = None
        self._ws = None
        self._last = None
        self._res_f32 = False
        self.labels = None                           # set_vocab: the class names by id, {character: id}, the CTC blank's id
        self.dictionary = None
        self.blank_id = 0

    def set_vocab(self, vocab: dict, blank_token: str = "<pad>", word_delimiter: str = "|"):
        """The checkpoint's own alphabet (``vocab.json``: {token: id}) -> ``labels`` (tokens by id), ``dictionary`` and ``blank_id``,
        which ``ForcedAligner`` then uses instead of ``alignment.LABELS`` and 0.  The ids must be 0 .. n_classes - 1, each once.
        ``word_delimiter`` is the token a space is aligned to; the dictionary also answers to "|" for it."""
        ids = sorted(int(i) for i in vocab.values())
        if ids != list(range(self.config.n_classes)):
            raise ValueError(f"the vocabulary must give the ids 0 .. {self.config.n_classes - 1} once each (n_classes), got {len(ids)} entries")
        for name, tok in (("blank_token", blank_token), ("word_delimiter", word_delimiter)):
            if tok not in vocab:
                raise ValueError(f"{name} {tok!r} is not in the vocabulary")
        by_id = {int(i): t for t, i in vocab.items()}
        self.labels = tuple(by_id[i] for i in range(len(ids)))
        self.dictionary = {t: int(i) for t, i in vocab.items()}
        self.dictionary["|"] = int(vocab[word_delimiter])
        self.blank_id = int(vocab[blank_token])
        return self

    @property
    def res_f32(self) -> bool:
        """Storage of the residual stream (ta_wav2vec2_weights.res_f32): fp32 or bf16, as the other towers' ``res_f32``."""
        return self._res_f32

    @res_f32.setter
    def res_f32(self, v):
        self._res_f32 = bool(v)
        if self._w is not None:
            self._w.res_f32 = int(self._res_f32)

    # ------------------------------------------------------------------ weights
    def load_state_dict_hf(self, sd, labels: str = "hf"):
        """sd: {``Wav2Vec2ForCTC`` parameter name: array-like}; the positional conv's weight norm may come as
        ``parametrizations.weight.original0|1``, as the older ``weight_g|weight_v``, or already folded (``weight``).
        ``labels="torchaudio"`` drops rows 1, 2, 3 of a 32-class head: the 29 classes of ``alignment.LABELS``, blank 0."""
        self._bufs = {k: v.to(self.device_) for k, v in pack_state_dict(sd, self.config, labels).items()}
        self._finalize()
        return self

    def load_state_dict_torchaudio(self, sd):
        """sd: ``torchaudio.pipelines.WAV2VEC2_ASR_BASE_960H.get_model().state_dict()``; renamed (``rename_torchaudio``) and packed
        like an HF one.  torchaudio is not installed where this package is tested: the torchaudio-side names are written from its
        published module layout and are unchecked against a real bundle -- the layer-norm family's (``MMS_FA``,
        ``WAV2VEC2_ASR_LARGE_LV60K_960H``: ``conv_layers.N.layer_norm.*``, ``conv_layers.N.conv.bias``,
        ``encoder.transformer.layer_norm.*``) included."""
        return self.load_state_dict_hf(rename_torchaudio(sd), labels="hf")

    def random_init(self, seed=0):
        """Seeded random weights at the configured shapes (``random_state_dict``)."""
        return self.load_state_dict_hf(random_state_dict(self.config, seed))

    def _finalize(self):
        c, b = self.config, self._bufs
        L = c.num_hidden_layers
        arr = (_lib.EncLayer * max(L, 1))()
        for i in range(L):
            p = f"layers.{i}."
            for f, _ in _lib.EncLayer._fields_:
                setattr(arr[i], f, b[p + f].data_ptr() if (p + f) in b else None)
        geom = dict(hidden=c.hidden_size, ffn=c.intermediate_size, n_layers=L, heads=c.num_attention_heads, conv_dim=c.conv_dim,
                    n_classes=c.n_classes, ln_eps=c.layer_norm_eps, res_f32=int(self._res_f32))
        if c.sln:
            w = _lib.Wav2Vec2SlnWeights(input_norm_eps=INPUT_NORM_EPS.get(c.normalize_input, 0.0), **geom)
            for i in range(7):
                w.conv_b[i], w.conv_ln_w[i], w.conv_ln_b[i] = (b[f"conv{i}_{f}"].data_ptr() for f in ("b", "ln_w", "ln_b"))
        else:
            w = _lib.Wav2Vec2Weights(**geom)
            w.gn_w, w.gn_b = b["gn_w"].data_ptr(), b["gn_b"].data_ptr()
        for f in ("conv0_w", "fp_ln_w", "fp_ln_b", "fp_w", "fp_b", "pos_w", "pos_b", "enc_ln_w", "enc_ln_b",
                  "head_w", "head_b"):
            setattr(w, f, b[f].data_ptr())
        for i in range(6):
            w.conv_w[i] = b[f"conv{i + 1}_w"].data_ptr()
        w.layers = C.cast(arr, C.POINTER(_lib.EncLayer))
        self._layers_arr, self._w = arr, w

    def export_state_dict_hf(self):
        """Back to ``Wav2Vec2ForCTC.state_dict()`` names as fp32 numpy (matrices carry their bf16 rounding).  The positional conv
        comes out as ``weight_g`` / ``weight_v`` with v = the folded weight and g = its per-tap norm, which folds to itself; the
        head has the classes this module keeps."""
        c, b = self.config, self._bufs
        H, Cd = c.hidden_size, c.conv_dim
        f = lambda t: t.detach().float().cpu().numpy()
        fe, fp, pc = "wav2vec2.feature_extractor.conv_layers.", "wav2vec2.feature_projection.", "wav2vec2.encoder.pos_conv_embed.conv."
        sd = {fe + "0.conv.weight": f(b["conv0_w"]).reshape(Cd, 1, CONV_KERNEL[0])}
        if c.sln:
            for i in range(7):
                sd[fe + f"{i}.conv.bias"] = f(b[f"conv{i}_b"])
                sd[fe + f"{i}.layer_norm.weight"], sd[fe + f"{i}.layer_norm.bias"] = f(b[f"conv{i}_ln_w"]), f(b[f"conv{i}_ln_b"])
        else:
            sd[fe + "0.layer_norm.weight"], sd[fe + "0.layer_norm.bias"] = f(b["gn_w"]), f(b["gn_b"])
        for i in range(1, 7):
            sd[fe + f"{i}.conv.weight"] = f(b[f"conv{i}_w"].float().reshape(Cd, CONV_KERNEL[i], Cd).permute(0, 2, 1).contiguous())
        sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"] = f(b["fp_ln_w"]), f(b["fp_ln_b"])
        sd[fp + "projection.weight"], sd[fp + "projection.bias"] = f(b["fp_w"]), f(b["fp_b"])
        pw = b["pos_w_plain"].float()
        sd[pc + "weight_v"], sd[pc + "weight_g"] = f(pw), f(pw.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
        sd[pc + "bias"] = f(b["pos_b"])
        sd["wav2vec2.encoder.layer_norm.weight"], sd["wav2vec2.encoder.layer_norm.bias"] = f(b["enc_ln_w"]), f(b["enc_ln_b"])
        for i in range(c.num_hidden_layers):
            p, q = f"layers.{i}.", f"wav2vec2.encoder.layers.{i}."
            w, bq = f(b[p + "wqkv"]), f(b[p + "bqkv"])
            for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
                sd[q + f"attention.{n}.weight"], sd[q + f"attention.{n}.bias"] = w[j * H:(j + 1) * H], bq[j * H:(j + 1) * H]
            sd[q + "attention.out_proj.weight"] = f(b[p + "wo"])
            sd[q + "feed_forward.intermediate_dense.weight"], sd[q + "feed_forward.output_dense.weight"] = f(b[p + "w1"]), f(b[p + "w2"])
            for fld, k in _LAYER_NAMES:
                sd[q + k] = f(b[p + fld])
        sd["lm_head.weight"], sd["lm_head.bias"] = f(b["head_w"][:c.n_classes]), f(b["head_b"])
        return sd

    # ------------------------------------------------------------------ forward
    def _pad(self, waveforms, lengths):
        clips, padded, lens = _as_clips(waveforms, lengths)
        short = [n for n in lens if n < MIN_SAMPLES]
        if short:
            raise ValueError(f"a clip of {short[0]} samples is shorter than the {MIN_SAMPLES} samples one wav2vec2 frame needs")
        if padded is not None:
            return padded.to(device=self.device_, dtype=F32).contiguous(), lens
        if len(clips) == 1:
            return clips[0].to(device=self.device_, dtype=F32).reshape(1, -1).contiguous(), lens
        wav = torch.zeros((len(clips), max(lens)), device=self.device_, dtype=F32)
        for i, w in enumerate(clips):
            wav[i, :lens[i]] = w.to(device=self.device_, dtype=F32)
        return wav, lens

    @torch.no_grad()
    def forward(self, waveforms, lengths=None, *, normalized: bool = False):
        """waveforms: a list of 1-D tensors / arrays (16 kHz, any lengths >= 400), or a padded [B, Ls] tensor with ``lengths``.
        -> (emissions f32 [sum T, n_classes], frames per clip as a list).  A clip shorter than 400 samples raises ``ValueError``.
        With ``config.normalize_input`` every clip is brought to zero mean and unit variance over its own samples first;
        ``normalized=True`` says the caller has done that already (``emissions_long``: the whole recording's statistics)."""
        from . import torch_ops
        if isinstance(waveforms, (list, tuple)) and len(waveforms) == 0:
            return torch.empty((0, self.config.n_classes), device=self.device_, dtype=F32), []
        wav, lens = self._pad(waveforms, lengths)
        if self.config.sln:
            em = torch.ops.ta355.wav2vec2_sln_emissions(wav, lens, bool(normalized), torch_ops.register_module(self))
        else:
            em = torch.ops.ta355.wav2vec2_emissions(wav, lens, torch_ops.register_module(self))
        return em, [frames_of(n) for n in lens]

    @torch.no_grad()
    def emissions_long(self, wave, window_s: float = 30.0, context_s: float = 2.0, batch_windows: int = 16):
        """One 16 kHz recording of any length -> emissions f32 [T, n_classes] on the device, T = (len - 400) // 320 + 1, for
        ``ForcedAligner.align_long``.  GroupNorm and attention are global over a clip, so an hour in one ``forward`` is not sensible:
        the recording is cut by ``long_windows`` into windows of ``window_s`` seconds that start on the global frame grid, each is
        extended by ``context_s`` seconds on both sides where audio exists and run through ``forward`` as one clip of a ragged batch
        (``batch_windows`` windows per call), and only the frames of a window's own span are kept.  This is the usual windowed
        approximation of the full-context model, not its value.  A recording no longer than one window is one ``forward`` call.
        With ``config.normalize_input`` the statistics are those of the WHOLE recording, taken once (``ops.w2v_input_norm``) and
        applied to every window, so the emissions do not depend on where the windows fall."""
        w = torch.as_tensor(np.ascontiguousarray(wave)) if isinstance(wave, np.ndarray) else wave
        if w.dim() == 2 and w.shape[0] == 1:
            w = w[0]
        if w.dim() != 1:
            raise ValueError(f"emissions_long takes one 1-D recording, got {tuple(w.shape)}")
        if w.shape[0] < MIN_SAMPLES:
            raise ValueError(f"a clip of {w.shape[0]} samples is shorter than the {MIN_SAMPLES} samples one wav2vec2 frame needs")
        if window_s <= 0 or context_s < 0 or batch_windows < 1:
            raise ValueError("emissions_long: window_s > 0, context_s >= 0 and batch_windows >= 1")
        table = long_windows(w.shape[0], int(round(window_s * SAMPLE_RATE)), int(round(context_s * SAMPLE_RATE)))
        if len(table) == 1:
            return self.forward([w])[0]
        w = w.to(device=self.device_, dtype=F32)
        prenorm = self.config.normalize_input is not None
        if prenorm:
            w = ops.w2v_input_norm(w.reshape(1, -1).contiguous(), torch.tensor([w.shape[0]], dtype=torch.int32, device=self.device_),
                                   INPUT_NORM_EPS[self.config.normalize_input])[0]
        out = torch.empty((table[-1][3], self.config.n_classes), device=self.device_, dtype=F32)
        for i in range(0, len(table), int(batch_windows)):
            group = table[i:i + int(batch_windows)]
            em, Ts = self.forward([w[s0:s1] for s0, s1, _, _ in group], normalized=prenorm)
            row = 0
            for (s0, _, f0, f1), t in zip(group, Ts):
                lo = row + f0 - s0 // FRAME_HOP
                out[f0:f1] = em[lo:lo + f1 - f0]
                row += t
        return out

    def _forward_impl(self, wav, lens, out=None, normalized=False):
        """wav f32 [B, Ls] on the device, lens: Python ints -> emissions [sum T, n_classes] (written into ``out`` when given: a
        contiguous f32 tensor of at least that many rows, whose further rows are left alone).  ``normalized``: skip the input
        normalisation of a ``normalize_input`` model for this call."""
        if self._w is None:
            raise _lib.Ta355Error("wav2vec2 weights not loaded (load_state_dict_hf / load_state_dict_torchaudio / random_init)")
        wav = wav.to(device=self.device_, dtype=F32).contiguous()
        B, Ls = wav.shape
        lens = [int(n) for n in lens]
        if len(lens) != B or any(n < MIN_SAMPLES or n > Ls for n in lens):
            raise ValueError(f"lengths {lens} do not fit a [{B}, {Ls}] waveform tensor ({MIN_SAMPLES} <= length <= {Ls})")
        frames = np.asarray([frames_of(n) for n in lens], np.int32)
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum(frames)
        rows, NC = int(cu[-1]), self.config.n_classes
        lens_host = np.asarray(lens, np.int32)
        lens_dev, cu_dev = torch.from_numpy(lens_host).to(self.device_), torch.from_numpy(cu).to(self.device_)
        sln = self.config.sln
        ws_bytes, fwd = (("ta_wav2vec2_sln_workspace_bytes", "ta_wav2vec2_sln_forward") if sln else
                         ("ta_wav2vec2_workspace_bytes", "ta_wav2vec2_forward"))
        if sln:
            self._w.input_norm_eps = 0.0 if normalized else INPUT_NORM_EPS.get(self.config.normalize_input, 0.0)
        n = getattr(_lib.lib(), ws_bytes)(C.byref(self._w), B, Ls, rows)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, device=self.device_, dtype=torch.uint8)
        if out is None:
            out = torch.empty((rows, NC), device=self.device_, dtype=F32)
        elif out.dtype != F32 or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != NC or out.shape[0] < rows:
            raise ValueError(f"out must be a contiguous f32 [>= {rows}, {NC}] tensor")
        _lib.check(getattr(_lib.lib(), fwd)(C.byref(self._w), ptr(wav), lens_host.ctypes.data_as(C.c_void_p), ptr(lens_dev),
                                            ptr(cu_dev), B, Ls, ptr(out), ptr(self._ws), self._ws.numel(), stream()), fwd)
        self._last = (n, rows, B, Ls)
        return out[:rows]

    def state_of_last_call(self, which: str):
        """Layer-norm family, for the per-stage tests: ``"feat"`` -> the feature extractor's output bf16 [rows, conv_dim];
        ``"stream"`` -> the residual stream behind the last layer [rows, hidden] in its dtype (behind the positional-conv add for
        a model of no layers), read from the workspace of the latest forward (``ta_wav2vec2_sln_ws_offsets``)."""
        n, rows, B, Ls = self._last
        feat, strm = C.c_long(0), C.c_long(0)
        _lib.check(_lib.lib().ta_wav2vec2_sln_ws_offsets(C.byref(self._w), B, Ls, rows, C.byref(feat), C.byref(strm)), "ta_wav2vec2_sln_ws_offsets")
        if which == "feat":
            Cd = self.config.conv_dim
            return self._ws[feat.value:feat.value + rows * Cd * 2].view(BF16).reshape(rows, Cd)
        if which == "stream":
            H, dt = self.config.hidden_size, (F32 if self._res_f32 else BF16)
            return self._ws[strm.value:strm.value + rows * H * dt.itemsize].view(dt).reshape(rows, H)
        raise ValueError(f'which must be "feat" or "stream", not {which!r}')

    def logits_of_last_call(self):
        """The lm_head logits [rows, n_classes] (bias added) of the latest forward, read back from the tail of the workspace where
        ``ta_wav2vec2_forward`` leaves the head GEMM's output (include/ta355.h): what the parity tests measure."""
        n, rows = self._last[:2]
        tail = (rows * HEAD_PAD * 4 + 255) // 256 * 256
        raw = self._ws[n - tail:n - tail + rows * HEAD_PAD * 4].view(F32).reshape(rows, HEAD_PAD)
        return raw[:, :self.config.n_classes] + self._bufs["head_b"]

"""Frozen Whisper audio encoder on MI355X: the reference's other ``audio_tower`` (tiny_audio/asr_modeling.py:203-237 loads
``WhisperModel.from_pretrained(id).encoder`` for every ``openai/whisper-*`` id and keeps the feature extractor's 3000-frame padding).

Reference module: ``WhisperEncoder`` TF:models/whisper/modeling_whisper.py:540-650.  Relative to ``GlmAsrEncoderMI355X`` the stem, the
layer arithmetic and the final LayerNorm are the same kernels (``ta_whisper_encoder_forward`` shares the layer loop of
``ta_encoder_forward``); there is no rotary embedding -- ``embed_positions.weight`` is added once behind the stem (``ta_pos_add``) --
and the input must be exactly ``2 * max_source_positions`` frames.  ``load_state_dict_hf`` takes ``WhisperEncoder.state_dict()`` names,
bare or under the ``model.encoder.`` / ``encoder.`` prefix of a ``WhisperForConditionalGeneration`` / ``WhisperModel`` checkpoint.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .asr_config import WhisperEncoderConfig
from .encoder import BaseModelOutput
from .ops import BF16, F32, ptr, stream

_PREFIXES = ("model.encoder.", "encoder.")
# ta_enc_layer field <- WhisperEncoderLayer parameter (TF:models/whisper/modeling_whisper.py:365-377)
_LAYER_NAMES = (("ln1_w", "self_attn_layer_norm.weight"), ("ln1_b", "self_attn_layer_norm.bias"),
                ("ln2_w", "final_layer_norm.weight"), ("ln2_b", "final_layer_norm.bias"),
                ("bo", "self_attn.out_proj.bias"), ("b1", "fc1.bias"), ("b2", "fc2.bias"))
Q_SCALE = (64 ** -0.5) * math.log2(math.e)      # softmax scale and log2(e), folded into the q rows (ta_attention_enc_fwd runs in base 2)


def sinusoids(length: int, channels: int, max_timescale: float = 10000.0) -> torch.Tensor:
    """The table ``WhisperEncoder`` initialises ``embed_positions`` with (TF:models/whisper/modeling_whisper.py:55-64): [sin | cos]."""
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2))
    t = torch.arange(length).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1).to(F32)


def strip_prefix(sd):
    """``WhisperEncoder`` names from a bare state dict or a ``WhisperModel`` / ``WhisperForConditionalGeneration`` one (decoder and
    head tensors are dropped)."""
    out = {}
    for k, v in sd.items():
        for p in _PREFIXES:
            if k.startswith(p):
                out[k[len(p):]] = v
                break
        else:
            if not k.startswith(("model.", "decoder.", "proj_out.")):
                out[k] = v
    return out


def conv1_k(n_mels: int) -> int:
    """Columns of the packed conv1 image: 3 * n_mels rounded up to the GEMM's 64-wide K tile (240 -> 256)."""
    return (3 * n_mels + 63) // 64 * 64


def pack_state_dict(sd, config: WhisperEncoderConfig):
    """``WhisperEncoder.state_dict()`` -> the images ``ta_whisper_encoder_weights`` / ``ta_enc_layer`` point to, as CPU tensors
    (matrices bf16, vectors fp32).  Pure tensor arithmetic: no device, no library."""
    sd = strip_prefix(sd)
    H, L, M = config.hidden_size, config.num_hidden_layers, config.num_mel_bins
    g = lambda k: torch.as_tensor(sd[k]).detach().to(F32).cpu()
    b = {}
    c1 = g("conv1.weight").permute(0, 2, 1).reshape(H, 3 * M)                         # col = tap * n_mels + cin
    b["conv1_w"] = torch.cat([c1, torch.zeros(H, conv1_k(M) - 3 * M)], 1).to(BF16).contiguous()
    b["conv1_b"] = g("conv1.bias")
    b["conv2_w"] = g("conv2.weight").permute(0, 2, 1).reshape(H, 3 * H).to(BF16).contiguous()
    b["conv2_b"] = g("conv2.bias")
    b["pos_emb"] = g("embed_positions.weight").contiguous()
    if tuple(b["pos_emb"].shape) != (config.max_source_positions, H):
        raise ValueError(f"embed_positions.weight is {tuple(b['pos_emb'].shape)}, the config says {(config.max_source_positions, H)}")
    b["norm_w"], b["norm_b"] = g("layer_norm.weight"), g("layer_norm.bias")
    for i in range(L):
        p, a = f"layers.{i}.", f"layers.{i}.self_attn."
        wq, wk, wv = g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight")
        bq, bv = g(a + "q_proj.bias"), g(a + "v_proj.bias")
        b[p + "wqkv"] = torch.cat([wq, wk, wv], 0).to(BF16).contiguous()              # kept for export_state_dict_hf (never read by the kernels)
        b[p + "bqkv"] = torch.cat([bq, torch.zeros(H), bv], 0).contiguous()
        # scaled from the fp32 master: one rounding to bf16, like the reference's own cast
        b[p + "wqkv_fa"] = torch.cat([(wq * Q_SCALE).to(BF16), wk.to(BF16), wv.to(BF16)], 0).contiguous()
        b[p + "bqkv_fa"] = torch.cat([bq * Q_SCALE, torch.zeros(H), bv], 0).contiguous()
        b[p + "wo"] = g(a + "out_proj.weight").to(BF16).contiguous()
        b[p + "w1"] = g(p + "fc1.weight").to(BF16).contiguous()
        b[p + "w2"] = g(p + "fc2.weight").to(BF16).contiguous()
        for f, k in _LAYER_NAMES:
            b[p + f] = g(p + k).contiguous()
    return b


class WhisperEncoderMI355X(torch.nn.Module):
    """``encoder(input_features=[B, n_mels, 3000] f32).last_hidden_state -> [B, 1500, H]`` (bf16 by default)."""

    def __init__(self, config: WhisperEncoderConfig, device="cuda"):
        super().__init__()
        self.config = config
        self.device_ = torch.device(device)
        self._bufs = {}
        self._layers_arr = None
        self._w = None
        self._ws = None
        self._ws_key = None
        self.out_dtype = BF16
        self._res_f32 = False

    @property
    def res_f32(self) -> bool:
        """Storage of the residual stream (ta_whisper_encoder_weights.res_f32): fp32 or bf16, as ``GlmAsrEncoderMI355X.res_f32``."""
        return self._res_f32

    @res_f32.setter
    def res_f32(self, v):
        self._res_f32 = bool(v)
        if self._w is not None:
            self._w.res_f32 = int(self._res_f32)

    # ------------------------------------------------------------------ weights
    def load_state_dict_hf(self, sd):
        """sd: {``WhisperEncoder`` parameter name (optionally ``model.encoder.`` / ``encoder.`` prefixed): array-like}."""
        self._bufs = {k: v.to(self.device_) for k, v in pack_state_dict(sd, self.config).items()}
        self._finalize()
        return self

    @torch.no_grad()
    def random_init(self, seed=0):
        """Seeded random weights generated on the device at the configured shapes; the position table is the sinusoidal one
        ``WhisperEncoder`` starts from (and every released checkpoint keeps: the table is frozen)."""
        c, dev = self.config, self.device_
        H, F, M, L = c.hidden_size, c.intermediate_size, c.num_mel_bins, c.num_hidden_layers
        gen = torch.Generator(device=dev); gen.manual_seed(seed)
        rn = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=gen, dtype=F32) * std
        b = self._bufs = {}
        c1 = rn(H, 3 * M, std=1 / math.sqrt(3 * M))
        b["conv1_w"] = torch.cat([c1, torch.zeros(H, conv1_k(M) - 3 * M, device=dev)], 1).to(BF16).contiguous()
        b["conv1_b"] = rn(H, std=0.02)
        b["conv2_w"] = rn(H, 3 * H, std=1 / math.sqrt(3 * H)).to(BF16)
        b["conv2_b"] = rn(H, std=0.02)
        b["pos_emb"] = sinusoids(c.max_source_positions, H).to(dev)
        b["norm_w"] = 1 + rn(H, std=0.1); b["norm_b"] = rn(H, std=0.02)
        for i in range(L):
            p = f"layers.{i}."
            w = rn(3 * H, H, std=1 / math.sqrt(H))
            bq = rn(3 * H, std=0.02); bq[H:2 * H] = 0
            b[p + "wqkv"], b[p + "bqkv"] = w.to(BF16), bq
            b[p + "wqkv_fa"] = torch.cat([(w[:H] * Q_SCALE).to(BF16), w[H:].to(BF16)], 0).contiguous()
            b[p + "bqkv_fa"] = torch.cat([bq[:H] * Q_SCALE, bq[H:]], 0).contiguous()
            b[p + "wo"] = rn(H, H, std=0.5 / math.sqrt(H)).to(BF16); b[p + "bo"] = rn(H, std=0.02)
            b[p + "w1"] = rn(F, H, std=1 / math.sqrt(H)).to(BF16); b[p + "b1"] = rn(F, std=0.02)
            b[p + "w2"] = rn(H, F, std=0.5 / math.sqrt(F)).to(BF16); b[p + "b2"] = rn(H, std=0.02)
            b[p + "ln1_w"] = 1 + rn(H, std=0.1); b[p + "ln1_b"] = rn(H, std=0.02)
            b[p + "ln2_w"] = 1 + rn(H, std=0.1); b[p + "ln2_b"] = rn(H, std=0.02)
        self._finalize()
        return self

    def _finalize(self):
        c, b = self.config, self._bufs
        L = c.num_hidden_layers
        arr = (_lib.EncLayer * L)()
        for i in range(L):
            p = f"layers.{i}."
            for f, _ in _lib.EncLayer._fields_:
                setattr(arr[i], f, b[p + f].data_ptr() if (p + f) in b else None)
        w = _lib.WhisperEncoderWeights(hidden=c.hidden_size, ffn=c.intermediate_size, n_layers=L, heads=c.num_attention_heads,
                                       n_mels=c.num_mel_bins, max_pos=c.max_source_positions, ln_eps=c.layer_norm_eps,
                                       res_f32=int(self._res_f32))
        for f in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "pos_emb", "norm_w", "norm_b"):
            setattr(w, f, b[f].data_ptr())
        w.layers = C.cast(arr, C.POINTER(_lib.EncLayer))
        self._layers_arr, self._w = arr, w

    def export_state_dict_hf(self):
        """Back to ``WhisperEncoder.state_dict()`` names as fp32 numpy (matrices carry their bf16 rounding)."""
        c, b = self.config, self._bufs
        H, M = c.hidden_size, c.num_mel_bins
        f = lambda t: t.detach().float().cpu().numpy()
        sd = {"conv1.weight": f(b["conv1_w"][:, :3 * M].float().reshape(H, 3, M).permute(0, 2, 1).contiguous()),
              "conv1.bias": f(b["conv1_b"]),
              "conv2.weight": f(b["conv2_w"].float().reshape(H, 3, H).permute(0, 2, 1).contiguous()),
              "conv2.bias": f(b["conv2_b"]), "embed_positions.weight": f(b["pos_emb"]),
              "layer_norm.weight": f(b["norm_w"]), "layer_norm.bias": f(b["norm_b"])}
        for i in range(c.num_hidden_layers):
            p, a = f"layers.{i}.", f"layers.{i}.self_attn."
            w, bq = f(b[p + "wqkv"]), f(b[p + "bqkv"])
            sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"] = w[:H], w[H:2 * H], w[2 * H:]
            sd[a + "q_proj.bias"], sd[a + "v_proj.bias"] = bq[:H], bq[2 * H:]
            sd[a + "out_proj.weight"] = f(b[p + "wo"])
            sd[p + "fc1.weight"], sd[p + "fc2.weight"] = f(b[p + "w1"]), f(b[p + "w2"])
            for fld, k in _LAYER_NAMES:
                sd[p + k] = f(b[p + fld])
        return sd

    # ------------------------------------------------------------------ forward
    def output_length(self, T):
        return (T - 1) // 2 + 1

    def _check_length(self, input_features):
        """WhisperEncoder.forward's own check (TF:models/whisper/modeling_whisper.py:612-616), before any device work."""
        expected = 2 * self.config.max_source_positions
        if input_features.shape[-1] != expected:
            raise ValueError(f"Whisper expects the mel input features to be of length {expected}, but found "
                             f"{input_features.shape[-1]}. Make sure to pad the input mel features to {expected}.")

    @torch.no_grad()
    def forward(self, input_features, frame_keep=None, return_f32=False, **_):
        """model.audio_tower(input_features=...).last_hidden_state through torch.ops.ta355.whisper_encoder_forward."""
        self._check_length(input_features)
        from . import torch_ops
        x = input_features.to(device=self.device_, dtype=F32)
        if frame_keep is not None:
            frame_keep = frame_keep.to(device=self.device_, dtype=F32).contiguous()
        return BaseModelOutput(torch.ops.ta355.whisper_encoder_forward(x, frame_keep, torch_ops.register_module(self), bool(return_f32)))

    def _forward_impl(self, input_features, frame_keep=None, return_f32=False):
        self._check_length(input_features)
        if self._w is None:
            raise _lib.Ta355Error("encoder weights not loaded (load_state_dict_hf / random_init)")
        x = input_features.to(device=self.device_, dtype=F32).contiguous()
        B, _, T = x.shape
        S, H = self.output_length(T), self.config.hidden_size
        key = (B, T)
        if self._ws_key != key:
            n = _lib.lib().ta_whisper_encoder_workspace_bytes(C.byref(self._w), B, T)
            self._ws = torch.empty(n, device=self.device_, dtype=torch.uint8)
            self._ws_key = key
        out_b = torch.empty((B, S, H), device=self.device_, dtype=BF16)
        out_f = torch.empty((B, S, H), device=self.device_, dtype=F32) if return_f32 else None
        if frame_keep is not None:
            frame_keep = frame_keep.to(device=self.device_, dtype=F32).contiguous()
        _lib.check(_lib.lib().ta_whisper_encoder_forward(C.byref(self._w), ptr(x), B, T, ptr(frame_keep), ptr(out_b), ptr(out_f),
                                                         ptr(self._ws), self._ws.numel(), stream()), "ta_whisper_encoder_forward")
        return out_f if return_f32 else out_b

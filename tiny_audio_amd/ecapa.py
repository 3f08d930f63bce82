"""Frozen ECAPA-TDNN speaker-embedding model on MI355X: windows of 16 kHz audio -> one embedding per window, the hot path of
speaker diarization.

The reference's ``LocalSpeakerDiarizer._extract_embeddings`` (tiny_audio/diarization.py:457-517) cuts every speech segment into
0.75 s windows 0.15 s apart, reflect-pads the short ones and pushes each through SpeechBrain's ``spkrec-ecapa-voxceleb``
``encode_batch`` -- one window per call.  ``EcapaTdnnMI355X.embed_windows`` uploads the audio once and computes every window's
embedding in one call (``ta_ecapa_forward``, csrc/ecapa.hip), each window as if alone.

Reference module: the published ECAPA-TDNN (Desplanques et al. 2020) at SpeechBrain's ``spkrec-ecapa-voxceleb`` hyper-parameters
behind its ``Fbank`` (n_fft 400, hop 160, Hamming, 80 mel, top_db 80) and sentence-mean normalisation.  SpeechBrain is not installed
where this package is tested: the architecture, the Fbank constants, the ReLU-then-BatchNorm order and the checkpoint's key names are
restated from the publication and from SpeechBrain's published module layout ("Speaker diarization", lists
them as recalled, not pinned).  Inference only.  tests/ecapa_ref.py is the float64 definition.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .ops import BF16, F32, ptr, stream

N_FFT, HOP, N_BINS, N_MELS = 400, 160, 201, 80
FEAT_STRIDE = 128                                # TA_ECAPA_FEAT_STRIDE
SCALE = 8                                        # TA_ECAPA_SCALE: Res2Net sub-bands
MIN_T, MAX_T = 5, 512                            # TA_ECAPA_MIN_T / TA_ECAPA_MAX_T
MAX_DILATION, MAX_CHANNELS, MAX_SE, MAX_ATTN, MAX_EMB = 4, 1024, 256, 256, 1024
SAMPLE_RATE = 16000
DEFAULT_CHUNK = 512                              # windows per pass of the composite: about 2.4 MB of workspace per 76-frame window; one
                                                 # Res2Net workgroup per window, so a chunk should hold a few windows per CU (profiles/diarization.md)
_BN = ("weight", "bias", "running_mean", "running_var")


@dataclass
class EcapaConfig:
    """Geometry of the model; the defaults are speechbrain/spkrec-ecapa-voxceleb."""
    channels: int = 1024
    se_channels: int = 128
    attention_channels: int = 128
    lin_neurons: int = 192
    dilations: tuple = (2, 3, 4)
    bn_eps: float = 1e-5

    def __post_init__(self):
        self.dilations = tuple(int(d) for d in self.dilations)
        if self.channels < 128 or self.channels > MAX_CHANNELS or self.channels % 128:
            raise ValueError(f"channels must be a multiple of 128 up to {MAX_CHANNELS} (Res2Net sub-bands of 16 .. 128 channels in steps of 16)")
        if not 1 <= self.se_channels <= MAX_SE:
            raise ValueError(f"se_channels must be in 1 .. {MAX_SE}")
        if self.attention_channels % 64 or not 64 <= self.attention_channels <= MAX_ATTN:
            raise ValueError(f"attention_channels must be a multiple of 64 up to {MAX_ATTN}")
        if self.lin_neurons % 4 or not 4 <= self.lin_neurons <= MAX_EMB:
            raise ValueError(f"lin_neurons must be a multiple of 4 up to {MAX_EMB}")
        if len(self.dilations) != 3 or any(d < 1 or d > MAX_DILATION for d in self.dilations):
            raise ValueError(f"dilations must be three values in 1 .. {MAX_DILATION}")

    @property
    def width(self) -> int:
        return self.channels // SCALE


def frames_of(num_samples: int) -> int:
    """Frames of a window: the centred STFT gives ``L // 160 + 1``."""
    return int(num_samples) // HOP + 1


def check_window_samples(window_samples: int) -> int:
    T = frames_of(window_samples)
    if window_samples < 1 or T < MIN_T or T > MAX_T:
        raise ValueError(f"a window of {window_samples} samples is {T} frames; the kernels take {MIN_T} .. {MAX_T} frames "
                         f"({(MIN_T - 1) * HOP} .. {MAX_T * HOP - 1} samples)")
    return T


# ----------------------------------------------------------------------------- filter bank tables
def hamming_window() -> np.ndarray:
    """Periodic Hamming window of 400 samples (torch.hamming_window's default), float64."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def mel_filterbank() -> np.ndarray:
    """[201, 80] float64: 80 triangular filters whose edges are equally spaced on 2595 log10(1 + f / 700) from 0 to 8000 Hz, shapes
    built in Hz: with f the bin frequency, c the centre and b the band (centre minus left edge), max(0, min((f - c) / b + 1,
    -(f - c) / b + 1))."""
    to_mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    hz = 700.0 * (10.0 ** (np.linspace(to_mel(0.0), to_mel(SAMPLE_RATE / 2.0), N_MELS + 2) / 2595.0) - 1.0)
    band = (hz[1:] - hz[:-1])[:-1]
    centre = hz[1:-1]
    f = np.linspace(0.0, SAMPLE_RATE / 2.0, N_BINS)
    slope = (f[:, None] - centre[None, :]) / band[None, :]
    return np.maximum(0.0, np.minimum(slope + 1.0, -slope + 1.0))


def fbank_tables():
    """-> (window f32 [400], twiddle f32 [400, 2] = (cos, -sin)(2 pi j / 400), mel f32 [201, 80], ranges int32 [80, 2] = first / end
    bin of every filter's non-zero taps in the f32 table)."""
    j = np.arange(N_FFT)
    tw = np.stack([np.cos(2.0 * np.pi * j / N_FFT), -np.sin(2.0 * np.pi * j / N_FFT)], 1)
    mel = mel_filterbank().astype(np.float32)
    rng = np.zeros((N_MELS, 2), np.int32)
    for m in range(N_MELS):
        nz = np.nonzero(mel[:, m])[0]
        rng[m] = (nz[0], nz[-1] + 1) if len(nz) else (0, 0)
    return hamming_window().astype(np.float32), tw.astype(np.float32), mel, rng


# ----------------------------------------------------------------------------- packing
def fold_batchnorm(weight, bias, mean, var, eps=1e-5):
    """Eval-mode BatchNorm as y = x * scale + shift, computed in float64: scale = weight / sqrt(var + eps), shift = bias - mean * scale."""
    w, b, m, v = (torch.as_tensor(np.asarray(a)).to(torch.float64) for a in (weight, bias, mean, var))
    scale = w / torch.sqrt(v + eps)
    return scale.to(F32), (b - m * scale).to(F32)


def pack_res2net(ws) -> torch.Tensor:
    """Seven plain conv weights [w, w, 3] -> the image ``ta_ecapa_res2net`` reads: bf16 [7][w][Kp], Kp = 3 w rounded up to 32, row =
    output channel, column = tap * w + cin, columns >= 3 w zero."""
    ws = [torch.as_tensor(np.asarray(x)).to(F32) for x in ws]
    w = ws[0].shape[0]
    kp = (3 * w + 31) // 32 * 32
    img = torch.zeros(len(ws), w, kp, dtype=F32)
    for m, x in enumerate(ws):
        if tuple(x.shape) != (w, w, 3):
            raise ValueError(f"res2net conv {m} is {tuple(x.shape)}, expected {(w, w, 3)}")
        img[m, :, :3 * w] = x.permute(0, 2, 1).reshape(w, 3 * w)
    return img.to(BF16).contiguous()


def _tdnn_names(prefix):
    return [prefix + "conv.conv.weight", prefix + "conv.conv.bias"] + [prefix + "norm.norm." + n for n in _BN]


def state_dict_names(config: EcapaConfig):
    """Every parameter / buffer name of SpeechBrain's ``ECAPA_TDNN`` this module reads, written from its module layout
    (``blocks.0`` a TDNNBlock, ``blocks.1-3`` SERes2NetBlocks, ``mfa``, ``asp``, ``asp_bn``, ``fc``); unchecked against a real file."""
    names = _tdnn_names("blocks.0.")
    for b in (1, 2, 3):
        p = f"blocks.{b}."
        names += _tdnn_names(p + "tdnn1.")
        for m in range(SCALE - 1):
            names += _tdnn_names(p + f"res2net_block.blocks.{m}.")
        names += _tdnn_names(p + "tdnn2.")
        names += [p + f"se_block.conv{i}.conv.{n}" for i in (1, 2) for n in ("weight", "bias")]
    names += _tdnn_names("mfa.") + _tdnn_names("asp.tdnn.") + ["asp.conv.conv.weight", "asp.conv.conv.bias"]
    names += ["asp_bn.norm." + n for n in _BN] + ["fc.conv.weight", "fc.conv.bias"]
    return names


def pack_state_dict(sd, config: EcapaConfig):
    """SpeechBrain ``ECAPA_TDNN.state_dict()`` -> the images ``ta_ecapa_weights`` points to, as CPU tensors (matrices bf16, vectors,
    SE matrices and filter-bank tables fp32).  Pure tensor arithmetic: no device, no library."""
    Cc, se, A, D, w = config.channels, config.se_channels, config.attention_channels, config.lin_neurons, config.width
    g = lambda k: torch.as_tensor(np.asarray(sd[k])).detach().to(F32).cpu()

    def conv(k, shape):
        x = g(k)
        if tuple(x.shape) != shape:
            raise ValueError(f"{k} is {tuple(x.shape)}, the config says {shape}")
        return x

    def bn(prefix):
        return fold_batchnorm(*(g(prefix + n) for n in _BN), eps=config.bn_eps)

    b = {}
    win, tw, mel, rng = fbank_tables()
    b["fb_window"], b["fb_twiddle"], b["fb_mel"] = torch.from_numpy(win), torch.from_numpy(tw).contiguous(), torch.from_numpy(mel).contiguous()
    b["fb_mel_range"] = torch.from_numpy(rng).contiguous()
    w0 = conv("blocks.0.conv.conv.weight", (Cc, N_MELS, 5))
    img = torch.zeros(Cc, 5, FEAT_STRIDE, dtype=F32)
    img[:, :, :N_MELS] = w0.permute(0, 2, 1)
    b["w0"], b["b0"] = img.reshape(Cc, 5 * FEAT_STRIDE).to(BF16).contiguous(), g("blocks.0.conv.conv.bias")
    b["bn0_s"], b["bn0_t"] = bn("blocks.0.norm.norm.")
    for i in (1, 2, 3):
        p, q = f"blocks.{i}.", f"blk{i - 1}."
        b[q + "w1"], b[q + "b1"] = conv(p + "tdnn1.conv.conv.weight", (Cc, Cc, 1))[:, :, 0].to(BF16).contiguous(), g(p + "tdnn1.conv.conv.bias")
        b[q + "bn1_s"], b[q + "bn1_t"] = bn(p + "tdnn1.norm.norm.")
        r = [p + f"res2net_block.blocks.{m}." for m in range(SCALE - 1)]
        b[q + "res_w"] = pack_res2net([conv(x + "conv.conv.weight", (w, w, 3)) for x in r])
        b[q + "res_b"] = torch.cat([g(x + "conv.conv.bias") for x in r]).contiguous()
        folded = [bn(x + "norm.norm.") for x in r]
        b[q + "res_s"], b[q + "res_t"] = torch.cat([f[0] for f in folded]).contiguous(), torch.cat([f[1] for f in folded]).contiguous()
        b[q + "w2"], b[q + "b2"] = conv(p + "tdnn2.conv.conv.weight", (Cc, Cc, 1))[:, :, 0].to(BF16).contiguous(), g(p + "tdnn2.conv.conv.bias")
        b[q + "bn2_s"], b[q + "bn2_t"] = bn(p + "tdnn2.norm.norm.")
        b[q + "se_w1t"] = conv(p + "se_block.conv1.conv.weight", (se, Cc, 1))[:, :, 0].t().contiguous()
        b[q + "se_b1"] = g(p + "se_block.conv1.conv.bias")
        b[q + "se_w2t"] = conv(p + "se_block.conv2.conv.weight", (Cc, se, 1))[:, :, 0].t().contiguous()
        b[q + "se_b2"] = g(p + "se_block.conv2.conv.bias")
    b["mfa_w"], b["mfa_b"] = conv("mfa.conv.conv.weight", (3 * Cc, 3 * Cc, 1))[:, :, 0].to(BF16).contiguous(), g("mfa.conv.conv.bias")
    b["mfa_s"], b["mfa_t"] = bn("mfa.norm.norm.")
    wa = conv("asp.tdnn.conv.conv.weight", (A, 9 * Cc, 1))[:, :, 0]
    b["att_wh"], b["att_wms"] = wa[:, :3 * Cc].to(BF16).contiguous(), wa[:, 3 * Cc:].to(BF16).contiguous()
    b["att_b"] = g("asp.tdnn.conv.conv.bias")
    b["att_s"], b["att_t"] = bn("asp.tdnn.norm.norm.")
    b["att_conv_w"], b["att_conv_b"] = conv("asp.conv.conv.weight", (3 * Cc, A, 1))[:, :, 0].to(BF16).contiguous(), g("asp.conv.conv.bias")
    b["aspbn_s"], b["aspbn_t"] = bn("asp_bn.norm.")
    b["fc_w"], b["fc_b"] = conv("fc.conv.weight", (D, 6 * Cc, 1))[:, :, 0].to(BF16).contiguous(), g("fc.conv.bias")
    return b


def random_state_dict(config: EcapaConfig, seed: int = 0, attention_gain: float = 8.0) -> dict:
    """A seeded SpeechBrain-named state dict at the configured shapes: O(1 / sqrt(fan_in)) convolutions, perturbed BatchNorm
    statistics, and ``asp.conv`` multiplied by ``attention_gain`` (at unit gain the attention is nearly flat)."""
    gen = torch.Generator().manual_seed(seed)
    Cc, se, A, D, w = config.channels, config.se_channels, config.attention_channels, config.lin_neurons, config.width
    rn = lambda *s, std=1.0: torch.randn(*s, generator=gen, dtype=F32) * std
    sd = {}

    def conv(name, o, i, k, gain=1.0):
        sd[name + "weight"], sd[name + "bias"] = rn(o, i, k, std=gain * math.sqrt(2.0 / (i * k))), rn(o, std=0.1)

    def bn(name, n):
        sd[name + "weight"], sd[name + "bias"] = 0.8 + 0.4 * torch.rand(n, generator=gen), rn(n, std=0.1)
        sd[name + "running_mean"], sd[name + "running_var"] = rn(n, std=0.1), 0.5 + torch.rand(n, generator=gen)

    def tdnn(p, o, i, k):
        conv(p + "conv.conv.", o, i, k)
        bn(p + "norm.norm.", o)

    tdnn("blocks.0.", Cc, N_MELS, 5)
    for b in (1, 2, 3):
        p = f"blocks.{b}."
        tdnn(p + "tdnn1.", Cc, Cc, 1)
        for m in range(SCALE - 1):
            tdnn(p + f"res2net_block.blocks.{m}.", w, w, 3)
        tdnn(p + "tdnn2.", Cc, Cc, 1)
        conv(p + "se_block.conv1.conv.", se, Cc, 1)
        conv(p + "se_block.conv2.conv.", Cc, se, 1)
    tdnn("mfa.", 3 * Cc, 3 * Cc, 1)
    tdnn("asp.tdnn.", A, 9 * Cc, 1)
    conv("asp.conv.conv.", 3 * Cc, A, 1, gain=attention_gain)
    bn("asp_bn.norm.", 6 * Cc)
    conv("fc.conv.", D, 6 * Cc, 1)
    return sd


_BLOCK_FIELDS = ("w1", "b1", "bn1_s", "bn1_t", "res_w", "res_b", "res_s", "res_t", "w2", "b2", "bn2_s", "bn2_t", "se_w1t", "se_b1",
                 "se_w2t", "se_b2")
_TOP_FIELDS = ("fb_window", "fb_twiddle", "fb_mel", "fb_mel_range", "w0", "b0", "bn0_s", "bn0_t", "mfa_w", "mfa_b", "mfa_s", "mfa_t",
               "att_wh", "att_wms", "att_b", "att_s", "att_t", "att_conv_w", "att_conv_b", "aspbn_s", "aspbn_t", "fc_w", "fc_b")


def _windows_args(n_audio, starts, lengths, window_samples):
    """Validated (starts, lengths) as int32 arrays: what ``ta_ecapa_forward`` would refuse, refused here with the limit named."""
    check_window_samples(window_samples)
    starts, lengths = np.asarray(starts, np.int64).reshape(-1), np.asarray(lengths, np.int64).reshape(-1)
    if starts.shape != lengths.shape:
        raise ValueError(f"{starts.size} starts for {lengths.size} lengths")
    for s, n in zip(starts.tolist(), lengths.tolist()):
        if n < 1 or n > window_samples:
            raise ValueError(f"a chunk of {n} samples does not fit a window of {window_samples}")
        if window_samples - n > n - 1:
            raise ValueError(f"a chunk of {n} samples cannot be reflect-padded to {window_samples}: the pad of {window_samples - n} "
                             f"needs at least {window_samples - n + 1} samples")
        if s < 0 or s + n > n_audio:
            raise ValueError(f"window [{s}, {s + n}) lies outside the {n_audio} samples of audio")
    if n_audio >= 2 ** 31:
        raise ValueError("the audio buffer must hold fewer than 2^31 samples")
    return starts.astype(np.int32), lengths.astype(np.int32)


class EcapaTdnnMI355X(torch.nn.Module):
    """``model.embed_windows(audio, starts, lengths, window_samples) -> f32 [N, lin_neurons]`` on the device;
    ``model.encode_batch(wavs [N, L]) -> [N, 1, lin_neurons]`` is SpeechBrain's call shape."""

    def __init__(self, config: EcapaConfig | None = None, device="cuda"):
        super().__init__()
        self.config = config if config is not None else EcapaConfig()
        self.device_ = torch.device(device)
        self.chunk_windows = DEFAULT_CHUNK
        self._bufs = {}
        self._w = None
        self._ws = None

    # ------------------------------------------------------------------ weights
    def load_state_dict_speechbrain(self, sd):
        """sd: {SpeechBrain ``ECAPA_TDNN`` parameter / buffer name: array-like} (``state_dict_names``; ``num_batches_tracked``
        entries are ignored).  The names are written from SpeechBrain's module layout and are unchecked against a real file."""
        self._bufs = {k: v.to(self.device_) for k, v in pack_state_dict(sd, self.config).items()}
        self._finalize()
        return self

    def random_init(self, seed=0):
        """Seeded random weights at the configured shapes (``random_state_dict``)."""
        return self.load_state_dict_speechbrain(random_state_dict(self.config, seed))

    def _finalize(self):
        c, b = self.config, self._bufs
        w = _lib.EcapaWeights(channels=c.channels, se_channels=c.se_channels, attn_channels=c.attention_channels, emb_dim=c.lin_neurons)
        for f in _TOP_FIELDS:
            setattr(w, f, b[f].data_ptr())
        for i in range(3):
            for f in _BLOCK_FIELDS:
                setattr(w.blocks[i], f, b[f"blk{i}.{f}"].data_ptr())
            w.blocks[i].dilation = c.dilations[i]
        self._w = w

    def export_state_dict_speechbrain(self):
        """Back to SpeechBrain's names as fp32 numpy (matrices carry their bf16 rounding).  A folded BatchNorm comes out as
        ``running_mean = 0, running_var = 1 - eps, weight = scale, bias = shift``, which folds to itself."""
        c, b = self.config, self._bufs
        Cc, w = c.channels, c.width
        f = lambda t: t.detach().float().cpu().numpy()
        sd = {}

        def bn(prefix, s, t):
            n = s.numel()
            sd[prefix + "weight"], sd[prefix + "bias"] = f(s), f(t)
            sd[prefix + "running_mean"], sd[prefix + "running_var"] = np.zeros(n, np.float32), np.full(n, 1.0 - c.bn_eps, np.float32)

        sd["blocks.0.conv.conv.weight"] = f(b["w0"]).reshape(Cc, 5, FEAT_STRIDE)[:, :, :N_MELS].transpose(0, 2, 1).copy()
        sd["blocks.0.conv.conv.bias"] = f(b["b0"])
        bn("blocks.0.norm.norm.", b["bn0_s"], b["bn0_t"])
        for i in (1, 2, 3):
            p, q = f"blocks.{i}.", f"blk{i - 1}."
            for n in ("1", "2"):
                sd[p + f"tdnn{n}.conv.conv.weight"], sd[p + f"tdnn{n}.conv.conv.bias"] = f(b[q + "w" + n])[:, :, None], f(b[q + "b" + n])
                bn(p + f"tdnn{n}.norm.norm.", b[q + f"bn{n}_s"], b[q + f"bn{n}_t"])
            img = f(b[q + "res_w"])
            for m in range(SCALE - 1):
                r = p + f"res2net_block.blocks.{m}."
                sd[r + "conv.conv.weight"] = img[m, :, :3 * w].reshape(w, 3, w).transpose(0, 2, 1).copy()
                sd[r + "conv.conv.bias"] = f(b[q + "res_b"][m * w:(m + 1) * w])
                bn(r + "norm.norm.", b[q + "res_s"][m * w:(m + 1) * w], b[q + "res_t"][m * w:(m + 1) * w])
            sd[p + "se_block.conv1.conv.weight"], sd[p + "se_block.conv1.conv.bias"] = f(b[q + "se_w1t"]).T[:, :, None].copy(), f(b[q + "se_b1"])
            sd[p + "se_block.conv2.conv.weight"], sd[p + "se_block.conv2.conv.bias"] = f(b[q + "se_w2t"]).T[:, :, None].copy(), f(b[q + "se_b2"])
        sd["mfa.conv.conv.weight"], sd["mfa.conv.conv.bias"] = f(b["mfa_w"])[:, :, None], f(b["mfa_b"])
        bn("mfa.norm.norm.", b["mfa_s"], b["mfa_t"])
        sd["asp.tdnn.conv.conv.weight"] = np.concatenate([f(b["att_wh"]), f(b["att_wms"])], 1)[:, :, None]
        sd["asp.tdnn.conv.conv.bias"] = f(b["att_b"])
        bn("asp.tdnn.norm.norm.", b["att_s"], b["att_t"])
        sd["asp.conv.conv.weight"], sd["asp.conv.conv.bias"] = f(b["att_conv_w"])[:, :, None], f(b["att_conv_b"])
        bn("asp_bn.norm.", b["aspbn_s"], b["aspbn_t"])
        sd["fc.conv.weight"], sd["fc.conv.bias"] = f(b["fc_w"])[:, :, None], f(b["fc_b"])
        return sd

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def embed_windows(self, audio, starts, lengths, window_samples):
        """audio: 1-D float array / tensor at 16 kHz (uploaded once); window i = ``audio[starts[i] : starts[i] + lengths[i]]``,
        reflect-padded on the right to ``window_samples`` while it is read (``np.pad(..., mode="reflect")``, so a chunk needs more
        samples than its pad) -> f32 [N, lin_neurons] on the device.  Out-of-envelope arguments raise ``ValueError``."""
        from . import torch_ops
        a = torch.as_tensor(np.ascontiguousarray(audio)) if isinstance(audio, np.ndarray) else torch.as_tensor(audio)
        if a.dim() != 1:
            raise ValueError(f"audio must be 1-D, got {tuple(a.shape)}")
        st, ln = _windows_args(int(a.shape[0]), starts, lengths, int(window_samples))
        if st.size == 0:
            return torch.empty((0, self.config.lin_neurons), device=self.device_, dtype=F32)
        a = a.to(device=self.device_, dtype=F32).contiguous()
        return torch.ops.ta355.ecapa_embeddings(a, st.tolist(), ln.tolist(), int(window_samples), torch_ops.register_module(self))

    @torch.no_grad()
    def encode_batch(self, wavs, wav_lens=None):
        """wavs [N, L] (or [L]): every row one full window -> embeddings [N, 1, lin_neurons], SpeechBrain's ``encode_batch`` shape
        (the reference squeezes it, tiny_audio/diarization.py:490-502).  ``wav_lens`` is accepted for the call shape and must be
        None or all ones: the windows are not padded."""
        w = torch.as_tensor(np.ascontiguousarray(wavs)) if isinstance(wavs, np.ndarray) else torch.as_tensor(wavs)
        if w.dim() == 1:
            w = w[None]
        if w.dim() != 2:
            raise ValueError(f"wavs must be [N, L], got {tuple(w.shape)}")
        if wav_lens is not None and not bool((torch.as_tensor(wav_lens) == 1).all()):
            raise ValueError("relative lengths other than 1 are not supported: pass windows of equal length")
        N, L = w.shape
        emb = self.embed_windows(w.reshape(-1), np.arange(N, dtype=np.int64) * L, np.full(N, L, np.int64), L)
        return emb[:, None, :]

    def _embed_impl(self, audio, starts, lengths, window_samples, out=None):
        """audio f32 [n] on the device, starts / lengths: Python ints -> embeddings [N, lin_neurons] (into ``out`` when given)."""
        if self._w is None:
            raise _lib.Ta355Error("ECAPA weights not loaded (load_state_dict_speechbrain / random_init)")
        audio = audio.to(device=self.device_, dtype=F32).contiguous()
        st, ln = _windows_args(int(audio.shape[0]), starts, lengths, int(window_samples))
        N, D, T = int(st.size), self.config.lin_neurons, frames_of(window_samples)
        chunk = max(1, min(int(self.chunk_windows), N))
        if chunk * T * 3 * self.config.channels > 2 ** 31 - 1 or chunk > 65535:
            raise ValueError(f"chunk_windows = {chunk} at {T} frames exceeds the 2^31 - 1 elements of one chunk's widest buffer")
        if out is None:
            out = torch.empty((N, D), device=self.device_, dtype=F32)
        elif out.dtype != F32 or not out.is_contiguous() or tuple(out.shape) != (N, D):
            raise ValueError(f"out must be a contiguous f32 [{N}, {D}] tensor")
        if N == 0:
            return out
        st_dev, ln_dev = torch.from_numpy(st).to(self.device_), torch.from_numpy(ln).to(self.device_)
        n = _lib.lib().ta_ecapa_workspace_bytes(C.byref(self._w), chunk, T)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(max(n, 256), device=self.device_, dtype=torch.uint8)
        _lib.check(_lib.lib().ta_ecapa_forward(C.byref(self._w), ptr(audio), int(audio.shape[0]), st.ctypes.data_as(C.c_void_p),
                                              ln.ctypes.data_as(C.c_void_p), ptr(st_dev), ptr(ln_dev), N, int(window_samples), chunk,
                                              ptr(out), ptr(self._ws), self._ws.numel(), stream()), "ta_ecapa_forward")
        return out

"""Device-side waveform augmentation: the numeric stages of the reference's production recipe between the raw audio and the log-mel.

The reference turns on ``rir_augmentation`` and ``noise_augmentation`` (configs/training/production.yaml:67-140) and runs them in CPU
dataloader workers through ``audiomentations`` (tiny_audio/augmentation.py:71-223, wired at scripts/train.py:530-587).  Here the
waveforms are already on the device when they would run, so ``DeviceWaveAugment`` runs the chain there, between the upload and
``ta_logmel_f32``: RIR convolution, background noise at an SNR, the always-on Gaussian floor, percentile clipping -- the reference's
order with its remaining members off.  The random DECISIONS are drawn on the host (``plan``); the device does the arithmetic
(``apply`` -> ``torch.ops.ta355.wave_augment``).  Semantics: DESIGN.md section 3 "Device-side augmentation"; tests/augment_ref.py is
the float64 definition.  ``audiomentations`` is not installed here: the stages are restated from its published behaviour.

Keyword names are those of the reference's ``RIRAugmentation`` / ``NoiseAugmentation`` wherever a stage exists; pools are handed in as
lists of float arrays at ``sample_rate`` (reading and resampling files is the caller's business).  ``DeviceWaveAugment`` refuses
``short_noises_prob``, ``eq_prob`` and ``bandlimit_prob`` by name; ``DeviceProductionAugment`` runs the whole production chain: those
three members in their places (short noises before the Gaussian floor, the EQ before the clipping, the band-limit last), through
``torch.ops.ta355.wave_augment_chain``; tests/augment_chain_ref.py is their float64 definition.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import F32, ptr, stream

CONV_HOP = 2048            # TA_WAVE_CONV_HOP (include/ta355.h): the overlap-save hop; the transform is 2 * CONV_HOP points
CONV_DIRECT = 32           # TA_WAVE_CONV_DIRECT: a clip or a response of at most this many samples is convolved directly, in double


@dataclass
class WaveAugmentPlan:
    """The per-clip descriptor of one batch (host arrays of B entries): what ``plan`` draws and ``apply`` consumes."""
    ir_idx: np.ndarray          # int32, impulse response per clip, -1 = no RIR
    noise_idx: np.ndarray       # int32, background clip, -1 = none
    noise_start: np.ndarray     # int64, offset of the noise window in that clip
    noise_snr_db: np.ndarray    # float32 (NaN where the stage is off)
    gauss_snr_db: np.ndarray    # float32 (NaN where the stage is off)
    clip_pct: np.ndarray        # int32 in 1..clipping_max_percentile, 0 = off
    seed: int                   # Philox key of the Gaussian floor
    offset: int                 # Philox offset: advances with every plan

    def stages(self) -> int:
        """Bit mask of the stages at least one clip uses: 1 RIR, 2 background, 4 Gaussian, 8 clipping."""
        return (1 * bool((self.ir_idx >= 0).any()) | 2 * bool((self.noise_idx >= 0).any())
                | 4 * bool(np.isfinite(self.gauss_snr_db).any()) | 8 * bool((self.clip_pct > 0).any()))

    def pack(self) -> np.ndarray:
        """One uint8 image for one upload: noise_start i64 | ir_idx, noise_idx, clip_pct i32 | noise_amp, gauss_amp f32, with
        amp = 10^(-snr / 20) (0 where the stage is off)."""
        def amp(snr):
            snr = np.asarray(snr, np.float64)
            on = np.isfinite(snr)
            return np.where(on, 10.0 ** (-np.where(on, snr, 0.0) / 20.0), 0.0).astype(np.float32)
        parts = [self.noise_start.astype(np.int64), self.ir_idx.astype(np.int32), self.noise_idx.astype(np.int32),
                 self.clip_pct.astype(np.int32), amp(self.noise_snr_db), amp(self.gauss_snr_db)]
        return np.concatenate([np.ascontiguousarray(p).view(np.uint8) for p in parts])


def _unpack(desc: torch.Tensor, B: int):
    """The device views of ``WaveAugmentPlan.pack``'s image."""
    i64 = desc[: 8 * B].view(torch.int64)
    rest = desc[8 * B:]
    i32 = lambda k: rest[4 * B * k: 4 * B * (k + 1)].view(torch.int32)
    f32 = lambda k: rest[4 * B * k: 4 * B * (k + 1)].view(torch.float32)
    return dict(noise_start=i64, ir_idx=i32(0), noise_idx=i32(1), clip_pct=i32(2), noise_amp=f32(3), gauss_amp=f32(4))


class DeviceWaveAugment:
    def __init__(self, *, rir_pool: Optional[Sequence] = None, rir_prob: float = 0.5, rir_peak: Optional[float] = 0.5,
                 max_ir_seconds: float = 4.0, noise_pool: Optional[Sequence] = None, prob: float = 0.5, min_snr_db: float = 5.0,
                 max_snr_db: float = 30.0, gaussian_min_snr_db: Optional[float] = None, gaussian_max_snr_db: Optional[float] = None,
                 clipping_prob: float = 0.0, clipping_max_percentile: int = 10, short_noises_prob: float = 0.0, eq_prob: float = 0.0,
                 bandlimit_prob: float = 0.0, sample_rate: int = 16000, device="cuda", seed: int = 0):
        self._take_members(short_noises_prob=short_noises_prob, eq_prob=eq_prob, bandlimit_prob=bandlimit_prob)
        if not 1 <= int(clipping_max_percentile) <= 100:
            raise ValueError(f"clipping_max_percentile must be in 1..100; got {clipping_max_percentile}")
        if rir_peak is not None and not rir_peak > 0.0:
            raise ValueError(f"rir_peak must be positive or None; got {rir_peak}")
        self.sample_rate, self.device, self.seed = int(sample_rate), torch.device(device), int(seed)
        self.rir_prob, self.rir_peak, self.max_ir_seconds = float(rir_prob), rir_peak, float(max_ir_seconds)
        self.prob, self.min_snr_db, self.max_snr_db = float(prob), float(min_snr_db), float(max_snr_db)
        self.gaussian_min_snr_db, self.gaussian_max_snr_db = gaussian_min_snr_db, gaussian_max_snr_db
        self.clipping_prob, self.clipping_max_percentile = float(clipping_prob), int(clipping_max_percentile)
        cap = int(round(self.max_ir_seconds * self.sample_rate))
        self.rir_pool = [np.asarray(h, dtype=np.float32).reshape(-1) for h in (rir_pool or [])]
        if any(len(h) == 0 for h in self.rir_pool):
            raise ValueError("an impulse response of the pool is empty")
        if any(len(h) > cap for h in self.rir_pool):
            warnings.warn(f"DeviceWaveAugment: impulse responses longer than max_ir_seconds = {self.max_ir_seconds} s are cut to "
                          f"{cap} taps at upload", stacklevel=2)
            self.rir_pool = [h[:cap] for h in self.rir_pool]
        self.noise_pool = [np.asarray(v, dtype=np.float32).reshape(-1) for v in (noise_pool or [])]
        if any(len(v) == 0 for v in self.noise_pool):
            raise ValueError("a noise clip of the pool is empty")
        self._rng = np.random.default_rng(self.seed)
        self._plans = 0
        self._dev = None                                  # device images of the pools: built at the first apply()

    def _take_members(self, **probs):
        """The three members of the reference's chain this class does not run: refused by name (``DeviceProductionAugment`` takes them)."""
        for name, p in probs.items():
            if p > 0.0:
                raise NotImplementedError(f"{name} > 0: that member of the reference's chain is not built on the device "
                                          "(DESIGN.md section 3, Device-side augmentation)")

    @property
    def gaussian_on(self) -> bool:
        return self.gaussian_min_snr_db is not None and self.gaussian_max_snr_db is not None

    # ---- host: the random decisions
    def plan(self, lens) -> WaveAugmentPlan:
        """Draw one batch's descriptor from the seeded generator.  Every call draws the same number of variates whatever the
        decisions are, so the sequence of plans is a function of the seed and of the batch sizes alone."""
        B = len(np.asarray(lens).reshape(-1))
        rng = self._rng
        u_rir, u_bg, u_clip = rng.random(B), rng.random(B), rng.random(B)
        r = rng.integers(0, max(len(self.rir_pool), 1), B)
        j = rng.integers(0, max(len(self.noise_pool), 1), B)
        u_start = rng.random(B)
        snr = rng.uniform(self.min_snr_db, self.max_snr_db, B)
        g_lo, g_hi = (self.gaussian_min_snr_db, self.gaussian_max_snr_db) if self.gaussian_on else (0.0, 0.0)
        gsnr = rng.uniform(g_lo, g_hi, B)
        pct = rng.integers(1, self.clipping_max_percentile + 1, B)
        on_rir = (u_rir < self.rir_prob) & bool(self.rir_pool)
        on_bg = (u_bg < self.prob) & bool(self.noise_pool)
        on_clip = u_clip < self.clipping_prob
        nlen = np.array([len(self.noise_pool[k]) for k in j], dtype=np.int64) if self.noise_pool else np.ones(B, dtype=np.int64)
        start = np.minimum((u_start * nlen).astype(np.int64), nlen - 1)
        self._plans += 1
        return WaveAugmentPlan(ir_idx=np.where(on_rir, r, -1).astype(np.int32), noise_idx=np.where(on_bg, j, -1).astype(np.int32),
                               noise_start=np.where(on_bg, start, 0).astype(np.int64),
                               noise_snr_db=np.where(on_bg, snr, np.nan).astype(np.float32),
                               gauss_snr_db=(gsnr if self.gaussian_on else np.full(B, np.nan)).astype(np.float32),
                               clip_pct=np.where(on_clip, pct, 0).astype(np.int32), seed=self.seed, offset=self._plans - 1)

    # ---- device
    def _prepare(self):
        if self._dev is not None:
            return self._dev
        L_, dev = _lib.lib(), self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d = dict(n_ir=len(self.rir_pool), n_noise=len(self.noise_pool), max_taps=0)
        if self.rir_pool:
            taps = np.array([len(h) for h in self.rir_pool], dtype=np.int64)
            parts = (taps + CONV_HOP - 1) // CONV_HOP
            d["max_taps"] = int(taps.max())
            d["ir"] = up(np.concatenate(self.rir_pool))
            d["ir_off"] = up(np.concatenate([[0], np.cumsum(taps)]).astype(np.int64))
            d["part_off"] = up(np.concatenate([[0], np.cumsum(parts)]).astype(np.int32))
            d["tw"] = torch.empty(2 * CONV_HOP, device=dev, dtype=F32)
            d["spectra"] = torch.empty(int(parts.sum()) * 2 * (CONV_HOP + 1), device=dev, dtype=F32)
            _lib.check(L_.ta_wave_fft_twiddles(ptr(d["tw"]), stream()), "ta_wave_fft_twiddles")
            _lib.check(L_.ta_wave_ir_spectra(ptr(d["ir"]), ptr(d["ir_off"]), ptr(d["part_off"]), d["n_ir"], int(parts.max()), ptr(d["tw"]),
                                             ptr(d["spectra"]), stream()), "ta_wave_ir_spectra")
        if self.noise_pool:
            d["noise"] = up(np.concatenate(self.noise_pool))
            d["noise_off"] = up(np.concatenate([[0], np.cumsum([len(v) for v in self.noise_pool])]).astype(np.int64))
        self._dev = d
        return d

    def apply(self, wav: torch.Tensor, lens: torch.Tensor, plan: WaveAugmentPlan) -> torch.Tensor:
        """wav f32 [B, Ls] (zero padded, device), lens i64 [B] (device) -> the augmented [B, Ls]; torch.ops.ta355.wave_augment."""
        from . import torch_ops
        B = wav.shape[0]
        for name in ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct"):
            if len(getattr(plan, name)) != B:
                raise ValueError(f"plan.{name} has {len(getattr(plan, name))} entries for a batch of {B}")
        if (plan.ir_idx >= len(self.rir_pool)).any() or (plan.noise_idx >= len(self.noise_pool)).any():
            raise ValueError("the plan names a pool entry this object does not hold")
        if (plan.clip_pct < 0).any() or (plan.clip_pct > 100).any():
            raise ValueError("plan.clip_pct must be in 0..100")
        desc = torch.from_numpy(plan.pack()).to(wav.device, non_blocking=True)
        return torch.ops.ta355.wave_augment(wav, lens, desc, plan.stages(), int(plan.seed), int(plan.offset),
                                            torch_ops.register_module(self))

    def _apply(self, wav: torch.Tensor, lens: torch.Tensor, desc: torch.Tensor, stages: int, seed: int, offset: int) -> torch.Tensor:
        """The launches: the convolution pass always (it is the one copy of a clip with every stage off), the others only when some
        clip of the batch uses them."""
        v = _unpack(desc, wav.shape[0])
        out = self._conv(wav, lens, v, stages)
        self._mix(out, lens, v, bool(stages & 2), bool(stages & 4), seed, offset)
        if stages & 8:
            self._clip(out, lens, v)
        return out

    def _conv(self, wav, lens, v, stages):
        L_, d = _lib.lib(), self._prepare()
        B, Ls = wav.shape
        wav = wav.contiguous()
        out = torch.empty_like(wav)
        conv = bool(stages & 1)
        ws = torch.empty(L_.ta_wave_conv_ws_bytes(B, Ls, d["max_taps"]) if conv else 0, device=wav.device, dtype=torch.uint8)
        _lib.check(L_.ta_wave_conv_f32(ptr(wav), ptr(lens), B, Ls, ptr(v["ir_idx"]) if conv else None, ptr(d.get("ir")), ptr(d.get("ir_off")),
                                       ptr(d.get("part_off")), d["n_ir"], d["max_taps"], ptr(d.get("tw")), ptr(d.get("spectra")),
                                       float(self.rir_peak or 0.0), ptr(out), ptr(ws) if conv else None, ws.numel(), stream()),
                   "ta_wave_conv_f32")
        return out

    def _mix(self, out, lens, v, bg: bool, gauss: bool, seed: int, offset: int):
        if not (bg or gauss):
            return
        L_, d = _lib.lib(), self._prepare()
        B, Ls = out.shape
        scratch = torch.empty(L_.ta_wave_mix_scratch_floats(B, Ls), device=out.device, dtype=F32)
        _lib.check(L_.ta_wave_mix_f32(ptr(out), ptr(lens), B, Ls, ptr(v["noise_idx"]) if bg else None, ptr(v["noise_start"]),
                                      ptr(v["noise_amp"]), ptr(d.get("noise")), ptr(d.get("noise_off")), d["n_noise"],
                                      ptr(v["gauss_amp"]) if gauss else None, seed, offset, ptr(scratch), stream()),
                   "ta_wave_mix_f32")

    def _clip(self, out, lens, v):
        B, Ls = out.shape
        _lib.check(_lib.lib().ta_wave_clip_f32(ptr(out), ptr(lens), B, Ls, ptr(v["clip_pct"]), stream()), "ta_wave_clip_f32")


# ============================================================================ the whole production chain
MAX_EVENTS = 64            # TA_WAVE_MAX_EVENTS: short-noise events per clip
IIR_MAX_SECTIONS = 8       # TA_WAVE_IIR_MAX_SECTIONS
IIR_CHUNK = 256            # TA_WAVE_IIR_CHUNK: samples per thread of the time-parallel cascade
# Everything below is what the reference leaves to audiomentations' defaults, RECALLED from its published behaviour.
# SevenBandParametricEQ: a low shelf, five peaking bands, a high shelf; (min, max) centre frequency in Hz and (min, max) Q.
EQ_BANDS = (("low_shelf", 42.0, 95.0, 0.1, 0.9), ("peaking", 91.0, 204.0, 0.9, 1.1), ("peaking", 196.0, 441.0, 0.9, 1.1),
            ("peaking", 421.0, 948.0, 0.9, 1.1), ("peaking", 909.0, 2045.0, 0.9, 1.1), ("peaking", 1957.0, 4404.0, 0.9, 1.1),
            ("high_shelf", 4216.0, 9486.0, 0.1, 0.9))
EQ_MAX_CENTER_FRACTION = 0.45      # a centre frequency is clamped to this fraction of the sample rate: a shelf at or above Nyquist is unstable
LOWPASS_ORDERS = (2, 3, 4)         # roll-off 12 / 18 / 24 dB per octave
BANDPASS_ORDERS = (1, 2)           # butter(N, band): roll-off 12 / 24 dB per octave (N sections)


def _hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def _mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def check_sos(sos) -> np.ndarray:
    """float64 [S, 5] sections (b0, b1, b2, a1, a2); ``ValueError`` unless every section's poles lie strictly inside the unit circle."""
    sos = np.asarray(sos, np.float64).reshape(-1, 5)
    if len(sos) > IIR_MAX_SECTIONS:
        raise ValueError(f"a cascade of {len(sos)} sections; at most {IIR_MAX_SECTIONS}")
    if not np.isfinite(sos).all():
        raise ValueError("a section has a coefficient that is not finite")
    a1, a2 = sos[:, 3], sos[:, 4]
    if not ((np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2)).all():
        raise ValueError("a section has a pole on or outside the unit circle: |a2| < 1 and |a1| < 1 + a2 must hold")
    return sos


def rbj_section(kind: str, f0: float, q: float, gain_db: float, sample_rate: int) -> np.ndarray:
    """One RBJ-cookbook biquad (``low_shelf``, ``peaking``, ``high_shelf``) as (b0, b1, b2, a1, a2), a0 = 1.  ``ValueError`` for a centre
    frequency at or above Nyquist."""
    if not 0.0 < f0 < 0.5 * sample_rate:
        raise ValueError(f"centre frequency {f0} Hz is not below Nyquist ({0.5 * sample_rate} Hz)")
    if not q > 0.0:
        raise ValueError(f"Q must be positive; got {q}")
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * f0 / sample_rate
    cs, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
    if kind == "peaking":
        b, a = (1 + alpha * A, -2 * cs, 1 - alpha * A), (1 + alpha / A, -2 * cs, 1 - alpha / A)
    elif kind == "low_shelf":
        k = 2 * np.sqrt(A) * alpha
        b = (A * ((A + 1) - (A - 1) * cs + k), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - k))
        a = ((A + 1) + (A - 1) * cs + k, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - k)
    elif kind == "high_shelf":
        k = 2 * np.sqrt(A) * alpha
        b = (A * ((A + 1) + (A - 1) * cs + k), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - k))
        a = ((A + 1) - (A - 1) * cs + k, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - k)
    else:
        raise ValueError(f"unknown section kind {kind!r}")
    return check_sos(np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]]))[0]


def _butter(order, freqs, btype, sample_rate) -> np.ndarray:
    """scipy.signal.butter(..., output="sos") as [S, 5] sections (a0 = 1 dropped); ``ValueError`` at or above Nyquist."""
    import scipy.signal
    f = np.atleast_1d(np.asarray(freqs, np.float64))
    if not ((f > 0.0) & (f < 0.5 * sample_rate)).all():
        raise ValueError(f"band edge(s) {f.tolist()} Hz are not inside (0, Nyquist = {0.5 * sample_rate} Hz)")
    sos = scipy.signal.butter(int(order), f if len(f) > 1 else float(f[0]), btype=btype, fs=sample_rate, output="sos")
    return check_sos(sos[:, [0, 1, 2, 4, 5]] / sos[:, 3:4])


def lowpass_sos(cutoff: float, order: int, sample_rate: int) -> np.ndarray:
    return _butter(order, cutoff, "lowpass", sample_rate)


def bandpass_sos(center: float, bandwidth_fraction: float, order: int, sample_rate: int) -> np.ndarray:
    return _butter(order, [center * (1.0 - 0.5 * bandwidth_fraction), center * (1.0 + 0.5 * bandwidth_fraction)], "bandpass", sample_rate)


@dataclass
class ProductionAugmentPlan(WaveAugmentPlan):
    """``WaveAugmentPlan`` plus the three remaining members.  Event arrays are [B, MAX_EVENTS] (entries past ``ev_count[b]`` unused)."""
    ev_count: np.ndarray        # int32 [B], 0 = no short noises
    ev_pool: np.ndarray         # int32, pool clip of the event
    ev_off: np.ndarray          # int64, source offset in that clip
    ev_len: np.ndarray          # int64, >= 1, ev_off + ev_len <= the clip's length
    ev_t0: np.ndarray           # int64, destination start, >= 0
    ev_fade_in: np.ndarray      # int32 samples
    ev_fade_out: np.ndarray     # int32 samples
    ev_snr_db: np.ndarray       # float32
    eq_nsec: np.ndarray         # int32 [B], 0 = no EQ
    eq_sos: np.ndarray          # float64 [B, IIR_MAX_SECTIONS, 5]: (b0, b1, b2, a1, a2)
    bl_nsec: np.ndarray         # int32 [B], 0 = no band-limit
    bl_sos: np.ndarray          # float64 [B, IIR_MAX_SECTIONS, 5]

    def stages(self) -> int:
        """The base mask, plus 16 short noises, 32 EQ, 64 band-limit."""
        return (super().stages() | 16 * bool((self.ev_count > 0).any()) | 32 * bool((self.eq_nsec > 0).any())
                | 64 * bool((self.bl_nsec > 0).any()))

    def base(self) -> WaveAugmentPlan:
        """The first four stages' fields alone."""
        return WaveAugmentPlan(self.ir_idx, self.noise_idx, self.noise_start, self.noise_snr_db, self.gauss_snr_db, self.clip_pct,
                               self.seed, self.offset)

    def ev_stride(self) -> int:
        return int(self.ev_count.max()) if len(self.ev_count) else 0

    def max_event_len(self) -> int:
        on = np.arange(self.ev_len.shape[1])[None, :] < self.ev_count[:, None]
        return int(self.ev_len[on].max()) if on.any() else 0

    def pack(self) -> np.ndarray:
        """``WaveAugmentPlan.pack``'s image, zero padding to a multiple of 8 bytes, then: eq_sos, bl_sos f64 [B, 8, 5] | ev_off, ev_len,
        ev_t0 i64 [B, E] | ev_pool, ev_fade_in, ev_fade_out i32 [B, E] | ev_amp f32 [B, E] | ev_count, eq_nsec, bl_nsec i32 [B], with
        E = ``ev_stride()`` and ev_amp = 10^(-snr / 20)."""
        head = self.base().pack()
        E = self.ev_stride()
        amp = (10.0 ** (-self.ev_snr_db[:, :E].astype(np.float64) / 20.0)).astype(np.float32)
        parts = [np.zeros((-len(head)) % 8, np.uint8), self.eq_sos.astype(np.float64), self.bl_sos.astype(np.float64),
                 self.ev_off[:, :E].astype(np.int64), self.ev_len[:, :E].astype(np.int64), self.ev_t0[:, :E].astype(np.int64),
                 self.ev_pool[:, :E].astype(np.int32), self.ev_fade_in[:, :E].astype(np.int32), self.ev_fade_out[:, :E].astype(np.int32),
                 amp, self.ev_count.astype(np.int32), self.eq_nsec.astype(np.int32), self.bl_nsec.astype(np.int32)]
        return np.concatenate([head] + [np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts])


def _unpack_chain(desc: torch.Tensor, B: int, E: int):
    """The device views of ``ProductionAugmentPlan.pack``'s image."""
    v = _unpack(desc[: 28 * B], B)
    at = [(28 * B + 7) // 8 * 8]

    def take(n, dtype, size):
        t = desc[at[0]: at[0] + n * size].view(dtype)
        at[0] += n * size
        return t
    S5 = IIR_MAX_SECTIONS * 5
    v["eq_sos"], v["bl_sos"] = take(B * S5, torch.float64, 8), take(B * S5, torch.float64, 8)
    for k in ("ev_off", "ev_len", "ev_t0"):
        v[k] = take(B * E, torch.int64, 8)
    for k in ("ev_pool", "ev_fade_in", "ev_fade_out"):
        v[k] = take(B * E, torch.int32, 4)
    v["ev_amp"] = take(B * E, torch.float32, 4)
    for k in ("ev_count", "eq_nsec", "bl_nsec"):
        v[k] = take(B, torch.int32, 4)
    if at[0] != desc.numel():
        raise ValueError(f"the descriptor has {desc.numel()} bytes; a batch of {B} with an event stride of {E} packs to {at[0]}")
    return v


class DeviceProductionAugment(DeviceWaveAugment):
    """The reference's whole waveform chain on the device, in its ``Compose`` order (tiny_audio/augmentation.py:153-216): RIR, background
    noise, SHORT NOISES, Gaussian floor, EQ, clipping, BAND-LIMIT.  Same ``plan(lens)`` / ``apply(wav, lens, plan)`` surface as
    ``DeviceWaveAugment``; the operator is ``torch.ops.ta355.wave_augment_chain``.

    Keyword names are the reference's where it has one.  What it leaves to audiomentations' defaults is an argument here, with the default
    recalled from audiomentations' published behaviour (``AddShortNoises``, ``SevenBandParametricEQ``, ``LowPassFilter``,
    ``BandPassFilter``) or a module constant (``EQ_BANDS``, ``LOWPASS_ORDERS``, ``BANDPASS_ORDERS``):

    * short noises: ``short_noises_pool`` (float arrays at ``sample_rate``; without one the stage is a silent no-op, as in the
      reference), SNR range, the pause between events, the burst probability and pause factor inside a burst, fade times, and
      ``fade_floor_db`` (the level a fade starts from).  The event's duration range is this library's own: an event is a window of a
      pool clip, never tiled.
    * EQ: seven RBJ sections, gains uniform in [eq_min_db, eq_max_db], centres uniform on the mel scale inside ``EQ_BANDS`` (clamped to
      ``EQ_MAX_CENTER_FRACTION`` of the sample rate), Q uniform.
    * band-limit: one of a Butterworth low-pass (cutoff uniform on the mel scale, order from ``LOWPASS_ORDERS``) or band-pass (centre
      uniform on the mel scale, bandwidth fraction uniform, order from ``BANDPASS_ORDERS``), each with probability one half.
    """

    def __init__(self, *, short_noises_pool: Optional[Sequence] = None, short_noises_prob: float = 0.0,
                 short_noises_min_snr_db: float = -6.0, short_noises_max_snr_db: float = 18.0,
                 short_noises_min_time_between: float = 2.0, short_noises_max_time_between: float = 8.0,
                 short_noises_min_duration: float = 0.25, short_noises_max_duration: float = 4.0,
                 short_noises_burst_prob: float = 0.22, short_noises_min_pause_factor: float = 0.1,
                 short_noises_max_pause_factor: float = 1.1, short_noises_min_fade_in: float = 0.005,
                 short_noises_max_fade_in: float = 0.08, short_noises_min_fade_out: float = 0.01, short_noises_max_fade_out: float = 0.1,
                 fade_floor_db: float = 70.0, eq_prob: float = 0.0, eq_min_db: float = -4.0, eq_max_db: float = 4.0,
                 bandlimit_prob: float = 0.0, lowpass_min_cutoff: float = 3000.0, lowpass_max_cutoff: float = 7500.0,
                 bandpass_min_center_freq: float = 2000.0, bandpass_max_center_freq: float = 2200.0,
                 bandpass_min_bandwidth_fraction: float = 1.7, bandpass_max_bandwidth_fraction: float = 1.9, **base):
        self.short_noises_pool = [np.asarray(v, dtype=np.float32).reshape(-1) for v in (short_noises_pool or [])]
        if any(len(v) == 0 for v in self.short_noises_pool):
            raise ValueError("a short-noise clip of the pool is empty")
        if not fade_floor_db >= 0.0:
            raise ValueError(f"fade_floor_db must not be negative; got {fade_floor_db}")
        pair = lambda lo, hi: (float(lo), float(hi))
        self.sn_snr = pair(short_noises_min_snr_db, short_noises_max_snr_db)
        self.sn_gap = pair(short_noises_min_time_between, short_noises_max_time_between)
        self.sn_dur = pair(short_noises_min_duration, short_noises_max_duration)
        self.sn_pause = pair(short_noises_min_pause_factor, short_noises_max_pause_factor)
        self.sn_fade_in = pair(short_noises_min_fade_in, short_noises_max_fade_in)
        self.sn_fade_out = pair(short_noises_min_fade_out, short_noises_max_fade_out)
        self.sn_burst_prob, self.fade_floor_db = float(short_noises_burst_prob), float(fade_floor_db)
        self.eq_db = pair(eq_min_db, eq_max_db)
        self.lowpass_cutoff = pair(lowpass_min_cutoff, lowpass_max_cutoff)
        self.bandpass_center = pair(bandpass_min_center_freq, bandpass_max_center_freq)
        self.bandpass_bw = pair(bandpass_min_bandwidth_fraction, bandpass_max_bandwidth_fraction)
        super().__init__(short_noises_prob=short_noises_prob, eq_prob=eq_prob, bandlimit_prob=bandlimit_prob, **base)
        ny = 0.5 * self.sample_rate
        if self.bandlimit_prob > 0.0:          # the widest band the ranges can draw must lie below Nyquist: refused here, not in a worker
            if not 0.0 < self.lowpass_cutoff[0] <= self.lowpass_cutoff[1] < ny:
                raise ValueError(f"low-pass cutoffs {self.lowpass_cutoff} Hz are not inside (0, Nyquist = {ny} Hz)")
            lo = self.bandpass_center[0] * (1.0 - 0.5 * self.bandpass_bw[1])
            hi = self.bandpass_center[1] * (1.0 + 0.5 * self.bandpass_bw[1])
            if not (0.0 < lo and hi < ny):
                raise ValueError(f"band-pass edges can reach {lo} .. {hi} Hz: not inside (0, Nyquist = {ny} Hz)")

    def _take_members(self, **probs):
        self.short_noises_prob, self.eq_prob, self.bandlimit_prob = (float(probs[k]) for k in ("short_noises_prob", "eq_prob", "bandlimit_prob"))

    # ---- host: the random decisions
    def plan(self, lens) -> ProductionAugmentPlan:
        """The base plan's draws first (so the first four stages of a seed are ``DeviceWaveAugment``'s), then a fixed number of variates
        for the three members, whatever is decided."""
        lens = np.asarray(lens).reshape(-1).astype(np.int64)
        B, E, sr = len(lens), MAX_EVENTS, self.sample_rate
        p = super().plan(lens)
        rng = self._rng
        u_sn, u_eq, u_bl, u_which, u_first = rng.random(B), rng.random(B), rng.random(B), rng.random(B), rng.random(B)
        pool = rng.integers(0, max(len(self.short_noises_pool), 1), (B, E))
        u_off, u_burst = rng.random((B, E)), rng.random((B, E))
        dur, gap, pause = rng.uniform(*self.sn_dur, (B, E)), rng.uniform(*self.sn_gap, (B, E)), rng.uniform(*self.sn_pause, (B, E))
        snr, f_in, f_out = rng.uniform(*self.sn_snr, (B, E)), rng.uniform(*self.sn_fade_in, (B, E)), rng.uniform(*self.sn_fade_out, (B, E))
        eq_gain, u_fc, u_q = rng.uniform(*self.eq_db, (B, 7)), rng.random((B, 7)), rng.random((B, 7))
        u_cut, u_center, bw = rng.random(B), rng.random(B), rng.uniform(*self.bandpass_bw, B)
        lp_order, bp_order = rng.integers(0, len(LOWPASS_ORDERS), B), rng.integers(0, len(BANDPASS_ORDERS), B)

        z = lambda dt: np.zeros((B, E), dt)
        ev = dict(ev_count=np.zeros(B, np.int32), ev_pool=z(np.int32), ev_off=z(np.int64), ev_len=np.ones((B, E), np.int64), ev_t0=z(np.int64),
                  ev_fade_in=z(np.int32), ev_fade_out=z(np.int32), ev_snr_db=z(np.float32))
        on_sn = (u_sn < self.short_noises_prob) & bool(self.short_noises_pool)
        for b in np.flatnonzero(on_sn):
            t, k = int(u_first[b] * min(gap[b, 0] * sr, float(lens[b]))), 0      # the first event starts inside the clip
            while k < E and t < lens[b]:
                src = self.short_noises_pool[pool[b, k]]
                length = int(min(max(round(dur[b, k] * sr), 1), len(src)))
                ev["ev_pool"][b, k], ev["ev_len"][b, k], ev["ev_t0"][b, k] = pool[b, k], length, t
                ev["ev_off"][b, k] = min(int(u_off[b, k] * (len(src) - length + 1)), len(src) - length)
                ev["ev_fade_in"][b, k], ev["ev_fade_out"][b, k] = min(round(f_in[b, k] * sr), length), min(round(f_out[b, k] * sr), length)
                ev["ev_snr_db"][b, k] = snr[b, k]
                t += max(int(pause[b, k] * length), 1) if u_burst[b, k] < self.sn_burst_prob else length + int(gap[b, k] * sr)
                k += 1
            ev["ev_count"][b] = k

        mel = lambda u, lo, hi: _mel_to_hz(_hz_to_mel(lo) + u * (_hz_to_mel(hi) - _hz_to_mel(lo)))
        eq_sos, bl_sos = np.zeros((B, IIR_MAX_SECTIONS, 5)), np.zeros((B, IIR_MAX_SECTIONS, 5))
        eq_nsec, bl_nsec = np.zeros(B, np.int32), np.zeros(B, np.int32)
        top = EQ_MAX_CENTER_FRACTION * sr
        for b in np.flatnonzero(u_eq < self.eq_prob):
            for k, (kind, f_lo, f_hi, q_lo, q_hi) in enumerate(EQ_BANDS):
                fc = float(mel(u_fc[b, k], min(f_lo, top), min(f_hi, top)))
                eq_sos[b, k] = rbj_section(kind, fc, q_lo + u_q[b, k] * (q_hi - q_lo), float(eq_gain[b, k]), sr)
            eq_nsec[b] = len(EQ_BANDS)
        for b in np.flatnonzero(u_bl < self.bandlimit_prob):
            if u_which[b] < 0.5:
                sos = lowpass_sos(float(mel(u_cut[b], *self.lowpass_cutoff)), LOWPASS_ORDERS[lp_order[b]], sr)
            else:
                sos = bandpass_sos(float(mel(u_center[b], *self.bandpass_center)), float(bw[b]), BANDPASS_ORDERS[bp_order[b]], sr)
            bl_sos[b, : len(sos)], bl_nsec[b] = sos, len(sos)
        return ProductionAugmentPlan(**{k: getattr(p, k) for k in ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db",
                                                                  "clip_pct", "seed", "offset")},
                                     **ev, eq_nsec=eq_nsec, eq_sos=eq_sos, bl_nsec=bl_nsec, bl_sos=bl_sos)

    # ---- device
    def _prepare(self):
        d = super()._prepare()
        if "n_events" not in d:
            d["n_events"] = len(self.short_noises_pool)
            if self.short_noises_pool:
                d["events"] = torch.from_numpy(np.concatenate(self.short_noises_pool)).to(self.device)
                off = np.concatenate([[0], np.cumsum([len(v) for v in self.short_noises_pool])]).astype(np.int64)
                d["events_off"] = torch.from_numpy(off).to(self.device)
        return d

    def apply(self, wav: torch.Tensor, lens: torch.Tensor, plan: ProductionAugmentPlan) -> torch.Tensor:
        """wav f32 [B, Ls] (zero padded, device), lens i64 [B] (device) -> the augmented [B, Ls]; torch.ops.ta355.wave_augment_chain."""
        from . import torch_ops
        B = wav.shape[0]
        for name in ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct", "ev_count", "ev_pool", "ev_off", "ev_len",
                     "ev_t0", "ev_fade_in", "ev_fade_out", "ev_snr_db", "eq_nsec", "eq_sos", "bl_nsec", "bl_sos"):
            if len(getattr(plan, name)) != B:
                raise ValueError(f"plan.{name} has {len(getattr(plan, name))} entries for a batch of {B}")
        if (plan.ir_idx >= len(self.rir_pool)).any() or (plan.noise_idx >= len(self.noise_pool)).any():
            raise ValueError("the plan names a pool entry this object does not hold")
        if (plan.clip_pct < 0).any() or (plan.clip_pct > 100).any():
            raise ValueError("plan.clip_pct must be in 0..100")
        E = plan.ev_stride()
        if (plan.ev_count < 0).any() or E > min(MAX_EVENTS, plan.ev_pool.shape[1]):
            raise ValueError(f"plan.ev_count must be in 0..{min(MAX_EVENTS, plan.ev_pool.shape[1])}")
        on = np.arange(plan.ev_pool.shape[1])[None, :] < plan.ev_count[:, None]
        if on.any():
            j, o, ln = plan.ev_pool[on], plan.ev_off[on], plan.ev_len[on]
            if (j < 0).any() or (j >= len(self.short_noises_pool)).any():
                raise ValueError("the plan names a pool entry this object does not hold")
            plen = np.array([len(v) for v in self.short_noises_pool], np.int64)[j]
            if (o < 0).any() or (ln < 1).any() or (o + ln > plen).any() or (plan.ev_t0[on] < 0).any():
                raise ValueError("an event must lie inside its pool clip (no tiling), have at least one sample and start at t0 >= 0")
            if (plan.ev_fade_in[on] < 0).any() or (plan.ev_fade_out[on] < 0).any() or not np.isfinite(plan.ev_snr_db[on]).all():
                raise ValueError("an event's fades must not be negative and its SNR must be finite")
        for nsec, sos in ((plan.eq_nsec, plan.eq_sos), (plan.bl_nsec, plan.bl_sos)):
            if (nsec < 0).any() or (nsec > IIR_MAX_SECTIONS).any() or sos.shape[1:] != (IIR_MAX_SECTIONS, 5):
                raise ValueError(f"a cascade has 0..{IIR_MAX_SECTIONS} sections of 5 coefficients")
            for b in np.flatnonzero(nsec > 0):
                check_sos(sos[b, : nsec[b]])
        desc = torch.from_numpy(plan.pack()).to(wav.device, non_blocking=True)
        return torch.ops.ta355.wave_augment_chain(wav, lens, desc, plan.stages(), int(plan.seed), int(plan.offset), E,
                                                  plan.max_event_len(), torch_ops.register_module(self))

    def _apply_chain(self, wav: torch.Tensor, lens: torch.Tensor, desc: torch.Tensor, stages: int, seed: int, offset: int, ev_stride: int,
                     max_event_len: int) -> torch.Tensor:
        """The launches, in the reference's order.  With no clip using a new member they are exactly ``DeviceWaveAugment._apply``'s; when
        some clip has events the mix runs twice (background only, then Gaussian only), so that the floor's rms is taken from its own input."""
        L_, d = _lib.lib(), self._prepare()
        B, Ls = wav.shape
        v = _unpack_chain(desc, B, ev_stride)
        out = self._conv(wav, lens, v, stages)
        bg, gauss = bool(stages & 2), bool(stages & 4)
        if stages & 16:
            self._mix(out, lens, v, bg, False, seed, offset)
            scratch = torch.empty(L_.ta_wave_events_scratch_floats(B, Ls, ev_stride, max_event_len), device=wav.device, dtype=F32)
            _lib.check(L_.ta_wave_events_f32(ptr(out), ptr(lens), B, Ls, ptr(v["ev_count"]), ev_stride, ptr(v["ev_pool"]), ptr(v["ev_off"]),
                                             ptr(v["ev_len"]), ptr(v["ev_t0"]), ptr(v["ev_fade_in"]), ptr(v["ev_fade_out"]), ptr(v["ev_amp"]),
                                             ptr(d.get("events")), ptr(d.get("events_off")), d["n_events"], max_event_len,
                                             self.fade_floor_db, ptr(scratch), stream()), "ta_wave_events_f32")
            self._mix(out, lens, v, False, gauss, seed, offset)
        else:
            self._mix(out, lens, v, bg, gauss, seed, offset)
        if stages & 32:
            self._sos(out, lens, v["eq_nsec"], v["eq_sos"])
        if stages & 8:
            self._clip(out, lens, v)
        if stages & 64:
            self._sos(out, lens, v["bl_nsec"], v["bl_sos"])
        return out

    def _sos(self, out, lens, nsec, sos, chunk: int = 0):
        L_ = _lib.lib()
        B, Ls = out.shape
        ws = torch.empty(L_.ta_wave_sos_ws_bytes(B, Ls, chunk), device=out.device, dtype=torch.uint8)
        _lib.check(L_.ta_wave_sos_f32(ptr(out), ptr(lens), B, Ls, ptr(nsec), ptr(sos), chunk, ptr(ws), ws.numel(), stream()), "ta_wave_sos_f32")

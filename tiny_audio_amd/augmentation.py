"""Device-side waveform augmentation: the numeric stages of the reference's production recipe between the raw audio and the log-mel.

The reference turns on ``rir_augmentation`` and ``noise_augmentation`` (configs/training/production.yaml:67-140) and runs them in CPU
dataloader workers through ``audiomentations`` (tiny_audio/augmentation.py:71-223, wired at scripts/train.py:530-587).  Here the
waveforms are already on the device when they would run, so ``DeviceWaveAugment`` runs the chain there, between the upload and
``ta_logmel_f32``: RIR convolution, background noise at an SNR, the always-on Gaussian floor, percentile clipping -- the reference's
order with its remaining members off.  The random DECISIONS are drawn on the host (``plan``); the device does the arithmetic
(``apply`` -> ``torch.ops.ta355.wave_augment``).  Semantics: DESIGN.md section 3 "Device-side augmentation"; tests/augment_ref.py is
the float64 definition.  ``audiomentations`` is not installed here: the stages are restated from its published behaviour.

Keyword names are those of the reference's ``RIRAugmentation`` / ``NoiseAugmentation`` wherever a stage exists; pools are handed in as
lists of float arrays at ``sample_rate`` (reading and resampling files is the caller's business).  Not built, and refused by name when
asked for: ``short_noises_prob``, ``eq_prob``, ``bandlimit_prob``.
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
        for name, p in (("short_noises_prob", short_noises_prob), ("eq_prob", eq_prob), ("bandlimit_prob", bandlimit_prob)):
            if p > 0.0:
                raise NotImplementedError(f"{name} > 0: that member of the reference's chain is not built on the device "
                                          "(DESIGN.md section 3, Device-side augmentation)")
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
        L_, d = _lib.lib(), self._prepare()
        B, Ls = wav.shape
        wav = wav.contiguous()
        v = _unpack(desc, B)
        out = torch.empty_like(wav)
        conv = bool(stages & 1)
        ws = torch.empty(L_.ta_wave_conv_ws_bytes(B, Ls, d["max_taps"]) if conv else 0, device=wav.device, dtype=torch.uint8)
        _lib.check(L_.ta_wave_conv_f32(ptr(wav), ptr(lens), B, Ls, ptr(v["ir_idx"]) if conv else None, ptr(d.get("ir")), ptr(d.get("ir_off")),
                                       ptr(d.get("part_off")), d["n_ir"], d["max_taps"], ptr(d.get("tw")), ptr(d.get("spectra")),
                                       float(self.rir_peak or 0.0), ptr(out), ptr(ws) if conv else None, ws.numel(), stream()),
                   "ta_wave_conv_f32")
        bg, gauss = bool(stages & 2), bool(stages & 4)
        if bg or gauss:
            scratch = torch.empty(L_.ta_wave_mix_scratch_floats(B, Ls), device=wav.device, dtype=F32)
            _lib.check(L_.ta_wave_mix_f32(ptr(out), ptr(lens), B, Ls, ptr(v["noise_idx"]) if bg else None, ptr(v["noise_start"]),
                                          ptr(v["noise_amp"]), ptr(d.get("noise")), ptr(d.get("noise_off")), d["n_noise"],
                                          ptr(v["gauss_amp"]) if gauss else None, seed, offset, ptr(scratch), stream()),
                       "ta_wave_mix_f32")
        if stages & 8:
            _lib.check(L_.ta_wave_clip_f32(ptr(out), ptr(lens), B, Ls, ptr(v["clip_pct"]), stream()), "ta_wave_clip_f32")
        return out

"""Voice activity detection on the device: per-frame speech decisions on the diarizer's grid (one frame per 256 samples of 16 kHz
audio), model-free.

The reference takes its decisions from TEN-VAD, a compiled third-party model that sees one frame per call
(tiny_audio/diarization.py:370-387).  Nothing learned can be pinned here, so ``DeviceVAD`` is a statistical detector of its own:
band energies of a centred 400-sample Hann frame (16 bands of 240 Hz, 80 Hz .. 3.92 kHz), smoothed over ``2 h + 1`` frames, against
a minimum-statistics noise floor taken over ``noise_window_s`` on EITHER side (non-causal: a whole recording is at hand, and every
frame is independent work), the Gaussian likelihood-ratio statistic averaged over the bands, and a threshold (csrc/vad.hip; DESIGN.md
section 3, "Voice activity detection"; the contract is tests/vad_ref.py).  The defaults are design choices checked on synthetic
signals only: they are NOT validated on real speech.

    >>> vad = DeviceVAD()
    >>> flags = vad.speech_frames(audio)                      # bool [frames]
    >>> SpeakerDiarizer.diarize(audio, vad=vad, speaker_model=ecapa)
    >>> model.transcribe_long(audio, vad=vad)                 # windows without speech are not decoded
"""
from __future__ import annotations

import numpy as np
import torch

from . import torch_ops  # noqa: F401  (registers torch.ops.ta355.vad)
from .ops import VAD_HOP, check_vad_options, vad_frames

SAMPLE_RATE = 16000


def speech_runs(flags) -> np.ndarray:
    """Per-frame decisions -> the runs of speech as frame ranges int64 [k, 2] (first frame, one past the last), without a Python loop
    over the frames."""
    f = np.asarray(flags).astype(bool).reshape(-1)
    edge = np.diff(np.concatenate(([0], f.astype(np.int8), [0])))
    return np.stack([np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)], axis=1).astype(np.int64)


def segments_from_flags(flags, sample_rate: int = SAMPLE_RATE) -> list[dict]:
    """Per-frame decisions -> the speech segments ``LocalSpeakerDiarizer._get_speech_segments(..., speech_frames=flags)`` builds: the
    same ``_span`` per run and the same hysteresis (gaps bridged, short segments dropped, the rest padded); the only loop is over runs."""
    from .diarization import LocalSpeakerDiarizer, _span
    frame_duration = VAD_HOP / sample_rate
    return LocalSpeakerDiarizer._apply_vad_hysteresis([_span(int(a), int(b), frame_duration, sample_rate) for a, b in speech_runs(flags)],
                                                      sample_rate)


class DeviceVAD:
    """threshold: theta, on the band-averaged likelihood-ratio statistic L.  noise_window_s: the noise floor is the minimum of the
    smoothed band energy over this many seconds on each side (rounded to frames of 16 ms).  smooth_frames: h, the energies are averaged
    over 2 h + 1 frames.  noise_bias: beta >= 1, the factor on the minimum (a minimum underestimates the mean noise level).  floor: e0,
    about the band energy of 16-bit quantisation noise; it keeps digital silence at L = 0."""

    def __init__(self, threshold: float = 0.15, noise_window_s: float = 1.5, smooth_frames: int = 2, noise_bias: float = 2.0,
                 floor: float = 1e-12):
        noise_window_s = float(noise_window_s)
        if not (noise_window_s == noise_window_s and 0.0 < noise_window_s < float("inf")):
            raise ValueError(f"vad: noise_window_s must be finite and > 0; got {noise_window_s}")
        self.noise_window_s = noise_window_s
        self.smooth, self.noise_window, self.noise_bias, self.threshold, self.floor = check_vad_options(
            smooth_frames, int(round(noise_window_s * SAMPLE_RATE / VAD_HOP)), noise_bias, threshold, floor)

    def options(self) -> tuple:
        return self.smooth, self.noise_window, self.noise_bias, self.threshold, self.floor

    def run_uploaded(self, flat, offsets, lens):
        """On a batch ``longform.upload`` made -> (stat f32 [R, F_max], flags uint8 [R, F_max], n_frames int32 [R]), all on the device;
        recording r owns the first ``ops.vad_frames(lens[r])`` positions of its row."""
        return torch.ops.ta355.vad(flat, offsets, int(max(lens)), *self.options())

    def speech_frames_uploaded(self, flat, offsets, lens):
        """On a batch ``longform.upload`` made -> (the decisions per recording as host bool arrays, flags uint8 [R, F_max] and n_frames
        int32 [R] on the device): one run, one read-back, and the device's copy kept for whoever reads it next (``spk_vote``)."""
        stat, flags, n_frames = self.run_uploaded(flat, offsets, lens)
        stat_h, flags_h = stat.cpu().numpy(), flags.cpu().numpy()
        out = []
        for r, n in enumerate(lens):
            F = vad_frames(n)
            if not np.isfinite(stat_h[r, :F]).all():
                raise ValueError(f"recording {r} holds non-finite samples")
            out.append(flags_h[r, :F].astype(bool))
        return out, flags, n_frames

    def _run(self, waves):
        """-> (single, [(L f32 [F_r], flags bool [F_r]) per recording]): one upload, two launches, one read-back."""
        from .longform import upload
        single = not isinstance(waves, (list, tuple))
        flat, offsets, lens = upload([waves] if single else list(waves))
        stat, flags, _ = self.run_uploaded(flat, offsets, lens)
        stat_h, flags_h = stat.cpu().numpy(), flags.cpu().numpy()
        out = []
        for r, n in enumerate(lens):
            F = vad_frames(n)
            L = stat_h[r, :F].copy()
            if not np.isfinite(L).all():
                raise ValueError(f"recording {r} holds non-finite samples")
            out.append((L, flags_h[r, :F].astype(bool)))
        return single, out

    def statistic(self, waves):
        """The statistic L of every frame: one 1-D recording (numpy array or tensor, host or device) -> f32 [frames]; a list -> a list."""
        single, out = self._run(waves)
        return out[0][0] if single else [o[0] for o in out]

    def speech_frames(self, waves):
        """The decisions L > threshold: one recording -> bool [frames], a list -> a list.  ``frames`` is the diarizer's count,
        ``len(range(0, n - 256, 256))``."""
        single, out = self._run(waves)
        return out[0][1] if single else [o[1] for o in out]

    def speech_segments(self, wave):
        """One recording -> (speech segments after the diarizer's hysteresis, the per-frame decisions bool [frames]): what
        ``LocalSpeakerDiarizer._get_speech_segments`` returns."""
        frames = self.speech_frames(wave)
        if isinstance(frames, list):
            raise ValueError("speech_segments takes one recording, not a list")
        return segments_from_flags(frames), frames


def window_speech_seconds(vad, flat, offsets, lens, windows) -> list[float]:
    """``vad.run_uploaded`` on an uploaded batch (no second upload; the flags are the one read-back) -> for every window
    ``(recording, start_sample, n_samples)`` the seconds of the recording's speech segments (after the diarizer's hysteresis) inside it."""
    _stat, flags, _nf = vad.run_uploaded(flat, offsets, lens)
    return speech_seconds_from_flags(flags.cpu().numpy() if isinstance(flags, torch.Tensor) else np.asarray(flags), lens, windows)


def speech_seconds_from_flags(flags_h, lens, windows) -> list[float]:
    """``window_speech_seconds`` behind the read-back: flags_h [R, F_max] on the host."""
    spans = []
    for r, n in enumerate(lens):
        segs = segments_from_flags(flags_h[r, :vad_frames(n)])
        spans.append((np.array([s["start"] for s in segs], np.float64), np.array([s["end"] for s in segs], np.float64)))
    out = []
    for r, start, n in windows:
        b, e = spans[r]
        w0, w1 = start / SAMPLE_RATE, (start + n) / SAMPLE_RATE
        out.append(float(np.clip(np.minimum(e, w1) - np.maximum(b, w0), 0.0, None).sum()))
    return out

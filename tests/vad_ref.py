"""The voice activity detector of csrc/vad.hip, restated in numpy: THE DEFINITION (include/ta355.h, "voice activity detection";
DESIGN.md section 3, "Voice activity detection"), and the synthetic signals its tests use.  ``statistic(x)`` is the float64 reference;
``statistic(x, dtype=np.float32)`` is the same formulas with every array and constant in float32 (the "float32 restatement": what f32
arithmetic costs in another order than the device's), whose distance from the reference sets the GPU test's gate.

A recording of n samples at 16 kHz, x[k] = 0 outside [0, n); h = smooth, W = noise_window, beta = noise_bias, theta = threshold,
e0 = floor:
  grid      frame i for every i >= 0 with 256 i < n - 256: F = len(range(0, n - 256, 256)), the diarizer's loop count
  spectrum  y[m] = w[m] x[256 i - 72 + m], w the periodic Hann window of 400;  P[i][f] = |DFT400(y)[f]|^2 / 400^2, f = 2 .. 97
  bands     E[i][b] = sum_{f = 2 + 6 b}^{7 + 6 b} P[i][f], b = 0 .. 15
  smoothing S[i][b] = mean of E[j][b] over max(0, i - h) <= j <= min(F - 1, i + h)
  floor     N[i][b] = min of S[j][b] over max(0, i - W) <= j <= min(F - 1, i + W)            (a NaN wins the minimum)
  statistic g = (S + e0) / (beta N + e0);  t = g - 1 - ln g where g > 1, NaN where g is NaN, else 0;  L[i] = (1 / 16) sum_b t[i][b]
  decision  flag[i] = L[i] > theta
"""
import numpy as np

HOP, NFFT, LEAD, BANDS, BAND_BINS, FIRST_BIN = 256, 400, 72, 16, 6, 2
DEFAULTS = dict(h=2, W=94, beta=2.0, theta=0.15, e0=1e-12)
BAND_REL = 0.05                    # the decision band |L64 - theta| <= BAND_REL * theta inside which a flag may differ
SAMPLE_RATE = 16000


def frames_of(n: int) -> int:
    return 0 if n <= HOP else (n - 1) // HOP


def hann(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)).astype(dtype)


def _dft_bins(dtype):
    """cos and -sin of 2 pi m f / 400 for m = 0 .. 399 and the bins f = 2 .. 97 -> two [400, 96] matrices."""
    f = np.arange(FIRST_BIN, FIRST_BIN + BANDS * BAND_BINS)
    a = 2.0 * np.pi * ((np.arange(NFFT)[:, None] * f[None, :]) % NFFT) / NFFT
    return np.cos(a).astype(dtype), (-np.sin(a)).astype(dtype)


def band_energies(x, dtype=np.float64, chunk=16384):
    """-> E [F, 16] in ``dtype``."""
    x = np.asarray(x).astype(dtype)
    n = x.shape[0]
    F = frames_of(n)
    E = np.zeros((F, BANDS), dtype)
    if F == 0:
        return E
    xp = np.zeros(LEAD + max(n, HOP * (F - 1) + NFFT), dtype)
    xp[LEAD:LEAD + n] = x
    w, (C, S) = hann(dtype), _dft_bins(dtype)
    scale = dtype(1.0) / dtype(NFFT * NFFT)
    for i0 in range(0, F, chunk):
        i1 = min(F, i0 + chunk)
        idx = HOP * np.arange(i0, i1)[:, None] + np.arange(NFFT)[None, :]          # xp[k + 72] = x[k]: frame i starts at 256 i - 72
        y = xp[idx] * w[None, :]
        P = ((y @ C) ** 2 + (y @ S) ** 2) * scale
        E[i0:i1] = P.reshape(i1 - i0, BANDS, BAND_BINS).sum(axis=2, dtype=dtype)
    return E


def statistic_from_energies(E, h=2, W=94, beta=2.0, theta=0.15, e0=1e-12):
    """E [F, 16] -> L [F], every step in E's dtype."""
    dtype = E.dtype.type
    F = E.shape[0]
    if F == 0:
        return np.zeros(0, dtype)
    pad = np.zeros((h, BANDS), dtype)
    Ep = np.concatenate([pad, E, pad])
    valid = np.concatenate([np.zeros(h), np.ones(F), np.zeros(h)])
    acc, cnt = np.zeros((F, BANDS), dtype), np.zeros(F)
    for k in range(2 * h + 1):                                                    # ascending j; a frame outside the grid adds an exact 0
        acc = acc + Ep[k:k + F]
        cnt = cnt + valid[k:k + F]
    S = acc / cnt.astype(dtype)[:, None]
    inf = np.full((W, BANDS), np.inf, dtype)
    Sp = np.concatenate([inf, S, inf])
    N = Sp[0:F]
    for k in range(1, 2 * W + 1):
        N = np.minimum(N, Sp[k:k + F])                                             # np.minimum propagates a NaN
    with np.errstate(all="ignore"):
        g = (S + dtype(e0)) / (dtype(beta) * N + dtype(e0))
        t = np.where(g > 1, (g - dtype(1)) - np.log(g), np.where(np.isnan(g), dtype(np.nan), dtype(0))).astype(dtype)
    L = np.zeros(F, dtype)
    for b in range(BANDS):
        L = L + t[:, b]
    return L * dtype(1.0 / BANDS)


def statistic(x, h=2, W=94, beta=2.0, theta=0.15, e0=1e-12, dtype=np.float64):
    return statistic_from_energies(band_energies(x, dtype), h, W, beta, theta, e0)


def flags_of(L, theta=0.15):
    with np.errstate(invalid="ignore"):
        return np.asarray(L) > theta


def in_band(L64, theta=0.15):
    """Frames whose reference statistic is so close to the threshold that f32 arithmetic may decide either way."""
    return np.abs(np.asarray(L64, np.float64) - theta) <= BAND_REL * theta


# ----------------------------------------------------------------------------- synthetic signals
def _burst(rng, n):
    t = np.arange(n) / SAMPLE_RATE
    f0 = rng.uniform(90.0, 220.0)
    phase = 2.0 * np.pi * f0 * (t - 0.02 / (2.0 * np.pi * 3.0) * np.cos(2.0 * np.pi * 3.0 * t))     # f(t) = f0 (1 + 0.02 sin(2 pi 3 t))
    y = np.zeros(n)
    for k in range(1, 25):
        amp = 1.0 / (1.0 + ((k * f0 - 600.0) / 500.0) ** 2) + 0.3 / (1.0 + ((k * f0 - 1800.0) / 400.0) ** 2)
        y += amp * np.sin(k * phase)
    y *= 0.55 + 0.45 * np.sin(2.0 * np.pi * 4.0 * t - np.pi / 2.0)
    ramp = min(int(0.02 * SAMPLE_RATE), n // 2)
    y[:ramp] *= np.arange(ramp) / ramp
    y[n - ramp:] *= np.arange(ramp, 0, -1) / ramp
    return y


def synth(seed, duration_s, snr_db, kind="white", bursts=None):
    """-> (x f32 [n], truth bool [F], counted bool [F], bursts [(start_sample, end_sample)]).  Harmonic bursts (rms 0.1 over their own
    samples) in Gaussian noise, white or pink, burst-rms / noise-rms = the SNR.  Bursts start at 1.0 s, last U(0.4, 1.5) s with gaps of
    U(0.3, 2.0) s, and end before duration - 1.5 s (``bursts``: fixed (start_s, end_s) pairs instead).  truth: most of the frame's 256
    samples lie in a burst.  counted: not within 3 frames before .. 4 frames after a truth boundary."""
    rng = np.random.default_rng(seed)
    n = int(round(duration_s * SAMPLE_RATE))
    spans = []
    if bursts is None:
        t = 1.0
        while True:
            dur = rng.uniform(0.4, 1.5)
            if t + dur > duration_s - 1.5:
                break
            spans.append((int(t * SAMPLE_RATE), int((t + dur) * SAMPLE_RATE)))
            t += dur + rng.uniform(0.3, 2.0)
    else:
        spans = [(int(a * SAMPLE_RATE), int(b * SAMPLE_RATE)) for a, b in bursts]
    sig, inside = np.zeros(n), np.zeros(n, bool)
    for a, b in spans:
        sig[a:b] = _burst(rng, b - a)
        inside[a:b] = True
    if spans:
        sig *= 0.1 / np.sqrt(np.mean(sig[inside] ** 2))
    noise = rng.standard_normal(n)
    if kind == "pink":
        spec = np.fft.rfft(noise)
        spec[1:] /= np.sqrt(np.arange(1, spec.shape[0]))
        noise = np.fft.irfft(spec, n)
    elif kind != "white":
        raise ValueError(kind)
    noise *= (0.1 / 10.0 ** (snr_db / 20.0)) / np.sqrt(np.mean(noise ** 2))
    x = (sig + noise).astype(np.float32)
    F = frames_of(n)
    truth = inside[:F * HOP].reshape(F, HOP).sum(1) > HOP // 2
    counted = np.ones(F, bool)
    for b in np.flatnonzero(truth[1:] != truth[:-1]) + 1:                          # b: the first frame of the new state
        counted[max(0, b - 3):b + 5] = False
    return x, truth, counted, spans


def tone(freqs, duration_s, amplitude=0.1):
    t = np.arange(int(duration_s * SAMPLE_RATE)) / SAMPLE_RATE
    return (amplitude * sum(np.sin(2.0 * np.pi * f * t) for f in freqs) / len(freqs)).astype(np.float32)


# ----------------------------------------------------------------------------- the inputs of tests/test_gpu_vad.py
CHORD = (261.63, 392.0, 523.25, 783.99)        # C4 G4 C5 G5: partials at least 130 Hz apart (closer ones beat inside one band: not stationary)
EDGE_BURSTS = ((0.2, 0.5), (0.9, 1.6), (2.2, 3.0), (4.0, 5.5), (7.0, 8.4))


def gpu_signals():
    """name -> (x, truth, counted, bursts): the four 15 s recordings of the statistic and decision tests."""
    return {f"{kind}-{snr}dB": synth(0, 15.0, snr, kind) for kind in ("white", "pink") for snr in (20, 10)}


def edge_base():
    """9 s at 10 dB with bursts from 0.2 s on, so that every prefix used as an edge case holds speech and noise."""
    return synth(3, 9.0, 10, "white", bursts=EDGE_BURSTS)[0]


def samples_for_frames(F: int, extra: int = 1) -> int:
    """A length n with frames_of(n) == F (F >= 1): 256 F + extra, 1 <= extra <= 256."""
    return HOP * F + extra


def edge_frame_counts(tile: int, energy_frames: int, W: int = 94, h: int = 2):
    """The frame counts at which the kernels change path: around the noise window, the statistic tile and the energy workgroup."""
    return sorted({1, 2, 3, h, h + 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 2 * W + 2, tile - 1, tile, tile + 1, 2 * tile + 1,
                   energy_frames - 1, energy_frames, energy_frames + 1, 2 * energy_frames + 1} - {0})

"""Float64 numpy definition of the three members that complete the production chain on the device (``DeviceProductionAugment``,
tiny_audio_amd/csrc/augment.hip, DESIGN.md section 3 "Device-side augmentation"): short noises, the seven-band EQ and the band-limit,
and of the whole chain in the reference's ``Compose`` order (tiny_audio/augmentation.py:153-216): RIR, background noise, short noises,
Gaussian floor, EQ, clipping, band-limit.  The first four stages are tests/augment_ref.py's, unchanged.

``audiomentations`` is not installable here; the stages are RESTATED from its published behaviour (AddShortNoises, SevenBandParametricEQ,
LowPassFilter, BandPassFilter).  Nothing here is pinned against it.

A cascade is an array [S, 5] of sections (b0, b1, b2, a1, a2), a0 = 1.  ``sos_run`` is the recurrence itself (direct form II
transposed, the form of scipy.signal.sosfilt), in any numpy float type: float64 defines the result, ``numpy.longdouble`` measures how
much of a difference is float64 rounding noise.  ``sos_chunked`` restates it the way the device evaluates it in parallel over time.
"""
import numpy as np

from tests import augment_ref as R


# ----------------------------------------------------------------------------- cascades of second-order sections
def sos_run(x, sos, state=None, dtype=np.float64):
    """x [..., n] through the cascade from ``state`` [..., S, 2] (zero when None) -> (y [..., n], the final state), all in ``dtype``.
    Leading axes of x are independent signals, advanced together."""
    x = np.asarray(x, dtype=dtype)
    sos = np.asarray(sos, dtype=dtype).reshape(-1, 5)
    S, n = len(sos), x.shape[-1]
    s = np.zeros(x.shape[:-1] + (S, 2), dtype=dtype) if state is None else np.array(state, dtype=dtype)
    y = np.empty_like(x)
    for t in range(n):
        v = x[..., t]
        for k in range(S):
            b0, b1, b2, a1, a2 = sos[k]
            w = b0 * v + s[..., k, 0]
            s[..., k, 0] = b1 * v - a1 * w + s[..., k, 1]
            s[..., k, 1] = b2 * v - a2 * w
            v = w
        y[..., t] = v
    return y, s


def sos_filter(x, sos):
    """The definition: the cascade over the whole clip from a zero state, float64."""
    return sos_run(x, sos)[0]


def sos_chunked(x, sos, T):
    """The same result the way the device forms it.  A cascade of S sections is one linear system with 2 S states, so with the clip cut
    into chunks of T samples:  s[c + 1] = M s[c] + z[c],  M = the zero-input map of a chunk (column j = T zero-input steps from the unit
    state e_j), z[c] = the final state of chunk c run from a zero state.  Phase 1: every z[c] (independent); phase 2: the entry states
    (sequential over chunks, 2 S x 2 S each); phase 3: every chunk again from its entry state (independent)."""
    x = np.asarray(x, dtype=np.float64)
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 5)
    S, n = len(sos), len(x)
    chunks = [x[c: c + T] for c in range(0, n, T)]
    z = [sos_run(c, sos)[1].reshape(-1) for c in chunks[:-1]]                                   # phase 1
    M = np.stack([sos_run(np.zeros(T), sos, e.reshape(S, 2))[1].reshape(-1) for e in np.eye(2 * S)], axis=1)
    entry = [np.zeros(2 * S)]
    for zc in z:                                                                               # phase 2
        entry.append(M @ entry[-1] + zc)
    return np.concatenate([sos_run(c, sos, s.reshape(S, 2))[0] for c, s in zip(chunks, entry)]) if n else x.copy()   # phase 3


def sos_l1_gain(sos, n: int) -> float:
    """sum |h[t]|, t < n: the factor by which the cascade can enlarge the largest error of its input."""
    imp = np.zeros(n)
    imp[0] = 1.0
    return float(np.abs(sos_filter(imp, sos)).sum())


# ----------------------------------------------------------------------------- short noises
def fade_envelope(length: int, f_in: int, f_out: int, floor_db: float) -> np.ndarray:
    """a_in a_out over an event of ``length`` samples: linear in dB from -floor_db to 0 over the first f_in samples, back over the last f_out."""
    i = np.arange(length, dtype=np.float64)
    a = np.ones(length)
    if f_in > 0:
        m = i < f_in
        a[m] *= 10.0 ** (-(floor_db / 20.0) * (1.0 - (i[m] + 1.0) / f_in))
    if f_out > 0:
        m = i >= length - f_out
        a[m] *= 10.0 ** (-(floor_db / 20.0) * (1.0 - (length - i[m]) / f_out))
    return a


def short_noises(x, events, pool, floor_db: float):
    """events: a list of (j, o, length, t0, f_in, f_out, snr_db), added in list order -> (y, sum_e |g_e a v| per sample, [g_e]).
    R = rms of x over the clip, once; r_e = rms of the event's own window before the fades; an event with r_e < 1e-9 is skipped
    (g_e = 0); samples past the clip's end are dropped."""
    x = np.asarray(x, dtype=np.float64)
    n, Rx = len(x), R.rms(x)
    y, mag, gains = x.copy(), np.zeros(n), []
    for (j, o, length, t0, f_in, f_out, snr_db) in events:
        v = np.asarray(pool[j], dtype=np.float64)[o: o + length]
        assert len(v) == length >= 1 and t0 >= 0
        r = R.rms(v)
        if r < 1e-9:
            gains.append(0.0)
            continue
        g = Rx * 10.0 ** (-float(snr_db) / 20.0) / r
        gains.append(g)
        keep = max(min(length, n - t0), 0)
        add = (g * fade_envelope(length, f_in, f_out, floor_db) * v)[:keep]
        y[t0: t0 + keep] += add
        mag[t0: t0 + keep] += np.abs(add)
    return y, mag, gains


# ----------------------------------------------------------------------------- the chain
def chain(x, b: int, *, ir=None, rir_peak=0.5, noise=None, noise_start=0, noise_snr_db=None, events=(), event_pool=(), fade_floor_db=70.0,
          gauss_snr_db=None, seed=0, offset=0, eq_sos=None, clip_pct=0, bl_sos=None):
    """One clip through the stages that are on -> (result, [the clip after each of the seven stages])."""
    y = np.asarray(x, dtype=np.float64).copy()
    after = []
    if ir is not None:
        y = R.rir(y, ir, rir_peak)
    after.append(y)
    if noise is not None:
        y = R.background(y, noise, noise_start, noise_snr_db)
    after.append(y)
    if len(events):
        y = short_noises(y, events, event_pool, fade_floor_db)[0]
    after.append(y)
    if gauss_snr_db is not None and np.isfinite(gauss_snr_db):
        y = R.gaussian(y, gauss_snr_db, seed, offset, b)
    after.append(y)
    if eq_sos is not None and len(eq_sos):
        y = sos_filter(y, eq_sos)
    after.append(y)
    if clip_pct:
        y = R.clipping(y, clip_pct)
    after.append(y)
    if bl_sos is not None and len(bl_sos):
        y = sos_filter(y, bl_sos)
    after.append(y)
    return y, after


# ----------------------------------------------------------------------------- the cascades the tests share
def cascades(sample_rate: int = 16000):
    """name -> [S, 5]: every section count the kernel dispatches on that matters (a first-order section, one, two, seven, eight), the
    slowest-decaying shelf of the EQ's ranges and a peak whose memory spans many chunks."""
    import scipy.signal
    from tiny_audio_amd.augmentation import rbj_section

    def butter(order, fc):
        sos = scipy.signal.butter(order, fc, fs=sample_rate, output="sos")
        return sos[:, [0, 1, 2, 4, 5]] / sos[:, 3:4]
    eq7 = np.stack([rbj_section("low_shelf", 42.0, 0.1, 4.0, sample_rate), rbj_section("peaking", 150.0, 1.0, -4.0, sample_rate),
                    rbj_section("peaking", 300.0, 0.9, 4.0, sample_rate), rbj_section("peaking", 700.0, 1.1, -4.0, sample_rate),
                    rbj_section("peaking", 1500.0, 1.0, 4.0, sample_rate), rbj_section("peaking", 3000.0, 1.0, -4.0, sample_rate),
                    rbj_section("high_shelf", 6000.0, 0.5, 4.0, sample_rate)])
    return {"first-order": butter(1, 3000.0), "one section": butter(2, 5000.0), "butterworth 3": butter(3, 3000.0),
            "butterworth 4": butter(4, 7500.0), "eq, seven sections": eq7,
            "eight sections": np.concatenate([eq7, rbj_section("peaking", 5000.0, 2.0, 3.0, sample_rate)[None]]),
            "20 Hz peak, Q 5": rbj_section("peaking", 20.0, 5.0, 4.0, sample_rate)[None]}


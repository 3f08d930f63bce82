"""Float64 numpy definition of the device-side waveform augmentation (tiny_audio_amd/csrc/augment.hip, DESIGN.md section 3
"Device-side augmentation"): the four numeric stages of the reference's production chain, in the reference's order -- RIR
convolution, background noise at an SNR, Gaussian floor at an SNR, percentile clipping.

``audiomentations`` is not installable here; the stages are RESTATED from its published behaviour (ApplyImpulseResponse,
AddBackgroundNoise, AddGaussianSNR, ClippingDistortion), the way the trl collation was.  Nothing here is pinned against it.

Every stage acts on one clip ``x`` = the real samples [0, n) (the caller cuts the padding off), in float64, and returns a new array.
The convolution is the direct sum (``numpy.convolve``), not a transform, so it is independent of the thing it checks.
"""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on Python integers (one counter) -> (w0, w1, w2, w3)."""
    c0, c1, c2, c3, k0, k1 = (int(v) & _MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def _philox_vec(c0, c1, c2, c3, k0, k1):
    """The same over a uint64 array of counter words c0 (c1..c3 and the key are scalars) -> uint64 [4, len(c0)]."""
    c0 = np.asarray(c0, dtype=np.uint64)
    c = [c0, np.full_like(c0, int(c1) & _MASK), np.full_like(c0, int(c2) & _MASK), np.full_like(c0, int(c3) & _MASK)]
    k0, k1 = int(k0) & _MASK, int(k1) & _MASK
    m = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c)


def normals(seed: int, offset: int, b: int, n: int) -> np.ndarray:
    """z[b, 0:n] float64: w = philox(counter = (t >> 2, b, lo32(offset), hi32(offset)), key = (lo32(seed), hi32(seed))); samples
    4q, 4q+1 from (w0, w1), 4q+2, 4q+3 from (w2, w3) by Box-Muller with u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24."""
    nq = (n + 3) // 4
    w = _philox_vec(np.arange(nq, dtype=np.uint64), b, offset & _MASK, (offset >> 32) & _MASK, seed & _MASK, (seed >> 32) & _MASK)
    z = np.empty((nq, 4), dtype=np.float64)
    for h in range(2):
        u1 = ((w[2 * h] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[2 * h + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * h] = r * np.cos(2.0 * np.pi * u2)
        z[:, 2 * h + 1] = r * np.sin(2.0 * np.pi * u2)
    return z.reshape(-1)[:n]


def rms(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def rir_full(x, h, rir_peak=0.5) -> np.ndarray:
    """The FULL convolution [0, n + m - 1), peak-scaled: what the kept part is cut from."""
    y = np.convolve(np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64))
    peak = float(np.max(np.abs(y)))
    if rir_peak is not None and peak > 0.0:
        y = y * (float(rir_peak) / peak)
    return y


def rir(x, h, rir_peak=0.5) -> np.ndarray:
    return rir_full(x, h, rir_peak)[: len(x)]


def noise_window(noise, start: int, n: int) -> np.ndarray:
    noise = np.asarray(noise, dtype=np.float64)
    return noise[(int(start) + np.arange(n)) % len(noise)]


def background_gain(x, noise, start: int, snr_db: float) -> float:
    """g of y = x + g v; 0.0 when the stage is skipped (a silent window)."""
    v = noise_window(noise, start, len(x))
    rv = rms(v)
    return 0.0 if rv < 1e-9 else rms(x) / (10.0 ** (float(snr_db) / 20.0)) / rv


def background(x, noise, start: int, snr_db: float) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    g = background_gain(x, noise, start, snr_db)
    return x.copy() if g == 0.0 else x + g * noise_window(noise, start, len(x))


def gaussian_sigma(x, snr_db: float) -> float:
    return rms(x) / (10.0 ** (float(snr_db) / 20.0))


def gaussian(x, snr_db: float, seed: int, offset: int, b: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return x + gaussian_sigma(x, snr_db) * normals(seed, offset, b, len(x))


def clip_thresholds(x, pct: int):
    q = int(pct) // 2
    lo, hi = np.percentile(np.asarray(x, dtype=np.float64), [q, 100 - q])
    return float(lo), float(hi)


def clipping(x, pct: int) -> np.ndarray:
    lo, hi = clip_thresholds(x, pct)
    return np.clip(np.asarray(x, dtype=np.float64), lo, hi)


def chain(x, b: int, *, ir=None, rir_peak=0.5, noise=None, noise_start=0, noise_snr_db=None, gauss_snr_db=None, seed=0, offset=0,
          clip_pct=0):
    """One clip through the stages that are on (None / 0 = off) -> (result, [the clip after each of the four stages])."""
    y = np.asarray(x, dtype=np.float64).copy()
    after = []
    if ir is not None:
        y = rir(y, ir, rir_peak)
    after.append(y)
    if noise is not None:
        y = background(y, noise, noise_start, noise_snr_db)
    after.append(y)
    if gauss_snr_db is not None and np.isfinite(gauss_snr_db):
        y = gaussian(y, gauss_snr_db, seed, offset, b)
    after.append(y)
    if clip_pct:
        y = clipping(y, clip_pct)
    after.append(y)
    return y, after

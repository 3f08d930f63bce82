"""-m "not gpu": the float64 definition of the voice activity detector (tests/vad_ref.py) on the synthetic signals of its issue --
every figure quoted in DESIGN.md section 3, "Voice activity detection", is recomputed here.  None of this is real speech: the
constants are design choices and stay unvalidated (DESIGN.md says so)."""
import numpy as np
import pytest

from tests import vad_ref as R
from tiny_audio_amd import ops

THETA = R.DEFAULTS["theta"]


def _quality(snr, kind, seed):
    x, truth, counted, spans = R.synth(seed, 15.0, snr, kind)
    L = R.statistic(x)
    f = R.flags_of(L)
    return x, L, int((f & ~truth & counted).sum()), int((~f & truth & counted).sum()), int((truth & counted).sum()), len(spans)


def test_frames_of_is_the_diarizers_loop_count():
    for n in (0, 1, 256, 257, 512, 513, 1000, 4096):
        assert R.frames_of(n) == len(range(0, n - 256, 256)) == ops.vad_frames(n), n
    assert [R.frames_of(n) for n in (256, 257, 512, 513, 1000)] == [0, 1, 1, 2, 3]
    for F in (1, 2, 255, 256):
        assert R.frames_of(R.samples_for_frames(F)) == F == R.frames_of(R.samples_for_frames(F, 256))


def test_zeros_give_exactly_zero():
    for dtype in (np.float64, np.float32):
        L = R.statistic(np.zeros(16000, np.float32), dtype=dtype)
        assert L.shape == (62,) and L.dtype == dtype and (L == 0).all()
    assert R.statistic(np.zeros(256, np.float32)).shape == (0,)


@pytest.mark.parametrize("kind", ["white", "pink"])
@pytest.mark.parametrize("snr", [20, 10])
def test_synthetic_quality_no_false_alarm_no_miss(kind, snr):
    for seed in range(3):
        _x, _L, fa, miss, speech, bursts = _quality(snr, kind, seed)
        print(f"{kind} {snr} dB seed {seed}: {bursts} bursts, {speech} counted speech frames, false alarms {fa}, misses {miss}")
        assert bursts >= 4 and speech >= 200
        assert fa == 0 and miss == 0


def test_stationary_inputs_are_not_speech():
    x = (0.03 * np.random.default_rng(0).standard_normal(60 * 16000)).astype(np.float32)
    L = R.statistic(x)
    print(f"60 s of white noise: largest L {L.max():.4f} against theta {THETA}")
    assert not R.flags_of(L).any() and L.max() < THETA
    for freqs in ((440.0,), R.CHORD):
        f = R.flags_of(R.statistic(R.tone(freqs, 15.0)))
        print(f"tone {freqs}: {100 * f.mean():.2f} % of frames, the last at frame {np.flatnonzero(f).max(initial=-1)}")
        assert f.mean() <= 0.01
        assert not f[10:].any(), "the onset only"


def test_level_invariance_quantisation_and_silence():
    x, *_ = R.synth(0, 15.0, 10, "white")
    L = R.statistic(x)
    f = R.flags_of(L)
    for scale in (0.1, 0.01):
        L2 = R.statistic((x * np.float32(scale)).astype(np.float32))
        flipped = (R.flags_of(L2) != f) & ~R.in_band(L) & ~R.in_band(L2)
        print(f"scale {scale}: {(R.flags_of(L2) != f).sum()} flags flipped, {flipped.sum()} outside the band")
        assert not flipped.any()
    x16 = (np.round(np.clip(x, -1.0, 1.0) * 32767.0) / 32767.0).astype(np.float32)
    assert ((R.flags_of(R.statistic(x16)) != f) & ~R.in_band(L)).sum() == 0
    assert not R.flags_of(R.statistic(np.zeros(48000, np.float32))).any()


def test_float32_restatement_and_band_share_of_every_gpu_signal():
    """What keeps the GPU comparison from hiding failures: few frames lie inside the decision band, and f32 arithmetic in numpy's own
    order stays far inside it."""
    signals = {k: v[0] for k, v in R.gpu_signals().items()}
    base = R.edge_base()
    for F in R.edge_frame_counts(ops.VAD_TILE, ops.VAD_ENERGY_FRAMES):
        signals[f"edge-{F}"] = base[:R.samples_for_frames(F)]
    for kind in ("white", "pink"):
        for seed in range(3):
            signals[f"{kind}-5dB-{seed}"] = R.synth(seed, 15.0, 5, kind)[0]
    worst = 0.0
    for name, x in signals.items():
        L64, L32 = R.statistic(x), R.statistic(x, dtype=np.float32)
        band = R.in_band(L64)
        e32 = float(np.max(np.abs(L32 - L64) / (L64 + THETA)))
        worst = max(worst, e32)
        assert band.sum() <= 0.02 * len(L64), (name, band.sum(), len(L64))
        assert e32 <= 5e-4, (name, e32)
        assert ((R.flags_of(L32) != R.flags_of(L64)) & ~band).sum() == 0, name
    print(f"{len(signals)} signals: largest |L32 - L64| / (L64 + theta) = {worst:.3g}")


def test_a_nan_sample_reaches_its_neighbourhood_only():
    x, *_ = R.synth(1, 6.0, 10, "white")
    y = x.copy()
    y[40000] = np.nan                                                               # frame 156
    L, Ly = R.statistic(x, W=20), R.statistic(y, W=20)
    bad = np.isnan(Ly)
    assert bad[156] and not R.flags_of(Ly)[bad].any()
    assert np.flatnonzero(bad).min() >= 156 - 1 - 2 - 20 and np.flatnonzero(bad).max() <= 156 + 1 + 2 + 20
    far = np.abs(np.arange(len(L)) - 156) > 1 + 2 + 2 * 20                          # beyond the reach of the NaN's floor as well
    assert np.array_equal(L[far], Ly[far])

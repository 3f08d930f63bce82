"""Device-side waveform augmentation, host side (no GPU): the float64 definition (tests/augment_ref.py) against scipy / numpy / the
library's numpy Philox, the plan drawn by ``DeviceWaveAugment``, the refusals, the host-only size queries, the operator's
registration, and the dry-run plumbing of the new entry points (as tests/test_packing_host.py does for its own: arguments are
marshalled through the real ctypes prototypes, nothing is computed)."""
import warnings

import numpy as np
import pytest
import scipy.signal
import torch

from tests import augment_ref as R
from tiny_audio_amd import _lib, augmentation
from tiny_audio_amd.augmentation import CONV_DIRECT, CONV_HOP, DeviceWaveAugment
from tiny_audio_amd.lora_dropout import philox4x32_10 as philox_np


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


# ----------------------------------------------------------------------------- the float64 definition
@pytest.mark.parametrize("n,m", [(1, 1), (50, 7), (7, 50), (300, 300)])
def test_ref_rir_is_fftconvolve_in_float64(n, m):
    rng = np.random.default_rng(n * 1000 + m)
    x, h = rng.standard_normal(n), rng.standard_normal(m) * np.exp(-np.arange(m) / 20.0)
    full = scipy.signal.fftconvolve(x, h)
    assert full.dtype == np.float64
    np.testing.assert_allclose(R.rir(x, h, rir_peak=None), full[:n], rtol=0, atol=1e-12 * np.abs(full).max())
    peak = np.abs(full).max()
    y = R.rir_full(x, h, rir_peak=0.5)
    np.testing.assert_allclose(y, full * (0.5 / peak), rtol=0, atol=1e-12)
    assert abs(np.abs(y).max() - 0.5) < 1e-12 and len(y) == n + m - 1
    # the peak is taken over the FULL convolution: for m > n it may lie in the part that is not kept
    assert np.abs(R.rir(x, h)).max() <= 0.5 + 1e-12
    assert np.array_equal(R.rir(np.zeros(n), h), np.zeros(n))          # P = 0: no scaling, no division


@pytest.mark.parametrize("n", [1, 2, 3, 1001])
@pytest.mark.parametrize("pct", [1, 2, 9, 10])
def test_ref_clipping_is_numpy_percentile(n, pct):
    x = np.random.default_rng(n + pct).standard_normal(n)
    lo, hi = np.percentile(x, [pct // 2, 100 - pct // 2])
    assert R.clip_thresholds(x, pct) == (lo, hi)
    y = R.clipping(x, pct)
    assert y.min() == max(lo, x.min()) and y.max() == min(hi, x.max())
    inside = (x > lo) & (x < hi)
    assert np.array_equal(y[inside], x[inside])
    if pct // 2 == 0:
        assert np.array_equal(y, x)


def test_ref_philox_and_normals_match_the_librarys_numpy_philox():
    counters = [(0, 0, 0, 0, 0, 0), (1, 2, 3, 4, 5, 6), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF),
                (12345, 7, 0xDEADBEEF, 1, 0x9E3779B9, 42)]
    for c in counters:
        assert R.philox4x32_10(*c) == tuple(int(v) for v in philox_np(*c))
    # Random123's known answer for the all-ones counter and key
    assert R.philox4x32_10(*counters[2]) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    seed, offset, b, n = 0x1234567890AB, (3 << 32) | 17, 5, 23
    z = R.normals(seed, offset, b, n)
    for t in (0, 1, 2, 3, 4, 21, 22):
        w = [int(v) for v in philox_np(t >> 2, b, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)]
        wa, wb = (w[0], w[1]) if (t & 3) < 2 else (w[2], w[3])
        u1, u2 = ((wa >> 8) + 1) * 2.0 ** -24, (wb >> 8) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        want = r * (np.cos(2 * np.pi * u2) if (t & 1) == 0 else np.sin(2 * np.pi * u2))
        assert abs(z[t] - want) < 1e-14, t
    big = R.normals(1, 0, 0, 200000)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1.0) < 0.01 and np.abs(big).max() <= 5.77
    assert not np.array_equal(R.normals(1, 1, 0, 64), big[:64]) and not np.array_equal(R.normals(1, 0, 1, 64), big[:64])


def test_ref_background_and_gaussian_hit_their_snr():
    rng = np.random.default_rng(3)
    x, noise = rng.standard_normal(16000), rng.standard_normal(100)
    y = R.background(x, noise, 93, 12.0)
    assert abs(10 * np.log10(np.sum(x * x) / np.sum((y - x) ** 2)) - 12.0) < 1e-9
    v = R.noise_window(noise, 93, 16000)
    assert np.array_equal(v[:7], noise[93:100]) and np.array_equal(v[7:107], noise)          # the window wraps
    assert np.array_equal(R.background(x, np.zeros(50), 0, 12.0), x)                         # a silent window: skipped
    g = R.gaussian(x, 20.0, 9, 0, 0)
    assert abs(10 * np.log10(np.sum(x * x) / np.sum((g - x) ** 2)) - 20.0) < 0.25


# ----------------------------------------------------------------------------- the plan
def _pools():
    rng = np.random.default_rng(0)
    return [rng.standard_normal(m).astype(np.float32) for m in (5, 3000)], [rng.standard_normal(m).astype(np.float32) for m in (100, 40000)]


def _aug(**kw):
    rirs, noises = _pools()
    base = dict(rir_pool=rirs, noise_pool=noises, gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, clipping_prob=0.1, device="cpu",
                seed=7)
    base.update(kw)
    return DeviceWaveAugment(**base)


def test_plan_is_reproducible_and_advances():
    lens = [16000, 12000, 8000, 4000] * 8
    a, b = _aug(), _aug()
    p1, p2, q1 = a.plan(lens), a.plan(lens), b.plan(lens)
    fields = ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct")
    for f in fields:
        assert np.array_equal(getattr(p1, f), getattr(q1, f), equal_nan=True), f
    assert (p1.seed, p1.offset) == (q1.seed, q1.offset) == (7, 0) and p2.offset == 1
    assert any(not np.array_equal(getattr(p1, f), getattr(p2, f), equal_nan=True) for f in fields)
    assert not np.array_equal(_aug(seed=8).plan(lens).noise_snr_db, p1.noise_snr_db, equal_nan=True)
    # ranges
    on = p1.noise_idx >= 0
    assert on.any() and (~on).any()
    assert ((p1.noise_snr_db[on] >= 5.0) & (p1.noise_snr_db[on] <= 30.0)).all() and np.isnan(p1.noise_snr_db[~on]).all()
    nlen = np.array([100, 40000])
    assert ((p1.noise_start[on] >= 0) & (p1.noise_start[on] < nlen[p1.noise_idx[on]])).all()
    assert ((p1.gauss_snr_db >= 20.0) & (p1.gauss_snr_db <= 40.0)).all()          # the floor is always on
    assert ((p1.clip_pct >= 0) & (p1.clip_pct <= 10)).all() and set(np.unique(p1.ir_idx)) <= {-1, 0, 1}
    assert p1.ir_idx.dtype == np.int32 and p1.noise_start.dtype == np.int64 and p1.clip_pct.dtype == np.int32


def test_probabilities_zero_and_one():
    lens = [1000] * 64
    off = _aug(rir_prob=0.0, prob=0.0, clipping_prob=0.0, gaussian_min_snr_db=None, gaussian_max_snr_db=None).plan(lens)
    assert (off.ir_idx == -1).all() and (off.noise_idx == -1).all() and (off.clip_pct == 0).all()
    assert np.isnan(off.gauss_snr_db).all() and np.isnan(off.noise_snr_db).all() and off.stages() == 0
    on = _aug(rir_prob=1.0, prob=1.0, clipping_prob=1.0).plan(lens)
    assert (on.ir_idx >= 0).all() and (on.noise_idx >= 0).all() and (on.clip_pct >= 1).all() and np.isfinite(on.gauss_snr_db).all()
    assert on.stages() == 15
    none = DeviceWaveAugment(rir_prob=1.0, prob=1.0, device="cpu").plan(lens)          # no pools: nothing to draw from
    assert (none.ir_idx == -1).all() and (none.noise_idx == -1).all() and none.stages() == 0
    amp = on.pack()[64 * (8 + 12):].view(np.float32)
    np.testing.assert_allclose(amp[:64], 10.0 ** (-on.noise_snr_db.astype(np.float64) / 20.0), rtol=1e-6)
    assert np.array_equal(off.pack()[64 * (8 + 12):].view(np.float32), np.zeros(128, np.float32))


@pytest.mark.parametrize("name", ["short_noises_prob", "eq_prob", "bandlimit_prob"])
def test_unbuilt_members_raise_by_name(name):
    with pytest.raises(NotImplementedError, match=name):
        DeviceWaveAugment(device="cpu", **{name: 0.1})
    DeviceWaveAugment(device="cpu", **{name: 0.0})


def test_long_impulse_responses_are_cut_and_said_so():
    with pytest.warns(UserWarning, match="max_ir_seconds"):
        a = DeviceWaveAugment(rir_pool=[np.ones(100, np.float32), np.ones(20, np.float32)], max_ir_seconds=0.002, device="cpu")
    assert [len(h) for h in a.rir_pool] == [32, 20]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        DeviceWaveAugment(rir_pool=[np.ones(100, np.float32)], device="cpu")


# ----------------------------------------------------------------------------- the library boundary
def test_workspace_queries_run_without_a_gpu():
    L = _lib.lib()
    H = CONV_HOP
    assert H == 2048 and "#define TA_WAVE_CONV_HOP 2048" in open(_lib.HEADER).read()
    assert CONV_DIRECT == 32 and "#define TA_WAVE_CONV_DIRECT 32" in open(_lib.HEADER).read()
    B, Ls, taps = 32, 160000, 32000
    ws = L.ta_wave_conv_ws_bytes(B, Ls, taps)
    nbx, nout = (Ls - 1) // H + 2, -(-(Ls + taps - 1) // H)
    need = B * nbx * (H + 1) * 8 + B * Ls * 4 + B * nout * 8
    assert need <= ws <= need + 3 * 256 and ws < 80e6
    assert L.ta_wave_conv_ws_bytes(0, Ls, taps) == 0
    assert L.ta_wave_mix_scratch_floats(B, Ls) == B * 40 * 3 and L.ta_wave_mix_scratch_floats(1, 4097) == 6


def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "wave_augment" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.wave_augment.default._schema)
    assert s.startswith("ta355::wave_augment(Tensor wav, Tensor lens, Tensor desc, SymInt stages, SymInt seed, SymInt offset, SymInt handle)")
    h = torch_ops.register_module(_aug())
    with FakeTensorMode():
        out = torch.ops.ta355.wave_augment(torch.empty(3, 5000), torch.empty(3, dtype=torch.int64), torch.empty(3 * 28, dtype=torch.uint8),
                                           15, 1, 2, h)
        assert out.shape == (3, 5000) and out.dtype == torch.float32


def test_apply_plumbing(dry):
    aug = _aug(rir_prob=1.0, prob=1.0, clipping_prob=1.0)
    wav, lens = torch.zeros(4, 5000), torch.tensor([5000, 4000, 1, 300])
    dry.calls.clear()
    out = aug.apply(wav, lens, aug.plan(lens))
    assert out.shape == wav.shape and out.dtype == torch.float32 and out.data_ptr() != wav.data_ptr()
    assert dry.calls == ["ta_wave_fft_twiddles", "ta_wave_ir_spectra", "ta_wave_conv_f32", "ta_wave_mix_f32", "ta_wave_clip_f32"]
    dry.calls.clear()
    aug.apply(wav, lens, aug.plan(lens))                                   # the pool spectra are computed once
    assert dry.calls == ["ta_wave_conv_f32", "ta_wave_mix_f32", "ta_wave_clip_f32"]
    # a batch in which no clip uses a stage does not launch it; the copy always runs
    quiet = _aug(rir_prob=0.0, prob=0.0, clipping_prob=0.0, gaussian_min_snr_db=None, gaussian_max_snr_db=None)
    dry.calls.clear()
    quiet.apply(wav, lens, quiet.plan(lens))
    assert dry.calls == ["ta_wave_fft_twiddles", "ta_wave_ir_spectra", "ta_wave_conv_f32"]          # (its own pool's upload first)
    p = aug.plan(lens)
    p.ir_idx[0] = 2
    with pytest.raises(ValueError, match="pool"):
        aug.apply(wav, lens, p)
    with pytest.raises(ValueError, match="entries"):
        aug.apply(wav[:3], lens[:3], aug.plan(lens))


def test_feature_extractor_and_collator_pass_augment_through(dry):
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    from tiny_audio_amd.collator import DataCollator
    from tests.test_packing_host import ToyTokenizer, _Proj, _clips
    fe = LogMelFeatureExtractor(128, "cpu")
    clips = [np.zeros(1600, np.float32), np.zeros(800, np.float32)]
    fe(clips, sampling_rate=16000)                                         # (the first call also computes the mel ranges)
    dry.calls.clear()
    fe(clips, sampling_rate=16000)
    plain = list(dry.calls)
    assert not any(c.startswith("ta_wave_") for c in plain) and "ta_logmel_f32" in plain
    dry.calls.clear()
    fe(clips, sampling_rate=16000, augment=None)
    assert dry.calls == plain
    aug = _aug(rir_prob=1.0)
    dry.calls.clear()
    fe(clips, sampling_rate=16000, augment=aug)
    assert "ta_wave_conv_f32" in dry.calls and dry.calls.index("ta_wave_conv_f32") < dry.calls.index("ta_logmel_f32")
    before = aug._plans
    fe(clips, sampling_rate=16000, augment=aug, augment_plan=aug.plan([1600, 800]))
    assert aug._plans == before + 1                                        # a given plan is used; none is drawn behind it

    # the collator: without ``augment`` the feature extractor sees exactly today's call
    seen = []

    def spy(arrays, **kw):
        seen.append(kw)
        T = [len(a) // 160 for a in arrays]
        att = torch.zeros((len(arrays), max(T)), dtype=torch.int64)
        for i, t in enumerate(T):
            att[i, :t] = 1
        return {"input_features": torch.zeros((len(arrays), 8, max(T))), "attention_mask": att}

    today = dict(sampling_rate=16000, padding="longest", return_attention_mask=True, return_tensors="pt")
    DataCollator(ToyTokenizer(), spy, 16000, projector=_Proj())(_clips([1.0, 0.5]))
    DataCollator(ToyTokenizer(), spy, 16000, projector=_Proj(), augment=None)(_clips([1.0, 0.5]))
    assert seen == [today, today]
    DataCollator(ToyTokenizer(), spy, 16000, projector=_Proj(), augment=aug)(_clips([1.0, 0.5]))
    assert seen[2] == {**today, "augment": aug}
    assert augmentation.CONV_HOP == CONV_HOP

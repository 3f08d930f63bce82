"""The whole production chain on the device, host side (no GPU): the float64 definition of the three new members
(tests/augment_chain_ref.py) against scipy and against its own time-parallel restatement, the plan drawn by
``DeviceProductionAugment``, the filter design's refusals, the host-only size queries, the operator's registration, and the dry-run
plumbing of ``apply`` (arguments marshalled through the real ctypes prototypes; nothing is computed)."""
import numpy as np
import pytest
import scipy.signal
import torch

from tests import augment_chain_ref as C
from tests import augment_ref as R
from tiny_audio_amd import _lib, augmentation
from tiny_audio_amd.augmentation import (IIR_CHUNK, IIR_MAX_SECTIONS, MAX_EVENTS, DeviceProductionAugment, DeviceWaveAugment,
                                         ProductionAugmentPlan)

FIELDS = ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct", "ev_count", "ev_pool", "ev_off", "ev_len", "ev_t0",
          "ev_fade_in", "ev_fade_out", "ev_snr_db", "eq_nsec", "eq_sos", "bl_nsec", "bl_sos")


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _to_scipy(sos):
    return np.ascontiguousarray(np.concatenate([sos[:, :3], np.ones((len(sos), 1)), sos[:, 3:]], axis=1))


# ----------------------------------------------------------------------------- the float64 definition
@pytest.mark.parametrize("name", list(C.cascades()))
def test_ref_cascade_is_sosfilt_and_its_chunked_form_is_the_same_recurrence(name):
    """The sequential reference is scipy.signal.sosfilt's recurrence (same operations in the same order: equal to rounding noise); the
    chunked restatement -- what the device evaluates -- equals the sequential one to 1e-12 of the output's peak.  Chunks of 256,
    n = 6000 (23 whole chunks and a part), noise at amplitude 0.1."""
    sos = C.cascades()[name]
    x = np.random.default_rng(1).standard_normal(6000) * 0.1
    y = C.sos_filter(x, sos)
    want = scipy.signal.sosfilt(_to_scipy(sos), x)
    assert want.dtype == np.float64
    peak = np.abs(want).max()
    assert np.abs(y - want).max() <= 1e-13 * peak
    got = C.sos_chunked(x, sos, 256)
    print(f"{name}: peak {peak:.3f}, chunked against sequential {np.abs(got - y).max() / peak:.2e} of the peak")
    assert np.abs(got - y).max() <= 1e-12 * peak
    for n in (1, 255, 256, 257):                                            # the chunk edges of the restatement itself
        assert np.abs(C.sos_chunked(x[:n], sos, 256) - y[:n]).max() <= 1e-12 * peak
    assert C.sos_l1_gain(sos, 6000) >= np.abs(y).max() / np.abs(x).max() - 1e-9


def test_ref_event_reaches_its_snr_and_fades():
    rng = np.random.default_rng(2)
    x, pool = rng.standard_normal(16000), [rng.standard_normal(5000), np.zeros(100)]
    y, mag, gains = C.short_noises(x, [(0, 100, 4000, 3000, 0, 0, 7.0)], pool, 70.0)
    d = y - x
    assert not d[:3000].any() and not d[7000:].any()
    # a single unfaded event: its rms against the WHOLE input's rms is the asked SNR
    assert abs(20 * np.log10(R.rms(x) / R.rms(d[3000:7000])) - 7.0) < 1e-9
    assert np.allclose(mag, np.abs(d), rtol=0, atol=1e-14) and len(gains) == 1
    # the envelope: -D dB (less one step) at the first sample, 0 dB at the last faded one, 1 in between, mirrored at the end
    a = C.fade_envelope(1000, 100, 50, 70.0)
    assert abs(20 * np.log10(a[0]) + 70.0 * 0.99) < 1e-9 and a[99] == 1.0 and (a[100:950] == 1.0).all()
    assert abs(20 * np.log10(a[999]) + 70.0 * (1 - 1 / 50)) < 1e-9 and abs(20 * np.log10(a[950])) < 1e-9
    assert np.array_equal(C.fade_envelope(10, 0, 0, 70.0), np.ones(10))
    # past the end: dropped, with the gain of the whole event; a silent event: skipped; overlapping events add
    y2, _, g2 = C.short_noises(x, [(0, 0, 5000, 14000, 0, 0, 0.0)], pool, 70.0)
    assert np.allclose(y2[14000:] - x[14000:], g2[0] * pool[0][:2000]) and abs(g2[0] - R.rms(x) / R.rms(pool[0])) < 1e-12
    assert np.array_equal(C.short_noises(x, [(1, 0, 100, 5, 3, 3, 0.0)], pool, 70.0)[0], x)
    both = C.short_noises(x, [(0, 0, 100, 50, 0, 0, 3.0), (0, 200, 100, 100, 0, 0, 3.0)], pool, 70.0)[0]
    one = C.short_noises(x, [(0, 0, 100, 50, 0, 0, 3.0)], pool, 70.0)[0]
    two = C.short_noises(x, [(0, 200, 100, 100, 0, 0, 3.0)], pool, 70.0)[0]
    assert np.allclose(both - x, (one - x) + (two - x), rtol=0, atol=1e-15)


def test_ref_chain_order():
    """Seven stages, the reference's Compose order; with the new members off the chain is tests/augment_ref.py's."""
    rng = np.random.default_rng(3)
    x, h, noise, pool = rng.standard_normal(3000), rng.standard_normal(40), rng.standard_normal(500), [rng.standard_normal(900)]
    kw = dict(ir=h, noise=noise, noise_start=7, noise_snr_db=10.0, gauss_snr_db=30.0, seed=5, offset=2, clip_pct=8)
    y, after = C.chain(x, 1, **kw)
    y0, after0 = R.chain(x, 1, **kw)
    assert np.array_equal(y, y0) and len(after) == 7 and np.array_equal(after[3], after0[2])
    cas = C.cascades()
    ev = [(0, 0, 900, 100, 10, 10, 3.0)]
    y, after = C.chain(x, 1, events=ev, event_pool=pool, eq_sos=cas["eq, seven sections"], bl_sos=cas["butterworth 3"], **kw)
    assert np.array_equal(after[1], after0[1]) and np.array_equal(after[2], C.short_noises(after[1], ev, pool, 70.0)[0])
    assert np.array_equal(after[3], R.gaussian(after[2], 30.0, 5, 2, 1))                    # the floor's rms: of its own input
    assert np.array_equal(after[4], C.sos_filter(after[3], cas["eq, seven sections"])) and np.array_equal(after[5], R.clipping(after[4], 8))
    assert np.array_equal(y, C.sos_filter(after[5], cas["butterworth 3"]))


# ----------------------------------------------------------------------------- the filter design
def test_filter_design_and_refusals():
    sr = 16000
    for kind, f0, q, db in (("peaking", 1000.0, 1.0, 4.0), ("peaking", 20.0, 5.0, -4.0), ("low_shelf", 42.0, 0.1, 4.0), ("high_shelf", 7200.0, 0.9, -4.0)):
        s = augmentation.rbj_section(kind, f0, q, db, sr)
        w, hresp = scipy.signal.sosfreqz(_to_scipy(s[None]), worN=[1e-3, f0, 7999.0], fs=sr)
        at = {"peaking": 1, "low_shelf": 0, "high_shelf": 2}[kind]
        assert abs(20 * np.log10(abs(hresp[at])) - db) < 0.05, (kind, f0)                   # the asked gain, where the band has it
    lp3 = augmentation.lowpass_sos(3000.0, 3, sr)
    assert lp3.shape == (2, 5) and (lp3[:, 2] == 0.0).sum() == 1 and (lp3[:, 4] == 0.0).sum() == 1   # order 3: a first-order pole and zero
    lp1 = augmentation.lowpass_sos(3000.0, 1, sr)
    assert lp1.shape == (1, 5) and lp1[0, 2] == 0.0 and lp1[0, 4] == 0.0                    # a first-order section: b2 = a2 = 0
    assert np.allclose(_to_scipy(lp3), scipy.signal.butter(3, 3000.0, fs=sr, output="sos"))
    bp = augmentation.bandpass_sos(2100.0, 1.8, 2, sr)
    assert np.allclose(_to_scipy(bp), scipy.signal.butter(2, [210.0, 3990.0], btype="bandpass", fs=sr, output="sos"))
    # above Nyquist, or poles not strictly inside the unit circle: ValueError
    for bad in (lambda: augmentation.rbj_section("high_shelf", 8500.0, 0.5, 4.0, sr), lambda: augmentation.rbj_section("peaking", 8000.0, 1.0, 4.0, sr),
                lambda: augmentation.lowpass_sos(8000.0, 2, sr), lambda: augmentation.bandpass_sos(5000.0, 1.9, 1, sr),
                lambda: augmentation.check_sos([[1, 0, 0, 0.0, 1.0]]), lambda: augmentation.check_sos([[1, 0, 0, -2.0, 1.0 - 1e-9]]),
                lambda: augmentation.check_sos([[1, 0, 0, 1.0, 0.0]]), lambda: augmentation.check_sos([[1, 0, 0, 0.5, np.nan]]),
                lambda: augmentation.check_sos(np.zeros((9, 5))),
                lambda: DeviceProductionAugment(bandlimit_prob=0.1, lowpass_max_cutoff=9000.0, device="cpu"),
                lambda: DeviceProductionAugment(bandlimit_prob=0.1, bandpass_max_center_freq=4200.0, device="cpu")):
        with pytest.raises(ValueError):
            bad()
    augmentation.check_sos([[1, 0, 0, -1.9, 0.95]])
    # the EQ's ranges reach 9486 Hz; every centre the plan can draw is clamped below Nyquist, so every drawn EQ is stable
    assert max(b[2] for b in augmentation.EQ_BANDS) > 8000.0 and augmentation.EQ_MAX_CENTER_FRACTION < 0.5
    p = DeviceProductionAugment(eq_prob=1.0, device="cpu", seed=11).plan([1000] * 200)
    for b in range(200):
        augmentation.check_sos(p.eq_sos[b, :7])


# ----------------------------------------------------------------------------- the plan
def _pools():
    rng = np.random.default_rng(0)
    return ([rng.standard_normal(m).astype(np.float32) for m in (5, 3000)], [rng.standard_normal(m).astype(np.float32) for m in (100, 40000)],
            [rng.standard_normal(m).astype(np.float32) for m in (2000, 30000)])


def _aug(**kw):
    rirs, noises, events = _pools()
    base = dict(rir_pool=rirs, noise_pool=noises, short_noises_pool=events, gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0,
                clipping_prob=0.1, short_noises_prob=0.5, eq_prob=0.5, bandlimit_prob=0.3, device="cpu", seed=7)
    base.update(kw)
    return DeviceProductionAugment(**base)


def test_plan_is_reproducible_and_advances():
    lens = [160000, 120000, 80000, 4000] * 8
    a, b = _aug(), _aug()
    p1, p2, q1 = a.plan(lens), a.plan(lens), b.plan(lens)
    assert isinstance(p1, ProductionAugmentPlan)
    for f in FIELDS:
        assert np.array_equal(getattr(p1, f), getattr(q1, f), equal_nan=True), f
    assert (p1.seed, p1.offset) == (q1.seed, q1.offset) == (7, 0) and p2.offset == 1
    assert any(not np.array_equal(getattr(p1, f), getattr(p2, f), equal_nan=True) for f in FIELDS[6:])
    # the same number of variates whatever is decided: after one plan each, objects that decided differently draw the same next variate
    c, d = _aug(short_noises_prob=0.0, eq_prob=0.0, bandlimit_prob=0.0), _aug(short_noises_prob=1.0, eq_prob=1.0, bandlimit_prob=1.0)
    c.plan(lens), d.plan(lens)
    assert c._rng.random() == d._rng.random()
    # the first four stages of a seed are DeviceWaveAugment's
    rirs, noises, _ = _pools()
    w = DeviceWaveAugment(rir_pool=rirs, noise_pool=noises, gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, clipping_prob=0.1, device="cpu",
                          seed=7).plan(lens)
    for f in FIELDS[:6]:
        assert np.array_equal(getattr(p1, f), getattr(w, f), equal_nan=True), f
    # ranges
    on = np.arange(MAX_EVENTS)[None, :] < p1.ev_count[:, None]
    assert (p1.ev_count > 0).any() and (p1.ev_count == 0).any() and p1.ev_count.max() <= MAX_EVENTS
    plen = np.array([2000, 30000])[p1.ev_pool[on]]
    assert (p1.ev_len[on] >= 1).all() and (p1.ev_off[on] >= 0).all() and (p1.ev_off[on] + p1.ev_len[on] <= plen).all()
    assert (p1.ev_t0[on] >= 0).all() and (p1.ev_t0[on] < np.repeat(np.asarray(lens)[:, None], MAX_EVENTS, 1)[on]).all()
    assert ((p1.ev_snr_db[on] >= -6.0) & (p1.ev_snr_db[on] <= 18.0)).all()
    assert ((p1.ev_fade_in[on] >= 0) & (p1.ev_fade_in[on] <= p1.ev_len[on])).all() and (p1.ev_fade_out[on] <= p1.ev_len[on]).all()
    assert (np.diff(p1.ev_t0, axis=1)[on[:, 1:]] > 0).all()                                   # events are listed in time order
    assert set(np.unique(p1.eq_nsec)) == {0, 7} and set(np.unique(p1.bl_nsec)) <= {0, 1, 2} and (p1.bl_nsec > 0).any()
    assert p1.eq_sos.dtype == np.float64 and p1.eq_sos.shape == (32, IIR_MAX_SECTIONS, 5) and p1.ev_off.dtype == np.int64
    for b_ in np.flatnonzero(p1.bl_nsec):
        augmentation.check_sos(p1.bl_sos[b_, : p1.bl_nsec[b_]])


def test_probabilities_zero_and_one_and_no_pool():
    lens = [20000] * 64
    off = _aug(short_noises_prob=0.0, eq_prob=0.0, bandlimit_prob=0.0).plan(lens)
    assert not off.ev_count.any() and not off.eq_nsec.any() and not off.bl_nsec.any() and off.stages() & ~15 == 0
    assert off.ev_stride() == 0 and off.max_event_len() == 0
    on = _aug(short_noises_prob=1.0, eq_prob=1.0, bandlimit_prob=1.0, rir_prob=1.0, prob=1.0, clipping_prob=1.0).plan(lens)
    assert (on.ev_count >= 1).all() and (on.eq_nsec == 7).all() and (on.bl_nsec >= 1).all() and on.stages() == 127
    both = {int(n) for n in on.bl_nsec}
    assert both == {1, 2}                                      # low-pass of order 2 (1 section), 3 and 4 (2), band-pass of 1 and 2 sections
    # a short-noise probability without a pool: a silent no-op, as in the reference
    rirs, noises, _ = _pools()
    none = DeviceProductionAugment(rir_pool=rirs, noise_pool=noises, short_noises_prob=1.0, device="cpu").plan(lens)
    assert not none.ev_count.any() and none.stages() & 16 == 0
    # the image: the base image first, then everything else, 8-byte aligned
    img, head = on.pack(), on.base().pack()
    assert np.array_equal(img[: len(head)], head)
    E = on.ev_stride()
    assert len(img) == (len(head) + 7) // 8 * 8 + 64 * (2 * 40 * 8 + E * (3 * 8 + 4 * 4) + 3 * 4)
    v = augmentation._unpack_chain(torch.from_numpy(img), 64, E)
    assert np.array_equal(v["eq_sos"].numpy().reshape(64, 8, 5), on.eq_sos) and np.array_equal(v["bl_nsec"].numpy(), on.bl_nsec)
    assert np.array_equal(v["ev_t0"].numpy().reshape(64, E), on.ev_t0[:, :E]) and np.array_equal(v["clip_pct"].numpy(), on.clip_pct)
    np.testing.assert_allclose(v["ev_amp"].numpy().reshape(64, E), 10.0 ** (-on.ev_snr_db[:, :E].astype(np.float64) / 20.0), rtol=1e-6)
    odd = _aug(short_noises_prob=1.0).plan([20000] * 3)                                        # 28 B is not a multiple of 8 for an odd batch
    augmentation._unpack_chain(torch.from_numpy(odd.pack()), 3, odd.ev_stride())


@pytest.mark.parametrize("name", ["short_noises_prob", "eq_prob", "bandlimit_prob"])
def test_base_class_still_refuses(name):
    with pytest.raises(NotImplementedError, match=name):
        DeviceWaveAugment(device="cpu", **{name: 0.1})
    assert getattr(DeviceProductionAugment(device="cpu", **{name: 0.1}), name) == 0.1
    assert issubclass(DeviceProductionAugment, DeviceWaveAugment)


# ----------------------------------------------------------------------------- the library boundary
def test_workspace_queries_run_without_a_gpu():
    L = _lib.lib()
    hdr = open(_lib.HEADER).read()
    assert f"#define TA_WAVE_MAX_EVENTS {MAX_EVENTS}" in hdr and MAX_EVENTS == 64
    assert f"#define TA_WAVE_IIR_MAX_SECTIONS {IIR_MAX_SECTIONS}" in hdr and IIR_MAX_SECTIONS == 8
    assert f"#define TA_WAVE_IIR_CHUNK {IIR_CHUNK}" in hdr and IIR_CHUNK % 32 == 0
    assert L.ta_version() == 4
    B, Ls = 32, 160000
    nck = -(-Ls // IIR_CHUNK)
    assert L.ta_wave_sos_ws_bytes(B, Ls, 0) == L.ta_wave_sos_ws_bytes(B, Ls, IIR_CHUNK) == B * (nck * 16 + 256) * 8 < 4e6
    assert L.ta_wave_sos_ws_bytes(B, Ls, Ls) == B * (16 + 256) * 8                               # one chunk per clip: the sequential form
    assert L.ta_wave_sos_ws_bytes(0, Ls, 0) == 0 and L.ta_wave_sos_ws_bytes(B, Ls, 100) == 0      # (not a multiple of 32: refused)
    assert L.ta_wave_events_scratch_floats(B, Ls, 64, 64000) == B * 40 + B * 64 * 16
    assert L.ta_wave_events_scratch_floats(1, 4097, 3, 1) == 2 + 3 and L.ta_wave_events_scratch_floats(B, Ls, 0, 100) == 0


def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "wave_augment_chain" in torch_ops.OPERATORS and "wave_augment" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.wave_augment_chain.default._schema)
    assert s.startswith("ta355::wave_augment_chain(Tensor wav, Tensor lens, Tensor desc, SymInt stages, SymInt seed, SymInt offset, "
                        "SymInt ev_stride, SymInt max_event_len, SymInt handle)")
    h = torch_ops.register_module(_aug())
    with FakeTensorMode():
        out = torch.ops.ta355.wave_augment_chain(torch.empty(3, 5000), torch.empty(3, dtype=torch.int64), torch.empty(4000, dtype=torch.uint8),
                                                 127, 1, 2, 4, 1000, h)
        assert out.shape == (3, 5000) and out.dtype == torch.float32


BASE_CALLS = ["ta_wave_conv_f32", "ta_wave_mix_f32", "ta_wave_clip_f32"]


def test_apply_plumbing(dry):
    every = dict(rir_prob=1.0, prob=1.0, clipping_prob=1.0)
    aug = _aug(short_noises_prob=1.0, eq_prob=1.0, bandlimit_prob=1.0, **every)
    wav, lens = torch.zeros(4, 5000), torch.tensor([5000, 4000, 1, 300])
    dry.calls.clear()
    out = aug.apply(wav, lens, aug.plan(lens))
    assert out.shape == wav.shape and out.dtype == torch.float32 and out.data_ptr() != wav.data_ptr()
    # events exist: the mix runs twice (background only, then the Gaussian floor on its own input); EQ before, band-limit after the clipping
    assert dry.calls == ["ta_wave_fft_twiddles", "ta_wave_ir_spectra", "ta_wave_conv_f32", "ta_wave_mix_f32", "ta_wave_events_f32",
                         "ta_wave_mix_f32", "ta_wave_sos_f32", "ta_wave_clip_f32", "ta_wave_sos_f32"]
    # no clip has events: one mix call, as today
    quiet = _aug(short_noises_prob=0.0, eq_prob=1.0, bandlimit_prob=1.0, **every)
    quiet.apply(wav, lens, quiet.plan(lens))
    dry.calls.clear()
    quiet.apply(wav, lens, quiet.plan(lens))
    assert dry.calls == ["ta_wave_conv_f32", "ta_wave_mix_f32", "ta_wave_sos_f32", "ta_wave_clip_f32", "ta_wave_sos_f32"]
    # the new stages off: exactly the calls DeviceWaveAugment makes for the same plan fields
    off = _aug(short_noises_prob=0.0, eq_prob=0.0, bandlimit_prob=0.0, **every)
    p = off.plan(lens)
    off.apply(wav, lens, p)
    dry.calls.clear()
    off.apply(wav, lens, p)
    assert dry.calls == BASE_CALLS
    rirs, noises, _ = _pools()
    base = DeviceWaveAugment(rir_pool=rirs, noise_pool=noises, gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, device="cpu", seed=7, **every)
    base.apply(wav, lens, p.base())
    dry.calls.clear()
    base.apply(wav, lens, p.base())
    assert dry.calls == BASE_CALLS
    # refusals of a plan that does not fit
    p = aug.plan(lens)
    p.ev_pool[0, 0] = 2
    with pytest.raises(ValueError, match="pool"):
        aug.apply(wav, lens, p)
    p = aug.plan(lens)
    p.ev_off[0, 0] = 30000
    with pytest.raises(ValueError, match="inside its pool clip"):
        aug.apply(wav, lens, p)
    p = aug.plan(lens)
    p.eq_sos[1, 0] = [1.0, 0.0, 0.0, 0.0, 1.0]
    with pytest.raises(ValueError, match="unit circle"):
        aug.apply(wav, lens, p)
    with pytest.raises(ValueError, match="entries"):
        aug.apply(wav[:3], lens[:3], aug.plan(lens))


def test_feature_extractor_and_collator_take_it_without_change(dry):
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    from tiny_audio_amd.collator import DataCollator
    from tests.test_packing_host import ToyTokenizer, _Proj, _clips
    fe = LogMelFeatureExtractor(128, "cpu")
    clips = [np.zeros(1600, np.float32), np.zeros(800, np.float32)]
    aug = _aug(short_noises_prob=1.0, eq_prob=1.0, bandlimit_prob=1.0)
    fe(clips, sampling_rate=16000, augment=aug)
    dry.calls.clear()
    fe(clips, sampling_rate=16000, augment=aug)
    assert dry.calls.count("ta_wave_sos_f32") == 2 and "ta_wave_events_f32" in dry.calls
    assert max(i for i, c in enumerate(dry.calls) if c.startswith("ta_wave_")) < dry.calls.index("ta_logmel_f32")
    seen = []

    def spy(arrays, **kw):
        seen.append(kw)
        T = [len(a) // 160 for a in arrays]
        att = torch.zeros((len(arrays), max(T)), dtype=torch.int64)
        for i, t in enumerate(T):
            att[i, :t] = 1
        return {"input_features": torch.zeros((len(arrays), 8, max(T))), "attention_mask": att}

    DataCollator(ToyTokenizer(), spy, 16000, projector=_Proj(), augment=aug)(_clips([1.0, 0.5]))
    assert seen[0]["augment"] is aug

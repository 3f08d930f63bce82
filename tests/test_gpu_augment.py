"""Device-side waveform augmentation on the GPU (tiny_audio_amd/csrc/augment.hip) against the float64 definition in
tests/augment_ref.py.  Shapes are the smallest at which each kernel can still go wrong: for the convolution one block, an exact block
edge, both sides of the direct-form threshold, a response longer than one partition and a response longer than the clip; for the mix one sample, less than a wave, a noise
window that wraps and a silent one; for the clipping 1-3 samples, heavy ties and an all-zero clip.

Measured on MI355X (profiles/wave_augment.md): the figures each test prints before it asserts.
"""
import numpy as np
import pytest
import scipy.signal
import torch

from tests import augment_ref as R
from tiny_audio_amd.augmentation import CONV_DIRECT, CONV_HOP, DeviceWaveAugment, WaveAugmentPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = CONV_HOP


def _plan(B, **kw):
    p = WaveAugmentPlan(ir_idx=np.full(B, -1, np.int32), noise_idx=np.full(B, -1, np.int32), noise_start=np.zeros(B, np.int64),
                        noise_snr_db=np.full(B, np.nan, np.float32), gauss_snr_db=np.full(B, np.nan, np.float32),
                        clip_pct=np.zeros(B, np.int32), seed=0, offset=0)
    for k, v in kw.items():
        setattr(p, k, np.asarray(v, dtype=getattr(p, k).dtype) if isinstance(getattr(p, k), np.ndarray) else v)
    return p


def _batch(clips):
    lens = np.array([len(c) for c in clips], dtype=np.int64)
    host = np.zeros((len(clips), int(lens.max())), dtype=np.float32)
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return host, lens


def _run(aug, host, lens, plan):
    out = aug.apply(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), plan)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _wave(rng, n, tau=None):
    return (rng.standard_normal(n) * np.exp(-np.arange(n) / (tau or max(n / 3.0, 1.0)))).astype(np.float32)


# ----------------------------------------------------------------------------- convolution
NS = (1, H - 1, H, H + 1, 3 * H + 17)
MS = (1, 2, H, H + 1, 2 * H + 5)


@pytest.fixture(scope="module")
def conv_case():
    """Every (n, m) pair once plus two clips without a response; the float64 results and the f32 fftconvolve's own error, once."""
    rng = np.random.default_rng(20240)
    irs = [np.ones(1, np.float32)] + [_wave(rng, m, m / 4.0) for m in MS[1:]]
    clips, ir_idx = [], []
    for n in NS:
        for r in range(len(MS)):
            clips.append(_wave(rng, n)); ir_idx.append(r)
    clips += [_wave(rng, 3 * H + 17), _wave(rng, 100)]
    ir_idx += [-1, -1]
    host, lens = _batch(clips)
    ref = []
    for x, r in zip(clips, ir_idx):
        if r < 0:
            ref.append(None)
            continue
        h = irs[r]
        full32 = scipy.signal.fftconvolve(x, h)
        assert full32.dtype == np.float32
        out = {}
        for peak in (0.5, None):
            y64 = R.rir(x, h, peak)
            p32 = np.abs(full32).max()                        # the same peak scaling, in the f32 the transform ran in
            y32 = full32 * (np.float32(peak) / p32) if peak is not None and p32 > 0 else full32
            assert y32.dtype == np.float32
            out[peak] = (y64, float(np.abs(y32[: len(x)].astype(np.float64) - y64).max()))
        ref.append(out)
    return dict(irs=irs, clips=clips, ir_idx=np.array(ir_idx, np.int32), host=host, lens=lens, ref=ref)


@pytest.mark.parametrize("peak", [0.5, None])
def test_convolution_grid(conv_case, peak):
    """Gate of every clip: max |y - y64| <= 4 x the error of scipy.signal.fftconvolve on the float32 inputs (same peak scaling).

    Where one of the two inputs has ONE sample scipy.signal.fftconvolve runs no transform: it drops every axis on which an input has
    length 1 and returns the plain product, so its error there is a single rounding (exactly 0 for h = [1.0] without scaling).  The
    library meets that through its direct form (min(n, m) <= CONV_DIRECT: sums in double, rounded once); the other 16 pairs go
    through the 4096-point transforms.  Measured ratios: profiles/wave_augment.md."""
    c = conv_case
    aug = DeviceWaveAugment(rir_pool=c["irs"], rir_peak=peak, device=DEV)
    out = _run(aug, c["host"], c["lens"], _plan(len(c["clips"]), ir_idx=c["ir_idx"]))
    worst = (0.0, None)
    bad = []
    for b, (x, r) in enumerate(zip(c["clips"], c["ir_idx"])):
        n = len(x)
        assert not out[b, n:].any(), f"clip {b}: padding not zero"
        if r < 0:
            assert np.array_equal(out[b, :n].view(np.uint32), x.view(np.uint32)), f"clip {b}: ir_idx = -1 must be the input, bit for bit"
            continue
        y64, e32 = c["ref"][b][peak]
        err = float(np.abs(out[b, :n].astype(np.float64) - y64).max())
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else np.inf)
        print(f"conv peak={peak} n={n} m={len(c['irs'][r])}: err {err:.3e}  f32 fftconvolve err {e32:.3e}  ratio {ratio:.2f}")
        if ratio > worst[0]:
            worst = (ratio, (n, len(c["irs"][r])))
        if not err <= 4.0 * e32:
            bad.append((n, len(c["irs"][r]), err, e32))
        if peak is None and r == 0:                          # h = [1.0]: the reference IS the input, so the gate above says out = in
            assert np.array_equal(y64, x.astype(np.float64))
    print(f"conv peak={peak}: largest ratio {worst[0]:.2f} at (n, m) = {worst[1]}")
    assert not bad, bad


def test_convolution_direct_threshold():
    """Both sides of CONV_DIRECT, for the clip and for the response, under the gate of the grid: at 32 samples the direct form runs, at
    33 the transforms.  The partner has H + 1 and 3 H + 17 samples, so the direct form also crosses a block edge and leaves its peak
    in a later block than the kept samples."""
    rng = np.random.default_rng(4242)
    D = CONV_DIRECT
    pairs = [(D, H + 1), (D + 1, H + 1), (3 * H + 17, D), (3 * H + 17, D + 1), (D, D)]
    irs = [_wave(rng, m, m / 4.0) for _, m in pairs]
    clips = [_wave(rng, n) for n, _ in pairs]
    host, lens = _batch(clips)
    for peak in (0.5, None):
        out = _run(DeviceWaveAugment(rir_pool=irs, rir_peak=peak, device=DEV), host, lens, _plan(len(clips), ir_idx=np.arange(len(pairs))))
        for b, (x, h) in enumerate(zip(clips, irs)):
            n = len(x)
            full32 = scipy.signal.fftconvolve(x, h)
            y32 = full32 * (np.float32(peak) / np.abs(full32).max()) if peak is not None else full32
            assert y32.dtype == np.float32
            y64 = R.rir(x, h, peak)
            e32 = float(np.abs(y32[:n].astype(np.float64) - y64).max())
            err = float(np.abs(out[b, :n].astype(np.float64) - y64).max())
            print(f"conv threshold peak={peak} n={n} m={len(h)}: err {err:.3e}  f32 fftconvolve err {e32:.3e}  ratio {err / e32:.2f}")
            assert err <= 4.0 * e32 and not out[b, n:].any()


def test_convolution_peak_lies_in_the_discarded_tail():
    """m > n with a response that RISES towards its end: the maximum of the full convolution sits beyond the clip, so the kept samples
    only come out right when the peak was taken over the tail blocks too.  The peak the device scaled to, recovered from its largest
    kept sample, equals rir_peak within the convolution gate (4 x the f32 fftconvolve's own error, carried to the peak)."""
    rng = np.random.default_rng(77)
    n, m = H - 1, 2 * H + 5
    x, h = _wave(rng, n), _wave(rng, m, m / 4.0)[::-1].copy()
    raw = np.convolve(x.astype(np.float64), h.astype(np.float64))
    t_peak, P = int(np.abs(raw).argmax()), float(np.abs(raw).max())
    assert t_peak >= n and np.abs(raw[:n]).max() < 0.5 * P                       # the peak lies in the tail, clearly
    full32 = scipy.signal.fftconvolve(x, h)
    y32 = full32 * (np.float32(0.5) / np.abs(full32).max())
    y64 = R.rir(x, h, 0.5)
    e32 = float(np.abs(y32[:n].astype(np.float64) - y64).max())
    host, lens = _batch([x])
    out = _run(DeviceWaveAugment(rir_pool=[h], rir_peak=0.5, device=DEV), host, lens, _plan(1, ir_idx=[0]))
    err = float(np.abs(out[0, :n].astype(np.float64) - y64).max())
    t = int(np.abs(raw[:n]).argmax())
    used = float(out[0, t]) / raw[t] * P                                         # the peak value the device scaled to
    gate = 4.0 * e32 * P / abs(raw[t])
    print(f"tail peak n={n} m={m}: full peak at t={t_peak}; kept err {err:.3e} (f32 fftconvolve {e32:.3e}); device scaled the peak to "
          f"{used:.9f} (gate {gate:.2e})")
    assert err <= 4.0 * e32 and abs(used - 0.5) <= gate


# ----------------------------------------------------------------------------- mix
@pytest.fixture(scope="module")
def mix_case():
    rng = np.random.default_rng(7)
    clips = [_wave(rng, n, 1e9) * 0.1 for n in (1, 255, 16000, 16001)]
    noises = [rng.standard_normal(100).astype(np.float32), rng.standard_normal(40000).astype(np.float32) * 0.3, np.zeros(50, np.float32)]
    host, lens = _batch(clips)
    return dict(clips=clips, noises=noises, host=host, lens=lens)


def test_background_noise(mix_case):
    c = mix_case
    aug = DeviceWaveAugment(noise_pool=c["noises"], device=DEV)
    for idx, start, snr in (([0, 0, 1, 2], [99, 93, 39000, 7], [5.0, 30.0, 12.0, 10.0]),
                            ([1, 1, 0, 1], [39999, 39990, 50, 30000], [17.5, 8.0, 20.0, 6.0])):
        out = _run(aug, c["host"], c["lens"], _plan(4, noise_idx=idx, noise_start=start, noise_snr_db=snr))
        for b, x in enumerate(c["clips"]):
            n = len(x)
            assert not out[b, n:].any()
            noise = c["noises"][idx[b]]
            g = R.background_gain(x, noise, start[b], snr[b])
            if g == 0.0:                                      # the silent noise clip: the stage is skipped, bit for bit
                assert idx[b] == 2 and np.array_equal(out[b, :n].view(np.uint32), x.view(np.uint32))
                continue
            y64 = R.background(x, noise, start[b], snr[b])
            bound = 1e-5 * (np.abs(x.astype(np.float64)) + np.abs(g * R.noise_window(noise, start[b], n)))
            err = np.abs(out[b, :n].astype(np.float64) - y64)
            print(f"background n={n} noise={idx[b]} start={start[b]}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all()
            if n == 16000:
                d = out[b, :n].astype(np.float64) - x
                got = 10 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum(d * d))
                print(f"background n=16000: asked {snr[b]} dB, achieved {got:.4f} dB")
                assert abs(got - snr[b]) <= 0.25


def test_gaussian_floor(mix_case):
    c = mix_case
    aug = DeviceWaveAugment(gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, device=DEV)
    snr = [20.0, 40.0, 25.0, 33.0]
    seed, offset = 0x5DEECE66D1234, (1 << 32) + 5
    run = lambda off: _run(aug, c["host"], c["lens"], _plan(4, gauss_snr_db=snr, seed=seed, offset=off))
    out = run(offset)
    for b, x in enumerate(c["clips"]):
        n = len(x)
        assert not out[b, n:].any()
        z = R.normals(seed, offset, b, n)
        sigma = R.gaussian_sigma(x, snr[b])
        y64 = x.astype(np.float64) + sigma * z
        bound = 1e-5 * sigma * np.maximum(1.0, np.abs(z)) + 1e-5 * np.abs(x.astype(np.float64))
        err = np.abs(out[b, :n].astype(np.float64) - y64)
        print(f"gaussian n={n}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        if n == 16000:
            d = out[b, :n].astype(np.float64) - x
            got = 10 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum(d * d))
            print(f"gaussian n=16000: asked {snr[b]} dB, achieved {got:.4f} dB")
            assert abs(got - snr[b]) <= 0.25
    assert np.array_equal(run(offset).view(np.uint32), out.view(np.uint32))          # same (seed, offset): the same bits
    assert not np.array_equal(run(offset + 1), out)                                  # the next offset: other draws


# ----------------------------------------------------------------------------- clipping
def test_clipping():
    rng = np.random.default_rng(11)
    base = [_wave(rng, n, 1e9) for n in (1, 2, 3, 1001)]
    base.append((np.round(_wave(rng, 16000, 1e9) * 0.1 * 32768.0) / 32768.0).astype(np.float32))       # the 16-bit PCM grid: heavy ties
    base.append(np.zeros(500, np.float32))
    clips, pct = [], []
    for p in (1, 2, 9, 10):
        clips += base; pct += [p] * len(base)
    host, lens = _batch(clips)
    aug = DeviceWaveAugment(clipping_prob=1.0, device=DEV)
    out = _run(aug, host, lens, _plan(len(clips), clip_pct=pct))
    for b, (x, p) in enumerate(zip(clips, pct)):
        n = len(x)
        assert not out[b, n:].any()
        lo, hi = R.clip_thresholds(x, p)
        y64 = R.clipping(x, p)
        if p // 2 == 0:
            assert np.array_equal(out[b, :n].view(np.uint32), x.view(np.uint32))                       # q = 0: minimum and maximum
        ulp = max(float(np.spacing(np.float32(abs(lo)))), float(np.spacing(np.float32(abs(hi)))))
        err = np.abs(out[b, :n].astype(np.float64) - y64)
        assert (err <= 4 * ulp).all(), (n, p, float(err.max()), ulp)
        inside = (x > lo) & (x < hi)
        assert np.array_equal(out[b, :n][inside].view(np.uint32), x[inside].view(np.uint32))
        if n == 16000:
            print(f"clipping n=16000 pct={p}: thresholds {lo:.8f} {hi:.8f}, {int((~inside).sum())} samples at or beyond, max err {float(err.max()):.2e}")
            assert p // 2 == 0 or (~inside).sum() > 100


# ----------------------------------------------------------------------------- chain and boundary
@pytest.fixture(scope="module")
def chain_case():
    rng = np.random.default_rng(5)
    clips = [_wave(rng, n) for n in (1001, H + 5, 2 * H + 100)]
    irs = [_wave(rng, 300, 60.0), _wave(rng, H + 1, 500.0)]
    noises = [rng.standard_normal(100).astype(np.float32), rng.standard_normal(40000).astype(np.float32)]
    plan = _plan(3, ir_idx=[1, 0, 1], noise_idx=[0, 1, 1], noise_start=[93, 39000, 5], noise_snr_db=[10.0, 20.0, 5.0],
                 gauss_snr_db=[25.0, 40.0, 20.0], clip_pct=[10, 4, 0], seed=99, offset=3)
    host, lens = _batch(clips)
    return dict(clips=clips, irs=irs, noises=noises, plan=plan, host=host, lens=lens)


def _chain_aug(c):
    return DeviceWaveAugment(rir_pool=c["irs"], noise_pool=c["noises"], gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0,
                             clipping_prob=0.1, device=DEV)


def test_full_chain_matches_the_reference_stage_by_stage(chain_case):
    c, p = chain_case, chain_case["plan"]
    out = _run(_chain_aug(c), c["host"], c["lens"], p)
    for b, x in enumerate(c["clips"]):
        n = len(x)
        h, noise = c["irs"][p.ir_idx[b]], c["noises"][p.noise_idx[b]]
        y64, (a_rir, a_bg, a_gauss, _) = R.chain(x, b, ir=h, noise=noise, noise_start=p.noise_start[b], noise_snr_db=p.noise_snr_db[b],
                                                  gauss_snr_db=p.gauss_snr_db[b], seed=p.seed, offset=p.offset, clip_pct=p.clip_pct[b])
        # the stage gates, each on the reference's own intermediate
        full32 = scipy.signal.fftconvolve(x, h).astype(np.float64)
        g_rir = 4.0 * float(np.abs(full32[:n] * (0.5 / np.abs(full32).max()) - a_rir).max())
        g = R.background_gain(a_rir, noise, p.noise_start[b], p.noise_snr_db[b])
        g_bg = 1e-5 * (np.abs(a_rir) + np.abs(g * R.noise_window(noise, p.noise_start[b], n)))
        sigma, z = R.gaussian_sigma(a_bg, p.gauss_snr_db[b]), R.normals(p.seed, p.offset, b, n)
        g_gauss = 1e-5 * sigma * np.maximum(1.0, np.abs(z)) + 1e-5 * np.abs(a_bg)
        g_clip = 0.0
        if p.clip_pct[b]:
            lo, hi = R.clip_thresholds(a_gauss, p.clip_pct[b])
            g_clip = 4 * max(float(np.spacing(np.float32(abs(lo)))), float(np.spacing(np.float32(abs(hi)))))
        bound = g_rir + g_bg + g_gauss + g_clip
        err = np.abs(out[b, :n].astype(np.float64) - y64)
        print(f"chain n={n}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all() and not out[b, n:].any()


def test_feature_extractor_boundary(chain_case):
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    c = chain_case
    aug = _chain_aug(c)
    fe = LogMelFeatureExtractor(128, DEV)
    clips = [np.concatenate([x, np.zeros(160, np.float32)]) for x in c["clips"]]
    host, lens = _batch(clips)
    got = fe(clips, sampling_rate=16000, augment=aug, augment_plan=c["plan"])
    wav = aug.apply(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), c["plan"])
    feats, mask = fe.extract(wav, torch.from_numpy(lens).to(DEV))
    assert torch.equal(got["input_features"], feats) and torch.equal(got["attention_mask"], mask)
    plain, none = fe(clips, sampling_rate=16000), fe(clips, sampling_rate=16000, augment=None)
    assert torch.equal(plain["input_features"], none["input_features"]) and torch.equal(plain["attention_mask"], none["attention_mask"])
    assert not torch.equal(plain["input_features"], feats)                            # (and the augmentation did something)
    drawn = fe(clips, sampling_rate=16000, augment=aug)                               # without a plan one is drawn
    assert drawn["input_features"].shape == feats.shape and bool(torch.isfinite(drawn["input_features"]).all())

"""The whole production chain on the GPU (``DeviceProductionAugment``, tiny_audio_amd/csrc/augment.hip) against the float64 definition in
tests/augment_chain_ref.py.  Shapes are the smallest at which each kernel can still go wrong: for the cascade one and two samples, both
sides of a chunk edge, several chunks and more than one workgroup of 64 chunks (40 T + 3 is not enough for that: the last grid test
adds 70 T + 5), every section count with a different code path; for the events every edge of the issue's list.

Measured on MI355X (profiles/wave_augment.md): the figures each test prints before it asserts.
"""
import numpy as np
import pytest
import scipy.signal
import torch

from tests import augment_chain_ref as C
from tests import augment_ref as R
from tiny_audio_amd.augmentation import (CONV_HOP, IIR_CHUNK, IIR_MAX_SECTIONS, MAX_EVENTS, DeviceProductionAugment, DeviceWaveAugment,
                                         ProductionAugmentPlan)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = IIR_CHUNK
H = CONV_HOP
LD = np.longdouble


def _plan(B, **kw):
    E = MAX_EVENTS
    p = ProductionAugmentPlan(ir_idx=np.full(B, -1, np.int32), noise_idx=np.full(B, -1, np.int32), noise_start=np.zeros(B, np.int64),
                              noise_snr_db=np.full(B, np.nan, np.float32), gauss_snr_db=np.full(B, np.nan, np.float32),
                              clip_pct=np.zeros(B, np.int32), seed=0, offset=0, ev_count=np.zeros(B, np.int32),
                              ev_pool=np.zeros((B, E), np.int32), ev_off=np.zeros((B, E), np.int64), ev_len=np.ones((B, E), np.int64),
                              ev_t0=np.zeros((B, E), np.int64), ev_fade_in=np.zeros((B, E), np.int32), ev_fade_out=np.zeros((B, E), np.int32),
                              ev_snr_db=np.zeros((B, E), np.float32), eq_nsec=np.zeros(B, np.int32),
                              eq_sos=np.zeros((B, IIR_MAX_SECTIONS, 5)), bl_nsec=np.zeros(B, np.int32), bl_sos=np.zeros((B, IIR_MAX_SECTIONS, 5)))
    for k, v in kw.items():
        setattr(p, k, np.asarray(v, dtype=getattr(p, k).dtype) if isinstance(getattr(p, k), np.ndarray) else v)
    return p


def _set_events(p, b, events):
    """events: the reference's tuples (j, o, length, t0, f_in, f_out, snr_db) of clip b."""
    p.ev_count[b] = len(events)
    for k, (j, o, length, t0, f_in, f_out, snr) in enumerate(events):
        p.ev_pool[b, k], p.ev_off[b, k], p.ev_len[b, k], p.ev_t0[b, k] = j, o, length, t0
        p.ev_fade_in[b, k], p.ev_fade_out[b, k], p.ev_snr_db[b, k] = f_in, f_out, snr


def _set_sos(p, which, b, sos):
    getattr(p, which + "_nsec")[b] = len(sos)
    getattr(p, which + "_sos")[b, : len(sos)] = sos


def _batch(clips, pad=7):
    lens = np.array([len(c) for c in clips], dtype=np.int64)
    host = np.zeros((len(clips), int(lens.max()) + pad), dtype=np.float32)          # Ls > max n
    for i, c in enumerate(clips):
        host[i, : len(c)] = c
    return host, lens


def _run(aug, host, lens, plan):
    out = aug.apply(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), plan)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _to_scipy(sos):
    return np.ascontiguousarray(np.concatenate([sos[:, :3], np.ones((len(sos), 1)), sos[:, 3:]], axis=1))


def _half_ulp(y):
    return 0.5 * np.spacing(np.abs(np.asarray(y)).astype(np.float32)).astype(np.float64)


def _sos_gate(x, sos):
    """-> (the long-double result, the per-sample gate of an f32 result) for the float64 input x [n]: half an f32 ulp of the reference
    (the one permitted rounding) + 16 x the largest difference between scipy.signal.sosfilt in float64 and the long-double run of the
    same case (f64 rounding noise of this recurrence, measured; the factor allows for FMA contraction and the chunked association)."""
    y_ld = C.sos_run(x, sos, dtype=LD)[0]
    y64 = scipy.signal.sosfilt(_to_scipy(sos), np.asarray(x, np.float64))
    noise = float(np.abs(y64.astype(LD) - y_ld).max())
    return y_ld, _half_ulp(y_ld) + 16.0 * noise, noise


# ----------------------------------------------------------------------------- the cascade
NS = (1, 2, T - 1, T, T + 1, 3 * T + 17, 40 * T + 3)
INPUTS = ("noise", "impulse at 0", "impulse at T - 1", "dc")


@pytest.fixture(scope="module")
def sos_case():
    """The four inputs at the longest n (a causal filter's shorter cases are prefixes) and, per cascade, the long-double and float64
    results of all four at once."""
    n = max(NS)
    x = np.zeros((4, n), np.float32)
    x[0] = np.random.default_rng(31).standard_normal(n) * 0.1
    x[1, 0] = 1.0
    x[2, T - 1] = 1.0
    x[3] = 0.25
    cas = C.cascades()
    ref = {}
    for name, sos in cas.items():
        y_ld = C.sos_run(x, sos, dtype=LD)[0]
        y64 = np.stack([scipy.signal.sosfilt(_to_scipy(sos), x[i].astype(np.float64)) for i in range(4)])
        ref[name] = (y_ld, y64)
    assert np.finfo(LD).nmant >= 63
    return dict(x=x, cas=cas, ref=ref)


@pytest.mark.parametrize("kind", range(4), ids=INPUTS)
def test_sos_grid(sos_case, kind):
    """Every (cascade, n) pair once, n and the section count mixed inside each batch (B = 4), through the EQ's slot in half of the
    batches and the band-limit's in the other half; one clip of every second batch has no cascade and must come back bit for bit.
    Gate per sample: |err| <= 1/2 ulp_f32(y_ref) + 16 max|y_f64 - y_longdouble|."""
    c = sos_case
    names = list(c["cas"])
    aug = DeviceProductionAugment(eq_prob=1.0, bandlimit_prob=1.0, device=DEV)
    x = c["x"][kind]
    worst, bad = (0.0, None), []
    for r in range(len(NS)):
        for which, group in (("eq", range(0, 4)), ("bl", range(4, 7))):
            pairs = [(names[i], NS[(i + r) % len(NS)]) for i in group]
            clips = [x[:n] for _, n in pairs]
            if which == "bl":
                clips.append(x[: NS[r]] + np.float32(0.5))                 # no cascade: untouched
            host, lens = _batch(clips)
            p = _plan(len(clips))
            for b, (name, _) in enumerate(pairs):
                _set_sos(p, which, b, c["cas"][name])
            out = _run(aug, host, lens, p)
            for b, clip in enumerate(clips):
                assert not out[b, len(clip):].any(), f"clip {b}: padding not zero"
            if which == "bl":
                assert np.array_equal(out[-1, : NS[r]].view(np.uint32), clips[-1].view(np.uint32)), "n_sec = 0 must leave the clip bit-identical"
            for b, (name, n) in enumerate(pairs):
                y_ld, y64 = c["ref"][name][0][kind, :n], c["ref"][name][1][kind, :n]
                noise = float(np.abs(y64.astype(LD) - y_ld).max())
                bound = _half_ulp(y_ld) + 16.0 * noise
                err = np.abs(out[b, :n].astype(LD) - y_ld).astype(np.float64)
                ratio = float((err / bound).max())
                print(f"sos {INPUTS[kind]} / {name} / n={n}: max err {float(err.max()):.3e}, f64 noise {noise:.2e}, max err / bound {ratio:.3f}")
                if ratio > worst[0]:
                    worst = (ratio, (name, n))
                if not (err <= bound).all():
                    bad.append((name, n, ratio))
    print(f"sos {INPUTS[kind]}: largest err / bound {worst[0]:.3f} at {worst[1]}")
    assert not bad, bad


def test_sos_more_than_one_workgroup_of_chunks():
    """70 T + 5 samples: 71 chunks, so two workgroups of 64 chunks and a carry across their edge; the seven-section EQ and the slow
    20 Hz peak; under the gate of the grid."""
    cas = C.cascades()
    n = 70 * T + 5
    x = (np.random.default_rng(32).standard_normal(n) * 0.1).astype(np.float32)
    names = ("eq, seven sections", "20 Hz peak, Q 5")
    host, lens = _batch([x, x[: 64 * T], x[: 64 * T + 1]])
    p = _plan(3)
    _set_sos(p, "eq", 0, cas[names[0]]); _set_sos(p, "eq", 1, cas[names[1]]); _set_sos(p, "eq", 2, cas[names[1]])
    out = _run(DeviceProductionAugment(eq_prob=1.0, device=DEV), host, lens, p)
    for b, (name, m) in enumerate(((names[0], n), (names[1], 64 * T), (names[1], 64 * T + 1))):
        y_ld, bound, noise = _sos_gate(x[:m].astype(np.float64), cas[name])
        err = np.abs(out[b, :m].astype(LD) - y_ld).astype(np.float64)
        print(f"sos two workgroups / {name} / n={m}: max err {float(err.max()):.3e}, f64 noise {noise:.2e}, max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all() and not out[b, m:].any()


# ----------------------------------------------------------------------------- short noises
def test_short_noise_events():
    rng = np.random.default_rng(41)
    pool = [rng.standard_normal(5000).astype(np.float32) * 0.3, np.zeros(300, np.float32), rng.standard_normal(700).astype(np.float32)]
    ns = (10000, 9000, 4500, 1, 12000, 16000)
    clips = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in ns]
    events = [
        [(0, 0, 3000, 0, 100, 200, 5.0), (0, 3000, 2000, 8000, 50, 50, 0.0)],                  # starts at 0; ends exactly at n
        [(0, 100, 3000, 8000, 10, 500, 3.0), (2, 5, 1, 17, 0, 0, -6.0), (2, 0, 1, 18, 1, 1, 0.0),   # runs past n; length 1 (with and without fades)
         (0, 1000, 1000, 2000, 700, 800, 10.0)],                                               # fades longer than half the event
        [(0, 0, 600, 3800, 20, 20, 6.0), (2, 0, 700, 4000, 0, 300, 2.0), (1, 0, 300, 100, 5, 5, 0.0)],   # overlapping, across a chunk edge; silent
        [],                                                                                   # no events, one sample
        [(2, (7 * k) % 37, 600 + k, 150 * k, k, 2 * k, float(k % 9)) for k in range(MAX_EVENTS)],       # 64 events, heavily overlapping
        [(0, 0, 5000, 6000, 0, 0, 7.0)],                                                       # a single unfaded event (two rms chunks)
    ]
    host, lens = _batch(clips)
    p = _plan(len(clips))
    for b, ev in enumerate(events):
        _set_events(p, b, ev)
    D = 70.0
    aug = DeviceProductionAugment(short_noises_pool=pool, short_noises_prob=1.0, fade_floor_db=D, device=DEV)
    out = _run(aug, host, lens, p)
    for b, (x, ev) in enumerate(zip(clips, events)):
        n = len(x)
        assert not out[b, n:].any()
        if not ev:
            assert np.array_equal(out[b, :n].view(np.uint32), x.view(np.uint32))              # no events: bit-identical
            continue
        y64, mag, gains = C.short_noises(x, ev, pool, D)
        bound = 1e-5 * (np.abs(x.astype(np.float64)) + mag)
        err = np.abs(out[b, :n].astype(np.float64) - y64)
        print(f"events clip {b} ({len(ev)} events, n={n}): max err {float(err.max()):.3e}, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
        if b == 2:
            assert gains[2] == 0.0                                                             # the silent event was skipped
        if b == 5:
            d = out[b, 6000:11000].astype(np.float64) - x[6000:11000]
            got = 20 * np.log10(R.rms(x) / R.rms(d))
            print(f"events: a single unfaded event asked {ev[0][6]} dB, achieved {got:.4f} dB")
            assert abs(got - ev[0][6]) <= 0.01
    # another fade floor is another result: D is an argument of the kernel
    out40 = _run(DeviceProductionAugment(short_noises_pool=pool, short_noises_prob=1.0, fade_floor_db=40.0, device=DEV), host, lens, p)
    y40, mag40, _ = C.short_noises(clips[0], events[0], pool, 40.0)
    assert (np.abs(out40[0, : ns[0]].astype(np.float64) - y40) <= 1e-5 * (np.abs(clips[0].astype(np.float64)) + mag40)).all()
    assert not np.array_equal(out40[0], out[0])


# ----------------------------------------------------------------------------- chain and boundary
def _wave(rng, n, tau=None):
    return (rng.standard_normal(n) * np.exp(-np.arange(n) / (tau or max(n / 3.0, 1.0)))).astype(np.float32)


@pytest.fixture(scope="module")
def chain_case():
    rng = np.random.default_rng(5)
    clips = [_wave(rng, n) for n in (1001, H + 5, 2 * H + 100)]
    irs = [_wave(rng, 300, 60.0), _wave(rng, H + 1, 500.0)]
    noises = [rng.standard_normal(100).astype(np.float32), rng.standard_normal(40000).astype(np.float32)]
    pool = [rng.standard_normal(900).astype(np.float32), rng.standard_normal(3000).astype(np.float32)]
    cas = C.cascades()
    p = _plan(3, ir_idx=[1, 0, 1], noise_idx=[0, 1, 1], noise_start=[93, 39000, 5], noise_snr_db=[10.0, 20.0, 5.0],
              gauss_snr_db=[25.0, 40.0, 20.0], clip_pct=[10, 4, 0], seed=99, offset=3)
    events = [[(0, 0, 900, 50, 30, 60, 3.0), (1, 100, 500, 400, 0, 100, 0.0)], [(1, 0, 3000, 1000, 80, 160, 6.0)], []]
    eq = [cas["eq, seven sections"], cas["eight sections"], None]
    bl = [cas["butterworth 3"], None, cas["butterworth 4"]]
    for b in range(3):
        _set_events(p, b, events[b])
        if eq[b] is not None:
            _set_sos(p, "eq", b, eq[b])
        if bl[b] is not None:
            _set_sos(p, "bl", b, bl[b])
    host, lens = _batch(clips, pad=0)
    return dict(clips=clips, irs=irs, noises=noises, pool=pool, plan=p, events=events, eq=eq, bl=bl, host=host, lens=lens)


def _chain_aug(c, cls=DeviceProductionAugment, **kw):
    if cls is DeviceProductionAugment:
        kw = dict(short_noises_pool=c["pool"], short_noises_prob=0.5, eq_prob=0.5, bandlimit_prob=0.3, **kw)
    return cls(rir_pool=c["irs"], noise_pool=c["noises"], gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, clipping_prob=0.1, device=DEV, **kw)


def test_full_chain_matches_the_reference_stage_by_stage(chain_case):
    """All seven stages (clip 0; clip 1 without the band-limit, clip 2 without events, EQ and clipping).  The gate of each stage is the
    gate of its own test, taken on the reference's own intermediate; a gate is carried through a later cascade by that cascade's l1 gain
    (sum |h|, from its impulse response), through the clipping unchanged (Lipschitz constant 1)."""
    c, p = chain_case, chain_case["plan"]
    out = _run(_chain_aug(c), c["host"], c["lens"], p)
    for b, x in enumerate(c["clips"]):
        n = len(x)
        h, noise = c["irs"][p.ir_idx[b]], c["noises"][p.noise_idx[b]]
        y64, (a_rir, a_bg, a_ev, a_gauss, a_eq, a_clip, _) = C.chain(
            x, b, ir=h, noise=noise, noise_start=p.noise_start[b], noise_snr_db=p.noise_snr_db[b], events=c["events"][b], event_pool=c["pool"],
            fade_floor_db=70.0, gauss_snr_db=p.gauss_snr_db[b], seed=p.seed, offset=p.offset, eq_sos=c["eq"][b], clip_pct=p.clip_pct[b],
            bl_sos=c["bl"][b])
        full32 = scipy.signal.fftconvolve(x, h).astype(np.float64)
        g = 4.0 * float(np.abs(full32[:n] * (0.5 / np.abs(full32).max()) - a_rir).max())
        gb = R.background_gain(a_rir, noise, p.noise_start[b], p.noise_snr_db[b])
        g = g + 1e-5 * (np.abs(a_rir) + np.abs(gb * R.noise_window(noise, p.noise_start[b], n)))
        if c["events"][b]:
            g = g + 1e-5 * (np.abs(a_bg) + C.short_noises(a_bg, c["events"][b], c["pool"], 70.0)[1])
        sigma, z = R.gaussian_sigma(a_ev, p.gauss_snr_db[b]), R.normals(p.seed, p.offset, b, n)
        g = g + 1e-5 * sigma * np.maximum(1.0, np.abs(z)) + 1e-5 * np.abs(a_ev)
        if c["eq"][b] is not None:
            g = C.sos_l1_gain(c["eq"][b], n) * float(np.max(g)) + _sos_gate(a_gauss, c["eq"][b])[1]
        if p.clip_pct[b]:
            lo, hi = R.clip_thresholds(a_eq, p.clip_pct[b])
            g = g + 4 * max(float(np.spacing(np.float32(abs(lo)))), float(np.spacing(np.float32(abs(hi)))))
        if c["bl"][b] is not None:
            g = C.sos_l1_gain(c["bl"][b], n) * float(np.max(g)) + _sos_gate(a_clip, c["bl"][b])[1]
        err = np.abs(out[b, :n].astype(np.float64) - y64)
        print(f"chain n={n}: max err {float(err.max()):.3e}, max err / bound {float((err / g).max()):.3f}")
        assert (err <= g).all() and not out[b, n:].any()


def test_new_stages_off_is_the_base_class_byte_for_byte(chain_case):
    c = chain_case
    p = _plan(3)
    for f in ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct", "seed", "offset"):
        setattr(p, f, getattr(c["plan"], f))
    assert p.stages() == 15
    got = _run(_chain_aug(c), c["host"], c["lens"], p)
    want = _run(_chain_aug(c, DeviceWaveAugment), c["host"], c["lens"], p.base())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and a clip whose new stages are off, beside clips that use them, is the base class's clip: stages act per clip
    q = c["plan"]
    mixed = _plan(3)
    for f in ("ir_idx", "noise_idx", "noise_start", "noise_snr_db", "gauss_snr_db", "clip_pct", "seed", "offset"):
        setattr(mixed, f, getattr(q, f))
    _set_events(mixed, 0, c["events"][0]); _set_sos(mixed, "eq", 0, c["eq"][0]); _set_sos(mixed, "bl", 1, c["bl"][0])
    got = _run(_chain_aug(c), c["host"], c["lens"], mixed)
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1])


def test_feature_extractor_boundary(chain_case):
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    c = chain_case
    aug = _chain_aug(c)
    fe = LogMelFeatureExtractor(128, DEV)
    clips = [np.concatenate([x, np.zeros(160, np.float32)]) for x in c["clips"]]
    host, lens = _batch(clips, pad=0)
    got = fe(clips, sampling_rate=16000, augment=aug, augment_plan=c["plan"])
    wav = aug.apply(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), c["plan"])
    feats, mask = fe.extract(wav, torch.from_numpy(lens).to(DEV))
    assert torch.equal(got["input_features"], feats) and torch.equal(got["attention_mask"], mask)
    plain = fe(clips, sampling_rate=16000)
    assert not torch.equal(plain["input_features"], feats)                            # (and the augmentation did something)
    drawn = fe(clips, sampling_rate=16000, augment=aug)                               # without a plan one is drawn
    assert drawn["input_features"].shape == feats.shape and bool(torch.isfinite(drawn["input_features"]).all())

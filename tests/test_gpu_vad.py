"""-m gpu: the voice activity detector (csrc/vad.hip) against its float64 definition (tests/vad_ref.py), and through the diarizer and
``ASRModel.transcribe_long`` end to end.

Gates.  Statistic: |L_dev - L64| <= gate * (L64 + theta) per frame, where gate = max(4 * e32, 1e-4) and e32 = the largest
|L32 - L64| / (L64 + theta) of the float32 numpy restatement ON THE SAME INPUT (four times it: the device's FFT and sums run in another
order); gate < 0.02 is asserted, so the gate stays inside the decision band.  Decisions: the device's flags equal the float64 flags on
every frame outside the band |L64 - theta| <= 0.05 theta, and at most 2 % of a signal's frames lie inside it (tests/test_vad_ref.py
shows that for every signal used here).  Ragged batches, two runs, poisoned outputs: bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import vad_ref as R

DEV = "cuda"
THETA = R.DEFAULTS["theta"]
_REFS = {}


def _ref(key, x, **opt):
    """(L64, L32) of one input, computed once per module."""
    if key not in _REFS:
        _REFS[key] = (R.statistic(x, **opt), R.statistic(x, dtype=np.float32, **opt))
    return _REFS[key]


def _run(waves, h=2, W=94, beta=2.0, theta=THETA, e0=1e-12, **kw):
    from tiny_audio_amd import longform, ops
    flat, off, lens = longform.upload(waves)
    stat, flags, nf = ops.vad(flat, off, max(lens), h, W, beta, theta, e0, **kw)
    torch.cuda.synchronize()
    return stat.cpu().numpy(), flags.cpu().numpy(), nf.cpu().numpy()


def _check(name, L_dev, f_dev, L64, L32, theta=THETA):
    """The two gates of the module docstring on one recording -> (device error, e32), both relative to L64 + theta."""
    assert L_dev.shape == L64.shape and f_dev.shape == L64.shape, (name, L_dev.shape, L64.shape)
    if len(L64) == 0:
        return 0.0, 0.0
    scale = L64 + theta
    e32 = float(np.max(np.abs(L32 - L64) / scale))
    gate = max(4.0 * e32, 1e-4)
    assert gate < 0.02, (name, e32)
    err = np.abs(L_dev.astype(np.float64) - L64) / scale
    assert np.isfinite(L_dev).all() and (err <= gate).all(), (name, int(np.argmax(err)), float(err.max()), gate)
    band = R.in_band(L64, theta)
    assert band.sum() <= 0.02 * len(L64), (name, int(band.sum()))
    differ = (f_dev.astype(bool) != R.flags_of(L64, theta)) & ~band
    assert set(np.unique(f_dev).tolist()) <= {0, 1} and not differ.any(), (name, np.flatnonzero(differ)[:8])
    return float(err.max()), e32


@pytest.fixture(scope="module")
def signals():
    return R.gpu_signals()


# ============================================================================ (a) the statistic and the decisions
@pytest.mark.parametrize("name", ["white-20dB", "white-10dB", "pink-20dB", "pink-10dB"])
def test_statistic_and_decisions_against_float64(signals, name):
    x, truth, counted, _ = signals[name]
    L64, L32 = _ref(name, x)
    stat, flags, nf = _run([x])
    F = R.frames_of(len(x))
    assert nf.tolist() == [F] and stat.shape == (1, F)
    err, e32 = _check(name, stat[0], flags[0], L64, L32)
    f = flags[0].astype(bool)
    print(f"{name}: device error {err:.3g}, e32 {e32:.3g}, gate {max(4 * e32, 1e-4):.3g} (all relative to L64 + theta); "
          f"{int(R.in_band(L64).sum())} of {F} frames in the band; false alarms {int((f & ~truth & counted).sum())}, "
          f"misses {int((~f & truth & counted).sum())} away from boundaries")


# ============================================================================ (b) edges
def test_edge_lengths_in_two_batches():
    """n = 256, 257, 512, 513, 1000 (F = 0, 1, 1, 2, 3); recordings shorter than h and than W; F around 2 W, around the statistic
    kernel's tile and around the energy kernel's frames per workgroup -- every one against float64, as members of ragged batches."""
    from tiny_audio_amd import ops
    base = R.edge_base()
    lengths = [256, 257, 512, 513, 1000] + [R.samples_for_frames(F) for F in R.edge_frame_counts(ops.VAD_TILE, ops.VAD_ENERGY_FRAMES)]
    lengths += [R.samples_for_frames(ops.VAD_TILE, 256), R.samples_for_frames(ops.VAD_ENERGY_FRAMES, 256)]      # the longest n of a frame count
    assert [R.frames_of(n) for n in lengths[:5]] == [0, 1, 1, 2, 3]
    waves = [base[:n] for n in lengths]
    worst = 0.0
    for part in (waves[0::2], waves[1::2]):
        stat, flags, nf = _run(part)
        for r, x in enumerate(part):
            F = R.frames_of(len(x))
            assert nf[r] == F
            L64, L32 = _ref(("edge", len(x)), x)
            err, _ = _check(f"edge n={len(x)}", stat[r, :F], flags[r, :F], L64, L32)
            worst = max(worst, err)
            assert not stat[r, F:].any() and not flags[r, F:].any(), "positions beyond F were written"
    print(f"{len(waves)} edge lengths: worst device error {worst:.3g} of L64 + theta")


@pytest.mark.parametrize("W,h", [(1, 2), (31, 2), (1024, 2), (94, 0), (94, 8), (1024, 8)])
def test_option_edges(signals, W, h):
    x = signals["white-10dB"][0]
    L64, L32 = _ref(("opt", W, h), x, W=W, h=h)
    stat, flags, _ = _run([x], h=h, W=W)
    band = R.in_band(L64)
    if band.sum() > 0.02 * len(L64):
        pytest.fail(f"W={W} h={h}: {int(band.sum())} frames in the band: this input cannot show a wrong flag")
    err, e32 = _check(f"W={W} h={h}", stat[0], flags[0], L64, L32)
    print(f"W={W} h={h}: device error {err:.3g}, e32 {e32:.3g}")


def test_other_thresholds_biases_and_floors(signals):
    x = signals["pink-10dB"][0]
    for beta, theta, e0 in ((1.0, 0.5, 1e-12), (4.0, 0.05, 1e-9), (2.0, 0.15, 1e-6)):
        L64 = R.statistic(x, beta=beta, theta=theta, e0=e0)
        L32 = R.statistic(x, beta=beta, theta=theta, e0=e0, dtype=np.float32)
        stat, flags, _ = _run([x], beta=beta, theta=theta, e0=e0)
        scale = L64 + theta
        gate = max(4.0 * float(np.max(np.abs(L32 - L64) / scale)), 1e-4)
        assert gate < 0.02
        assert (np.abs(stat[0] - L64) <= gate * scale).all(), (beta, theta, e0)
        assert not ((flags[0].astype(bool) != R.flags_of(L64, theta)) & ~R.in_band(L64, theta)).any()


# ============================================================================ (c) batches, bits, what is not written
def _ragged(signals):
    base = R.edge_base()
    return [base[:513], signals["pink-10dB"][0], base[:200], base[:R.samples_for_frames(257)], base[:1000]]


def test_ragged_batch_equals_every_recording_alone_bit_for_bit(signals):
    waves = _ragged(signals)
    offsets = np.cumsum([0] + [len(w) for w in waves])
    assert (offsets[1:4] % 2 == 1).all() and (offsets[1:4] % 4 != 0).all(), "members start at odd samples: no 16-byte alignment"
    stat, flags, nf = _run(waves)
    stat2, flags2, nf2 = _run(waves)
    assert np.array_equal(stat.view(np.uint32), stat2.view(np.uint32)) and np.array_equal(flags, flags2) and np.array_equal(nf, nf2)
    assert nf.tolist() == [R.frames_of(len(w)) for w in waves] and nf[2] == 0
    assert stat.shape == (5, R.frames_of(240000))
    for r, w in enumerate(waves):
        a_stat, a_flags, a_nf = _run([w])
        F = int(nf[r])
        assert a_nf.tolist() == [F]
        assert np.array_equal(stat[r, :F].view(np.uint32), a_stat[0, :F].view(np.uint32)), r
        assert np.array_equal(flags[r, :F], a_flags[0, :F]), r
    assert flags[1].any() and not flags[1].all()


def test_a_silent_recording_between_loud_ones_stays_exactly_zero():
    rng = np.random.default_rng(11)
    loud = [(0.9 * rng.standard_normal(n)).astype(np.float32) for n in (4097, 5003)]
    stat, flags, nf = _run([loud[0], np.zeros(5001, np.float32), loud[1]])
    assert nf.tolist() == [16, 19, 19]
    assert (stat[1, :19] == 0).all() and not flags[1].any(), "a neighbour's samples leaked into a frame's window"
    assert (stat[0, :16] >= 0).all() and np.isfinite(stat).all()


def test_poisoned_outputs_keep_their_poison_beyond_F(signals):
    from tiny_audio_amd import ops
    waves = _ragged(signals)[2:] + [R.edge_base()[:R.samples_for_frames(64)]]
    maxF = max(R.frames_of(len(w)) for w in waves)
    ld = maxF + 3
    stat = torch.full((len(waves), ld), float("nan"), device=DEV)
    flags = torch.full((len(waves), ld), 0xFF, device=DEV, dtype=torch.uint8)
    s, f, nf = _run(waves, stat=stat, flags=flags)
    assert s.shape == (len(waves), ld)
    for r, w in enumerate(waves):
        F = R.frames_of(len(w))
        assert nf[r] == F and not np.isnan(s[r, :F]).any() and (f[r, :F] <= 1).all(), r
        assert np.isnan(s[r, F:]).all() and (f[r, F:] == 0xFF).all(), r
    with pytest.raises(ValueError, match="ld >="):
        ops.vad(torch.zeros(1000, device=DEV), torch.tensor([0, 1000], device=DEV), 1000, stat=torch.zeros(1, 2, device=DEV))


def test_non_finite_samples(signals):
    from tiny_audio_amd.vad import DeviceVAD
    x = signals["white-20dB"][0][:64000].copy()
    clean = [signals["pink-20dB"][0][:50001], signals["white-10dB"][0][:33333]]
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[30000] = bad                                                             # frame 117
        with pytest.raises(ValueError, match="non-finite"):
            DeviceVAD().statistic(y)                                               # a host array: refused before the upload
        with pytest.raises(ValueError, match="recording 1 holds non-finite"):
            DeviceVAD().speech_frames([torch.from_numpy(clean[0]).to(DEV), torch.from_numpy(y).to(DEV)])      # device tensors: on the read-back
    y = x.copy()
    y[30000] = np.nan
    from tiny_audio_amd import ops
    flat = torch.from_numpy(np.concatenate([clean[0], y, clean[1]])).to(DEV)
    off = torch.tensor(np.cumsum([0, len(clean[0]), len(y), len(clean[1])]), device=DEV)
    stat, flags, nf = (t.cpu().numpy() for t in ops.vad(flat, off, 64000))
    for r, c in ((0, clean[0]), (2, clean[1])):
        a = _run([c])
        assert np.array_equal(stat[r, :nf[r]].view(np.uint32), a[0][0].view(np.uint32)) and np.array_equal(flags[r, :nf[r]], a[1][0]), r
    bad_frames = np.isnan(stat[1, :nf[1]])
    assert bad_frames[117] and not flags[1, :nf[1]][bad_frames].any()
    ref_bad = np.isnan(R.statistic(y))
    wider = ref_bad.copy()
    wider[1:] |= ref_bad[:-1]
    wider[:-1] |= ref_bad[1:]
    # the NaN reaches every frame the definition says, and beyond them at most the frame that shares a transform with one of them
    assert (bad_frames | ~ref_bad).all() and (wider | ~bad_frames).all() and not bad_frames.all()


def test_operator_passes_opcheck_and_the_python_faces_agree(signals):
    from tiny_audio_amd.diarization import LocalSpeakerDiarizer
    from tiny_audio_amd.vad import DeviceVAD
    x = torch.randn(5000, device=DEV)
    off = torch.tensor([0, 1700, 5000], device=DEV)
    torch.library.opcheck(torch.ops.ta355.vad, (x, off, 3300, 2, 94, 2.0, 0.15, 1e-12), test_utils=("test_schema", "test_faketensor"))
    vad = DeviceVAD()
    a, b = signals["white-10dB"][0], signals["pink-20dB"][0][:100000]
    Ls, fs = vad.statistic([a, b]), vad.speech_frames([a, b])
    assert isinstance(Ls, list) and isinstance(fs, list) and Ls[0].dtype == np.float32 and fs[0].dtype == bool
    one = vad.statistic(a)
    assert isinstance(one, np.ndarray) and np.array_equal(one, Ls[0]) and np.array_equal(vad.speech_frames(a), fs[0])
    assert np.array_equal(fs[1], Ls[1] > np.float32(THETA)) and len(fs[1]) == R.frames_of(100000)
    segs, frames = vad.speech_segments(a)
    want, want_frames = LocalSpeakerDiarizer._get_speech_segments(a, 16000, speech_frames=fs[0])
    assert segs == want and frames.tolist() == want_frames and len(segs) >= 3


# ============================================================================ (d) end to end
def _allowed(spans, n, tol):
    """True bursts (samples) widened by ``tol`` seconds per side and merged where the diarizer may bridge them -> [(lo_s, hi_s)]."""
    from tiny_audio_amd.diarization import LocalSpeakerDiarizer as D
    out = []
    for a, b in spans:
        lo, hi = a / 16000 - tol, b / 16000 + tol
        if out and lo - out[-1][1] <= max(D.VAD_MAX_GAP, D.SAME_SPEAKER_GAP):
            out[-1] = (out[-1][0], hi)
        else:
            out.append((lo, hi))
    return out


def test_diarizer_end_to_end_with_nothing_third_party():
    from tests.golden import ecapa_recipe as ER
    from tiny_audio_amd import ecapa as E
    from tiny_audio_amd.diarization import LocalSpeakerDiarizer as D, SpeakerDiarizer
    from tiny_audio_amd.vad import DeviceVAD
    x, truth, counted, spans = R.synth(5, 12.0, 20, "white")
    m = E.EcapaTdnnMI355X(E.EcapaConfig(**ER.GEOMS["a"]), device=DEV).random_init(0)
    vad = DeviceVAD()
    # boundary frames (4 of 16 ms), the hysteresis padding, one voting frame
    tol = 4 * 0.016 + max(D.VAD_PAD_ONSET, D.VAD_PAD_OFFSET) + D.VOTING_RATE
    allowed = _allowed(spans, len(x), tol)
    vsegs, frames = vad.speech_segments(x)
    assert len(frames) == R.frames_of(len(x)) and vsegs
    for s in vsegs:
        assert any(lo <= s["start"] and s["end"] <= hi for lo, hi in allowed), (s, allowed)
    for a, b in spans:                                                             # every burst is heard
        assert any(s["start"] <= a / 16000 + tol and s["end"] >= b / 16000 - tol for s in vsegs), (a, b, vsegs)
    out = SpeakerDiarizer.diarize(x, vad=vad, speaker_model=m, cluster_device=DEV)
    assert out and all(set(s) == {"speaker", "start", "end"} for s in out)
    for s in out:                                                                  # nothing about the labels: random weights
        assert any(lo <= s["start"] and s["end"] <= hi for lo, hi in allowed), (s, allowed)
    assert len(allowed) >= 2, "the recording must hold a noise-only stretch longer than VAD_MAX_GAP between bursts"


LONG_BURSTS = ((0.5, 1.6), (2.0, 3.2), (3.6, 5.0), (5.3, 6.0), (31.0, 32.2), (32.6, 34.0), (34.4, 35.6), (35.9, 36.6))


@pytest.fixture(scope="module")
def model():
    from oracle import weights as OW
    from tests.golden import recipe as RC
    from tests.test_gpu_longform import _Tok
    from tests.test_gpu_parity import build_model
    S = RC.SMALL
    wE, wL, wP = OW.init_encoder(S["enc"], 0), RC.gen_lm_weights(), OW.init_mlp_projector(S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"])
    m = build_model(S["enc"], S["lm"], S["proj_hidden"], wE, wL, wP, audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"],
                    eos_token_id=S["eos_id"])
    m.tokenizer = _Tok(S["audio_token_id"])
    m.system_prompt = None
    return m


def test_long_form_skips_the_windows_without_speech(model):
    from tiny_audio_amd.vad import DeviceVAD
    m = model
    x = R.synth(9, 37.0, 20, "white", bursts=LONG_BURSTS)[0]
    rows = []
    real_generate = m.generate

    def spy(**kw):
        rows.append(int(kw["input_ids"].shape[0]))
        return real_generate(**kw)

    m.generate = spy
    try:
        res = m.transcribe_long(x, max_window_s=12.0, min_window_s=5.0, max_new_tokens=4, vad=DeviceVAD())
        with_vad = sum(rows)
        rows.clear()
        plain = m.transcribe_long(x, max_window_s=12.0, min_window_s=5.0, max_new_tokens=4)
        without = sum(rows)
    finally:
        del m.generate
    chunks = res["chunks"]
    assert set(res) == {"text", "chunks"} and all(set(c) == {"text", "timestamp", "speech_s"} for c in chunks)
    in_noise = [c for c in chunks if c["timestamp"][0] >= 6.0 + 0.2 and c["timestamp"][1] <= 31.0 - 0.2]
    assert in_noise, [c["timestamp"] for c in chunks]
    for c in in_noise:
        assert c["speech_s"] == 0.0 and c["text"] == ""
    spoken = [c for c in chunks if c["speech_s"] > 0.0]
    assert with_vad == len(spoken) and 2 <= len(spoken) < len(chunks), "only the windows with speech reach generate"
    # the gaps inside either group of bursts (at most 0.4 s) are bridged: 0.5 .. 6.0 s and 31.0 .. 36.6 s, each end within 4 frames + padding
    assert abs(sum(c["speech_s"] for c in chunks) - (5.5 + 5.6)) < 4 * (4 * 0.016 + 0.05)
    assert res["text"] == " ".join(c["text"] for c in chunks if c["text"])
    # without a VAD: today's keys, every window decoded, the same windows
    assert set(plain) == {"text", "chunks"} and all(set(c) == {"text", "timestamp"} for c in plain["chunks"])
    assert without == len(plain["chunks"]) == len(chunks)
    assert [c["timestamp"] for c in plain["chunks"]] == [c["timestamp"] for c in chunks]
    # everything skipped: no call at all
    m.generate = spy
    try:
        rows.clear()
        none = m.transcribe_long(x, max_window_s=12.0, min_window_s=5.0, max_new_tokens=4, vad=DeviceVAD(), min_speech_s=30.0)
    finally:
        del m.generate
    assert not rows and none["text"] == "" and all(c["text"] == "" for c in none["chunks"])

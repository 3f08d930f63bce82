"""-m "not gpu": the host side of voice activity detection (tiny_audio_amd/vad.py, the ``vad`` operator, the ``vad=`` keywords of the
diarizer and of ``transcribe_long``) -- the ABI additions, the dry-run marshalling, every refusal, the run-length helpers against the
diarizer's own frame loop, and the bookkeeping of skipped windows.  The kernels compute nothing here (``_lib.DRY_RUN``): the detector
is played by stubs; the numerics are in tests/test_gpu_vad.py and the definition's own figures in tests/test_vad_ref.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from tests import vad_ref as R
from tests.test_longform_host import _model, _plans, _ramp, _record
from tiny_audio_amd import _lib, ops, torch_ops, vad as V
from tiny_audio_amd.diarization import LocalSpeakerDiarizer, SpeakerDiarizer


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


# ----------------------------------------------------------------------------- the ABI and the operator
def test_header_sources_symbols_and_version(dry):
    protos = _lib.parse_header()
    for name, nargs, ret in (("ta_vad_frames", 1, C.c_long), ("ta_vad_workspace_bytes", 2, C.c_long), ("ta_vad_f32", 12, C.c_int)):
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] is ret, name
    assert "vad.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T ta_vad" in line}
    assert exported == {"ta_vad_frames", "ta_vad_workspace_bytes", "ta_vad_f32"} and exported <= set(protos)
    text = open(_lib.HEADER).read()
    assert "ta_vad_options" in text and "#define TA_VAD_TILE 256" in text and "#define TA_VAD_ENERGY_FRAMES 32" in text
    assert ops.VAD_TILE == 256 and ops.VAD_ENERGY_FRAMES == 32 and ops.VAD_HOP == R.HOP
    assert [f for f, _ in _lib.VadOptions._fields_] == ["smooth", "noise_window", "noise_bias", "threshold", "floor"]
    assert "vad" in torch_ops.OPERATORS
    assert str(torch.ops.ta355.vad.default._schema).startswith("ta355::vad(")
    L = _lib.lib()
    for n in (-5, 0, 1, 256, 257, 512, 513, 1000, 4096, 160 * 1048576):
        assert L.ta_vad_frames(n) == ops.vad_frames(n) == R.frames_of(n) == len(range(0, n - 256, 256)), n
    assert L.ta_vad_workspace_bytes(3, 1000) == 3 * 3 * 64 and L.ta_vad_workspace_bytes(1, 256) == 0
    assert L.ta_vad_workspace_bytes(65, 1000) == 0 and L.ta_vad_workspace_bytes(1, 160 * 1048576 + 1) == 0 and L.ta_vad_workspace_bytes(0, 1000) == 0
    assert L.ta_vad_workspace_bytes(64, 160 * 1048576) == 64 * 655359 * 64


def test_dry_run_marshalling_and_fake_shapes(dry):
    wav, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    stat, flags, nf = torch.ops.ta355.vad(wav, off, 600, 2, 94, 2.0, 0.15, 1e-12)
    assert stat.shape == flags.shape == (2, 2) and stat.dtype == torch.float32 and flags.dtype == torch.uint8
    assert nf.shape == (2,) and nf.dtype == torch.int32 and not stat.any() and not flags.any() and not nf.any()
    assert dry.calls == ["ta_vad_f32"]
    stat, flags, nf = torch.ops.ta355.vad(wav, off[:2], 200, 0, 1, 1.0, 0.5, 1e-9)           # no frame at all: [R, 0]
    assert stat.shape == flags.shape == (1, 0) and dry.calls == ["ta_vad_f32"] * 2
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        got = torch.ops.ta355.vad(torch.empty(1000), torch.empty(3, dtype=torch.int64), 600, 2, 94, 2.0, 0.15, 1e-12)
        assert [(tuple(t.shape), t.dtype) for t in got] == [((2, 2), torch.float32), ((2, 2), torch.uint8), ((2,), torch.int32)]
    vad = V.DeviceVAD()
    assert vad.options() == (2, 94, 2.0, 0.15, 1e-12) and V.DeviceVAD(noise_window_s=0.5).noise_window == 31
    L, f = vad.statistic(np.zeros(1000, np.float32)), vad.speech_frames([np.zeros(1000, np.float32), torch.zeros(300)])
    assert L.shape == (3,) and L.dtype == np.float32 and isinstance(f, list) and [a.shape for a in f] == [(3,), (1,)] and f[0].dtype == bool
    segs, frames = vad.speech_segments(np.zeros(5000, np.float32))
    assert segs == [] and frames.shape == (19,)


def test_every_refusal(dry):
    wav, off = torch.zeros(1000), torch.tensor([0, 1000])
    for kw, what in ((dict(smooth=-1), "smooth"), (dict(smooth=9), "smooth"), (dict(noise_window=0), "noise_window"),
                     (dict(noise_window=1025), "noise_window"), (dict(noise_bias=0.99), "noise_bias"), (dict(noise_bias=float("inf")), "noise_bias"),
                     (dict(noise_bias=float("nan")), "noise_bias"), (dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"),
                     (dict(threshold=float("inf")), "threshold"), (dict(floor=0.0), "floor"), (dict(floor=-1e-12), "floor"),
                     (dict(floor=float("inf")), "floor"), (dict(floor=1e-60), "floor")):
        with pytest.raises(ValueError, match=what):
            ops.vad(wav, off, 1000, **kw)
    ops.vad(wav, off, 1000, smooth=0, noise_window=1, noise_bias=1.0)
    ops.vad(wav, off, 1000, smooth=8, noise_window=1024)
    with pytest.raises(ValueError, match="65 recordings"):
        ops.vad(wav, torch.arange(66), 10)
    with pytest.raises(ValueError, match="beyond the kernel's limit"):
        ops.vad(wav, off, 160 * 1048576 + 1)
    with pytest.raises(ValueError, match="at least 1"):
        ops.vad(wav, off, 0)
    with pytest.raises(ValueError, match="ld >= 3"):
        ops.vad(wav, off, 1000, stat=torch.zeros(1, 2), flags=torch.zeros(1, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one shape"):
        ops.vad(wav, off, 1000, stat=torch.zeros(1, 5), flags=torch.zeros(1, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1-D"):
        ops.vad(torch.zeros(2, 500), off, 1000)
    assert "ta_vad_f32" not in dry.calls[2:], "every refusal comes before any device work"
    for kw in (dict(smooth_frames=9), dict(noise_window_s=0.0), dict(noise_window_s=17.0), dict(noise_window_s=float("nan")), dict(noise_bias=0.5),
               dict(threshold=-1.0), dict(floor=0.0)):
        with pytest.raises(ValueError):
            V.DeviceVAD(**kw)
    vad = V.DeviceVAD()
    with pytest.raises(ValueError, match="1-D"):
        vad.statistic(np.zeros((2, 1000), np.float32))
    with pytest.raises(ValueError, match="non-finite"):
        vad.speech_frames(np.array([0.0, np.nan] * 300, np.float32))
    with pytest.raises(ValueError, match="beyond the cap"):
        vad.statistic(torch.empty(160 * 1048576 + 1, dtype=torch.int8))
    with pytest.raises(ValueError, match="65 recordings"):
        vad.statistic([np.zeros(300, np.float32)] * 65)
    with pytest.raises(ValueError, match="one recording"):
        vad.speech_segments([np.zeros(300, np.float32)])


def test_the_abi_refuses_what_the_python_layer_refuses():
    """The C entry point's own argument checks (they return before any launch, so no GPU is needed)."""
    L = _lib._load()
    good = dict(smooth=2, noise_window=94, noise_bias=2.0, threshold=0.15, floor=1e-12)
    one, buf = C.c_void_p(16), C.c_void_p(32)                       # never dereferenced: every call below is refused first

    def call(R=1, max_n=1000, ld=3, ws_bytes=1 << 20, **kw):
        opt = _lib.VadOptions(**{**good, **kw})
        return L.ta_vad_f32(one, buf, R, max_n, C.byref(opt), one, one, ld, buf, one, ws_bytes, None)

    for kw in (dict(smooth=-1), dict(smooth=9), dict(noise_window=0), dict(noise_window=1025), dict(noise_bias=0.5), dict(noise_bias=float("nan")),
               dict(noise_bias=float("inf")), dict(threshold=0.0), dict(threshold=float("inf")), dict(floor=0.0), dict(floor=float("nan"))):
        assert call(**kw) == 1, kw
    assert call(R=65) == 1 and call(R=-1) == 1 and call(max_n=0) == 1 and call(max_n=160 * 1048576 + 1) == 1
    assert call(ld=2) == 1 and call(ws_bytes=3 * 64 - 1) == 1
    assert L.ta_vad_f32(one, buf, 1, 1000, None, one, one, 3, buf, one, 1 << 20, None) == 1
    assert call(R=0) == 0                                            # an empty batch is no error, and launches nothing


# ----------------------------------------------------------------------------- runs and segments
def test_speech_runs_and_segments_equal_the_diarizers_frame_loop():
    rng = np.random.default_rng(3)
    cases = [np.zeros(0, bool), np.zeros(1, bool), np.ones(1, bool), np.zeros(40, bool), np.ones(40, bool)]
    for p in (0.05, 0.5, 0.95):
        cases += [rng.random(n) < p for n in (2, 7, 100, 2000)]
    sticky = np.repeat(rng.random(60) < 0.4, rng.integers(1, 60, 60))       # long runs: bridged gaps, dropped blips, padded ends
    cases += [sticky, ~sticky, sticky.astype(np.uint8), sticky.tolist()]
    for flags in cases:
        runs = V.speech_runs(flags)
        f = np.asarray(flags).astype(bool)
        assert runs.dtype == np.int64 and runs.shape == (len(runs), 2)
        rebuilt = np.zeros(len(f), bool)
        for a, b in runs:
            assert 0 <= a < b <= len(f) and f[a:b].all() and (a == 0 or not f[a - 1]) and (b == len(f) or not f[b])
            rebuilt[a:b] = True
        assert np.array_equal(rebuilt, f)
        want, want_frames = LocalSpeakerDiarizer._get_speech_segments(np.zeros(256 * len(f) + 257, np.float32), 16000, speech_frames=flags)
        assert V.segments_from_flags(flags) == want and want_frames == f.tolist()

    vad = V.DeviceVAD()
    vad.speech_frames = lambda wave: sticky                                   # the detector's decisions, fixed
    segs, frames = vad.speech_segments(np.zeros(10, np.float32))
    assert segs == LocalSpeakerDiarizer._get_speech_segments(None, 16000, speech_frames=sticky)[0] and frames is sticky


def test_speech_runs_handles_a_recording_at_the_cap_without_a_frame_loop():
    flags = np.zeros(655359, np.uint8)
    flags[1000:5000] = 1
    flags[400000:400003] = 1
    assert V.speech_runs(flags).tolist() == [[1000, 5000], [400000, 400003]]
    segs = V.segments_from_flags(flags)
    assert len(segs) == 1 and segs[0]["start"] == pytest.approx(16.0 - 0.05) and segs[0]["end"] == pytest.approx(80.0 + 0.05)


# ----------------------------------------------------------------------------- the diarizer
class _WholeVad:
    """An object with ``speech_frames`` only: any look for ``process`` is an error."""

    def __init__(self, flags):
        self.flags, self.calls = flags, []

    def speech_frames(self, audio):
        self.calls.append(audio)
        return self.flags

    def __getattr__(self, name):
        if name == "process":
            raise AssertionError("the diarizer looked for process() on a whole-recording detector")
        raise AttributeError(name)


def test_the_diarizer_calls_a_whole_recording_detector_exactly_once():
    from tests.golden import diarization_recipe as D
    audio = (0.1 * np.random.default_rng(0).standard_normal(256 * 125 + 7)).astype(np.float32)
    frames = len(range(0, len(audio) - 256, 256))
    flags = np.zeros(frames, bool)
    flags[10:60] = True
    flags[70:90] = True
    vad = _WholeVad(flags)
    segs, got = LocalSpeakerDiarizer._get_speech_segments(audio.astype(np.float32), 16000, vad=vad)
    want, want_frames = LocalSpeakerDiarizer._get_speech_segments(audio, 16000, speech_frames=flags)
    assert len(vad.calls) == 1 and vad.calls[0].shape == audio.shape and segs == want and got == want_frames and isinstance(got, list)

    class Marker:
        def embed_windows(self, buf, starts, lengths, window):
            e = np.zeros((len(starts), 8), np.float32)
            e[:, 0] = 1.0
            e[:, 1] = np.arange(len(starts)) % 2
            return torch.from_numpy(e)

    vad = _WholeVad(flags)
    a = SpeakerDiarizer.diarize(audio, vad=vad, speaker_model=Marker())
    b = SpeakerDiarizer.diarize(audio, speech_frames=flags, speaker_model=Marker())
    assert len(vad.calls) == 1 and a == b and a
    # speech_frames= wins over vad=, and the process() protocol is what it was
    vad = _WholeVad(flags)
    assert LocalSpeakerDiarizer._get_speech_segments(audio, 16000, speech_frames=flags, vad=vad)[0] == want and not vad.calls
    assert LocalSpeakerDiarizer._get_speech_segments(audio, 16000, vad=D.ReplayVad(flags.tolist()))[0] == want


# ----------------------------------------------------------------------------- transcribe_long
class _StubVad:
    """``run_uploaded`` of a detector whose decisions are given per recording."""

    def __init__(self, flags_per_recording):
        self.flags, self.calls = flags_per_recording, 0

    def run_uploaded(self, flat, offsets, lens):
        self.calls += 1
        assert flat.dim() == 1 and offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        F = max(ops.vad_frames(n) for n in lens)
        out = torch.zeros((len(lens), F), dtype=torch.uint8)
        for r, f in enumerate(self.flags):
            assert len(f) == ops.vad_frames(lens[r])
            out[r, :len(f)] = torch.from_numpy(np.asarray(f, np.uint8))
        return torch.zeros((len(lens), F)), out, torch.tensor([ops.vad_frames(n) for n in lens], dtype=torch.int32)


def test_transcribe_long_skips_windows_without_speech(dry, monkeypatch):
    m = _model()
    n0, n1 = 160 * 1000, 160 * 800
    _plans(monkeypatch, [0, 300, 500, 900, 1000], [0, 400, 800])
    # recording 0 (windows 0-3 s, 3-5 s, 5-9 s, 9-10 s): speech 1.0 .. 2.0 s and 4.96 .. 5.6 s; recording 1: none at all
    f0 = np.zeros(ops.vad_frames(n0), bool)
    f0[int(1.0 / 0.016) + 1:int(2.0 / 0.016)] = True
    f0[310:350] = True
    vad = _StubVad([f0, np.zeros(ops.vad_frames(n1), bool)])
    segs = V.segments_from_flags(f0)
    assert len(segs) == 2

    def inside(w0, w1):
        return sum(max(0.0, min(s["end"], w1) - max(s["start"], w0)) for s in segs)

    calls = _record(m, monkeypatch)
    res = m.transcribe_long([_ramp(n0, 5000), _ramp(n1, 7000)], batch_size=8, max_new_tokens=4, vad=vad)
    assert vad.calls == 1 and len(calls) == 1 and calls[0]["input_ids"].shape[0] == 3, "three windows hold speech; they share one batch"
    firsts = sorted(int(round(float(v))) for v in calls[0]["input_features"][:, 0, 0])
    assert firsts == [5000, 5300, 5500]
    c0, c1 = res[0]["chunks"], res[1]["chunks"]
    assert all(set(c) == {"text", "timestamp", "speech_s"} for c in c0 + c1)
    assert [c["speech_s"] for c in c0] == pytest.approx([inside(0, 3), inside(3, 5), inside(5, 9), 0.0]) and c0[1]["speech_s"] == pytest.approx(0.09, abs=1e-9)
    assert [bool(c["text"]) for c in c0] == [True, True, True, False] and [c["timestamp"] for c in c0] == [(0.0, 3.0), (3.0, 5.0), (5.0, 9.0), (9.0, 10.0)]
    assert [c["speech_s"] for c in c1] == [0.0, 0.0] and [c["text"] for c in c1] == ["", ""] and res[1]["text"] == ""
    assert res[0]["text"] == " ".join(c["text"] for c in c0 if c["text"])
    # min_speech_s: the 0.09 s window goes too (speech_s <= min_speech_s is skipped)
    calls.clear()
    res = m.transcribe_long([_ramp(n0, 5000), _ramp(n1, 7000)], batch_size=8, vad=vad, min_speech_s=0.09 + 1e-9)
    assert calls[0]["input_ids"].shape[0] == 2 and [bool(c["text"]) for c in res[0]["chunks"]] == [True, False, True, False]
    # everything skipped: nothing is decoded, the text is empty
    calls.clear()
    _plans(monkeypatch, [0, 400, 800])
    res = m.transcribe_long(_ramp(n1, 7000), vad=_StubVad([np.zeros(ops.vad_frames(n1), bool)]))
    assert not calls and res["text"] == "" and [c["text"] for c in res["chunks"]] == ["", ""]


def test_skipped_windows_have_no_words(dry, monkeypatch):
    from tiny_audio_amd.alignment import ForcedAligner
    m = _model()
    _plans(monkeypatch, [0, 300, 700])
    _record(m, monkeypatch)
    seen = []

    def align_audio_batch(audios, texts, acoustic_model, **kw):
        seen.append([int(a.shape[0]) for a in audios])
        return [[{"word": "w", "start": 0.25, "end": 0.5}] for _ in texts]

    monkeypatch.setattr(ForcedAligner, "align_audio_batch", staticmethod(align_audio_batch))
    f = np.zeros(ops.vad_frames(160 * 700), bool)
    f[250:400] = True                                                         # 4.0 .. 6.4 s: the second window only
    res = m.transcribe_long(_ramp(160 * 700, 5000), return_timestamps=True, acoustic_model="AM", vad=_StubVad([f]))
    assert seen == [[64000]] and res["words"] == [{"word": "w", "start": 3.25, "end": 3.5}]


def test_without_a_vad_the_result_is_todays(dry, monkeypatch):
    m = _model()
    _plans(monkeypatch, [0, 300, 700])
    calls = _record(m, monkeypatch)
    res = m.transcribe_long(_ramp(160 * 700, 5000))
    assert set(res) == {"text", "chunks"} and all(set(c) == {"text", "timestamp"} for c in res["chunks"])
    assert calls[0]["input_ids"].shape[0] == 2 and "ta_vad_f32" not in dry.calls
    assert "vad" not in calls[0] and "min_speech_s" not in calls[0], "the new keywords are not generate keywords"
    with pytest.raises(ValueError, match="needs vad="):
        m.transcribe_long(_ramp(160 * 700, 5000), min_speech_s=0.5)
    with pytest.raises(ValueError, match="min_speech_s"):
        m.transcribe_long(_ramp(160 * 700, 5000), vad=V.DeviceVAD(), min_speech_s=-1.0)
    with pytest.raises(ValueError, match="run_uploaded"):
        m.transcribe_long(_ramp(160 * 700, 5000), vad=object())
    # a DeviceVAD under dry run: the operator is reached on the uploaded buffer, its zeros skip every window
    calls.clear()
    res = m.transcribe_long(_ramp(160 * 700, 5000), vad=V.DeviceVAD())
    assert "ta_vad_f32" in dry.calls and not calls and res["text"] == "" and [c["speech_s"] for c in res["chunks"]] == [0.0, 0.0]

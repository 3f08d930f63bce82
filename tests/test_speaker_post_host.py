"""-m "not gpu": the host side of the speaker-turn stage (csrc/speaker_post.hip; ``spk_vote`` / ``spk_merge`` / ``spk_words``; the
``device=`` / ``post_device=`` keywords of the diarizer; ``transcribe_long(return_speakers=True)``) -- the ABI additions, the workspace
query, every refusal, the dry-run marshalling and launch order, and that nothing changes without the new keywords.  The kernels
compute nothing here (``_lib.DRY_RUN``); their results are in tests/test_gpu_speaker_post.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from tests.golden import diarization_recipe as D
from tests.test_longform_host import _model, _plans, _ramp, _record
from tiny_audio_amd import _lib, ops, torch_ops
from tiny_audio_amd.diarization import LocalSpeakerDiarizer, SpeakerDiarizer

OPT = LocalSpeakerDiarizer.spk_options()
I32 = torch.int32


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def i32(*v):
    return torch.tensor(v, dtype=I32)


# ----------------------------------------------------------------------------- the ABI and the operators
def test_header_sources_symbols_and_version(dry):
    protos = _lib.parse_header()
    for name, nargs, ret in (("ta_spk_post_workspace_bytes", 4, C.c_long), ("ta_spk_vote_i32", 22, C.c_int), ("ta_spk_merge_i32", 12, C.c_int),
                             ("ta_spk_words_f64", 10, C.c_int)):
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] is ret, name
    assert "speaker_post.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T ta_spk_" in line}
    assert {"ta_spk_post_workspace_bytes", "ta_spk_vote_i32", "ta_spk_merge_i32", "ta_spk_words_f64"} <= exported <= set(protos)
    text = open(_lib.HEADER).read()
    for cite in ("tiny_audio/diarization.py:520-537", "tiny_audio/diarization.py:539-614", "tiny_audio/diarization.py:616-643",
                 "tiny_audio/diarization.py:645-682", "ta_spk_post_options", f"#define TA_SPK_FRAME_TILE {ops.SPK_FRAME_TILE}",
                 f"#define TA_SPK_SEG_TILE {ops.SPK_SEG_TILE}", f"#define TA_SPK_MAX_FRAMES {ops.SPK_LIMITS['frames']}",
                 f"#define TA_SPK_MAX_ITEMS {ops.SPK_LIMITS['items']}", f"#define TA_SPK_MAX_SPEAKERS {ops.SPK_LIMITS['speakers']}",
                 f"#define TA_SPK_MAX_RECORDINGS {ops.SPK_LIMITS['recordings']}"):
        assert cite in text, cite
    assert [f for f, _ in _lib.SpkPostOptions._fields_] == list(ops.SPK_OPTION_NAMES) and C.sizeof(_lib.SpkPostOptions) == 40
    assert {"spk_vote", "spk_merge", "spk_words"} <= set(torch_ops.OPERATORS)
    for name in ("spk_vote", "spk_merge", "spk_words"):
        assert str(getattr(torch.ops.ta355, name).default._schema).startswith(f"ta355::{name}(")
    src = open(_lib.CSRC + "/speaker_post.hip").read()
    assert "#pragma clang fp contract(off)" in src and "fast" not in _lib.build.__doc__.lower()
    assert ops.SPK_LIMITS == {"recordings": 64, "speakers": 16, "frames": 1048577, "items": 1048576}


def test_the_workspace_query(dry):
    L = _lib.lib()
    assert L.ta_spk_post_workspace_bytes(1, 1, 0, 0) == 16 + 64 + 16 + 4 + 8
    assert L.ta_spk_post_workspace_bytes(2, 3, 2049, 10) == 2 * 3 * 2052 * 4 + 2 * 3 * 64 + 16 + 2 * 2052 + 2 * 3 * 8
    assert L.ta_spk_post_workspace_bytes(64, 16, 1048577, 1048576) > 2 ** 32            # a long: the cap of everything at once is 4 GB
    for bad in ((0, 1, 10, 1), (65, 1, 10, 1), (1, 0, 10, 1), (1, 17, 10, 1), (1, 1, -1, 1), (1, 1, 1048578, 1), (1, 1, 10, -1),
                (1, 1, 10, 1048577)):
        assert L.ta_spk_post_workspace_bytes(*bad) == -1, bad


def test_the_abi_refuses_what_the_python_layer_refuses():
    """The entry points' own argument checks return before any HIP call, so no GPU is needed."""
    L = _lib._load()
    p = C.c_void_p(64)                                                # never dereferenced: every call below is refused first
    good = _lib.SpkPostOptions(*OPT)

    def vote(R=1, S=2, max_frames=100, n_win=3, opt=good, ws=p, ws_bytes=1 << 30, ld=4):
        return L.ta_spk_vote_i32(p, p, p, p, n_win, R, S, p, max_frames, p, ld, p, None if opt is None else C.byref(opt), p, p, p, p, p, p,
                                 ws, ws_bytes, None)

    assert vote(R=65) == 1 and vote(R=-1) == 1 and vote(S=0) == 1 and vote(S=17) == 1 and vote(max_frames=1048578) == 1
    assert vote(max_frames=-1) == 1 and vote(n_win=1048577) == 1 and vote(n_win=-1) == 1 and vote(opt=None) == 1 and vote(ws=None) == 1
    assert vote(ws_bytes=L.ta_spk_post_workspace_bytes(1, 2, 100, 3) - 1) == 1 and vote(ld=-1) == 1
    assert vote(R=0) == 0                                             # an empty batch is no error and launches nothing
    for k in range(5):
        for v in (0.0, -0.01, float("nan"), float("inf")):
            vals = list(OPT)
            vals[k] = v
            bad = _lib.SpkPostOptions(*vals)
            assert vote(opt=bad) == 1, (k, v)
            assert L.ta_spk_merge_i32(p, p, p, p, None, 1, C.byref(bad), p, p, p, p, None) == 1
    assert L.ta_spk_merge_i32(p, p, p, p, None, 65, C.byref(good), p, p, p, p, None) == 1
    assert L.ta_spk_merge_i32(p, p, p, None, None, 1, C.byref(good), p, p, p, p, None) == 1
    assert L.ta_spk_merge_i32(p, p, p, p, None, 0, C.byref(good), p, p, p, p, None) == 0
    assert L.ta_spk_words_f64(p, p, p, p, p, p, 65, 10, p, None) == 1 and L.ta_spk_words_f64(p, p, p, p, p, p, 1, 1048577, p, None) == 1
    assert L.ta_spk_words_f64(p, p, p, p, p, p, 1, -1, p, None) == 1 and L.ta_spk_words_f64(p, p, None, p, p, p, 1, 5, p, None) == 1
    assert L.ta_spk_words_f64(p, p, p, p, p, p, 0, 5, p, None) == 0 and L.ta_spk_words_f64(p, p, p, p, p, p, 3, 0, p, None) == 0


def _vote_args(**kw):
    a = dict(first=i32(0, 5, 2), last=i32(4, 9, 2), label=i32(0, 1, 0), cu_win=i32(0, 2, 3), S=2, n_frames=i32(10, 4), max_frames=10,
             vad=torch.ones(2, 6, dtype=torch.uint8), n_vad=i32(6, 0), cu_cap=i32(0, 6, 9), options=OPT)
    a.update(kw)
    return a


def test_dry_run_marshalling_and_fake_shapes(dry):
    run_spk, run_f0, run_f1, n_runs, status = ops.spk_vote(**_vote_args())
    assert run_spk.shape == run_f0.shape == run_f1.shape == (9,) and n_runs.shape == status.shape == (2,) and run_spk.dtype == I32
    seg = ops.spk_merge(run_spk, run_f0, run_f1, i32(0, 6, 9), OPT, n_run=n_runs)
    assert [t.shape for t in seg] == [(9,), (9,), (9,), (2,)]
    w = ops.spk_words(torch.zeros(5, dtype=torch.float64), torch.ones(5, dtype=torch.float64), i32(0, 2, 5), torch.zeros(3, dtype=torch.float64),
                      torch.ones(3, dtype=torch.float64), i32(0, 3, 3))
    assert w.shape == (5,) and w.dtype == I32
    assert dry.calls == ["ta_spk_vote_i32", "ta_spk_merge_i32", "ta_spk_words_f64"]
    a = _vote_args()
    got = torch.ops.ta355.spk_vote(a["first"], a["last"], a["label"], a["cu_win"], 2, a["n_frames"], 10, a["vad"], a["n_vad"], a["cu_cap"], 9, *OPT)
    assert [tuple(t.shape) for t in got] == [(9,), (9,), (9,), (2,), (2,)]
    got = torch.ops.ta355.spk_merge(got[0], got[1], got[2], a["cu_cap"], None, *OPT)
    assert [tuple(t.shape) for t in got] == [(9,), (9,), (9,), (2,)]
    # no words, or no recording: nothing is launched
    n = len(dry.calls)
    e = torch.zeros(0, dtype=torch.float64)
    assert ops.spk_words(e, e, i32(0, 0), torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64), i32(0, 2)).shape == (0,)
    assert len(dry.calls) == n
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        z = lambda n, dt=I32: torch.empty(n, dtype=dt)  # noqa: E731
        got = torch.ops.ta355.spk_vote(z(3), z(3), z(3), z(3), 2, z(2), 10, torch.empty(2, 6, dtype=torch.uint8), z(2), z(3), 9, *OPT)
        assert [(tuple(t.shape), t.dtype) for t in got] == [((9,), I32)] * 3 + [((2,), I32)] * 2
        got = torch.ops.ta355.spk_merge(z(9), z(9), z(9), z(3), z(2), *OPT)
        assert [(tuple(t.shape), t.dtype) for t in got] == [((9,), I32)] * 3 + [((2,), I32)]
        got = torch.ops.ta355.spk_words(z(5, torch.float64), z(5, torch.float64), z(3), z(4, torch.float64), z(4, torch.float64), z(3))
        assert tuple(got.shape) == (5,) and got.dtype == I32


def test_every_refusal(dry):
    for kw, what in ((dict(S=0), "speakers"), (dict(S=17), "speakers"), (dict(max_frames=1048578), "1048577"),
                     (dict(label=i32(0, 2, 0)), r"outside \[0, 2\)"), (dict(label=i32(0, -1, 0)), "outside"),
                     (dict(first=i32(0, -1, 2)), "first >= 0"), (dict(n_frames=i32(10, 11)), "max_frames"), (dict(n_frames=i32(-1, 4)), "max_frames"),
                     (dict(n_vad=i32(7, 0)), "n_vad"), (dict(cu_win=i32(0, 2, 4)), "ascend"), (dict(cu_win=i32(0, 3, 2)), "ascend"),
                     (dict(cu_cap=i32(1, 6, 9)), "ascend"), (dict(last=i32(4, 9)), "one length"), (dict(first=torch.zeros(3)), "one length"),
                     (dict(vad=torch.ones(2, 6)), "uint8"), (dict(n_frames=i32(10)), "n_frames"), (dict(capacity=8), "ascend")):
        with pytest.raises(ValueError, match=what):
            ops.spk_vote(**_vote_args(**kw))
    for k, name in enumerate(ops.SPK_OPTION_NAMES):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            o = list(OPT)
            o[k] = v
            with pytest.raises(ValueError, match=name):
                ops.spk_vote(**_vote_args(options=o))
            with pytest.raises(ValueError, match=name):
                ops.spk_merge(i32(0), i32(0), i32(5), i32(0, 1), o)
    with pytest.raises(ValueError, match="65 recordings"):
        ops.spk_merge(i32(), i32(), i32(), torch.zeros(66, dtype=I32), OPT)
    big = torch.zeros(1048577, dtype=I32)
    with pytest.raises(ValueError, match="1048577 runs"):
        ops.spk_merge(big, big, big, i32(0, 1048577), OPT)
    with pytest.raises(ValueError, match="1048577 windows"):
        ops.spk_vote(**_vote_args(first=big, last=big, label=big, cu_win=i32(0, 1048577, 1048577)))
    with pytest.raises(ValueError, match="ascend"):
        ops.spk_merge(i32(0, 0), i32(0, 1), i32(5, 6), i32(0, 1), OPT)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    with pytest.raises(ValueError, match="word's start or end is not finite"):
        ops.spk_words(f64(0.0, float("nan")), f64(1.0, 2.0), i32(0, 2), f64(0.0), f64(1.0), i32(0, 1))
    with pytest.raises(ValueError, match="segment's start or end is not finite"):
        ops.spk_words(f64(0.0, 1.0), f64(1.0, 2.0), i32(0, 2), f64(0.0), f64(float("inf")), i32(0, 1))
    with pytest.raises(ValueError, match="float64"):
        ops.spk_words(torch.zeros(2), torch.ones(2), i32(0, 2), f64(0.0), f64(1.0), i32(0, 1))
    with pytest.raises(ValueError, match="2 recordings"):
        ops.spk_words(f64(0.0, 1.0), f64(1.0, 2.0), i32(0, 1, 2), f64(0.0), f64(1.0), i32(0, 1))
    with pytest.raises(ValueError, match="1048577 words"):
        ops.spk_words(torch.zeros(1048577, dtype=torch.float64), torch.zeros(1048577, dtype=torch.float64), i32(0, 1048577), f64(0.0), f64(1.0), i32(0, 1))
    assert not dry.calls, "every refusal comes before any device work"
    # the diarizer's own refusals, all on the host
    win = [{"start": 0.0, "end": 0.75}]
    with pytest.raises(ValueError, match="first >= 0"):
        LocalSpeakerDiarizer._postprocess_segments([{"start": -0.02, "end": 0.75}], [0], 2.0, [True] * 100, device="cpu")
    with pytest.raises(ValueError, match="at most 16"):
        LocalSpeakerDiarizer._postprocess_segments(win * 17, list(range(17)), 2.0, [True] * 100, device="cpu")
    with pytest.raises(ValueError, match="1048577 per recording"):
        LocalSpeakerDiarizer._postprocess_segments(win, [0], 10485.77, [True] * 100, device="cpu")
    with pytest.raises(ValueError, match="not finite"):
        LocalSpeakerDiarizer._postprocess_segments([{"start": 0.0, "end": float("nan")}], [0], 2.0, [True] * 100, device="cpu")
    with pytest.raises(ValueError, match="voting grid"):
        LocalSpeakerDiarizer._merge_short_segments([{"speaker": "SPEAKER_0", "start": 0.005, "end": 1.0}], device="cpu")
    with pytest.raises(ValueError, match="word's start or end is not finite"):
        LocalSpeakerDiarizer.assign_speakers_to_words([{"word": "a", "start": float("inf"), "end": 1.0}],
                                                      [{"speaker": "SPEAKER_0", "start": 0.0, "end": 1.0}], device="cpu")
    with pytest.raises(ValueError, match="segment's start or end is not finite"):
        LocalSpeakerDiarizer.assign_speakers_to_words([{"word": "a", "start": 0.0, "end": 1.0}],
                                                      [{"speaker": "SPEAKER_0", "start": 0.0, "end": float("nan")}], device="cpu")
    assert not dry.calls


# ----------------------------------------------------------------------------- the host's share
def test_vote_inputs_turns_from_frames_and_options():
    for name, (wins, labels, duration, _vad) in D.postprocess_cases().items():
        if not wins:
            continue
        first, last, rank, names, n_frames = LocalSpeakerDiarizer.vote_inputs(wins, labels, duration)
        r = LocalSpeakerDiarizer.VOTING_RATE
        assert n_frames == int(np.ceil(duration / r)) + 1 and first.dtype == last.dtype == rank.dtype == np.int32
        speakers = np.unique(labels)
        for w, lbl, a, b, k in zip(wins, labels, first, last, rank):
            assert b == min(int(w["end"] / r), n_frames) and speakers[k] == lbl
            assert a == int(w["start"] / r) or (a == n_frames and int(w["start"] / r) >= n_frames)
        assert names == [f"SPEAKER_{k}" for k in range(len(speakers))]
    got = LocalSpeakerDiarizer.turns_from_frames([1, 0], [14, 57], [29, 700], ["A", "B"])
    assert got == [{"speaker": "B", "start": 14 * 0.01, "end": 29 * 0.01}, {"speaker": "A", "start": 57 * 0.01, "end": 700 * 0.01}]
    assert got[1]["start"] == 0.5700000000000001, "the time is the product, not the decimal"

    class Coarse(LocalSpeakerDiarizer):
        VOTING_RATE = 0.02
        MIN_SEGMENT_DURATION = 0.3
        SAME_SPEAKER_GAP = 1.0

    assert LocalSpeakerDiarizer.spk_options() == (0.01, 0.016, 0.15, 0.1, 0.5) and Coarse.spk_options() == (0.02, 0.016, 0.3, 0.1, 1.0)
    assert Coarse.turns_from_frames([0], [3], [7], ["S"]) == [{"speaker": "S", "start": 3 * 0.02, "end": 7 * 0.02}]
    assert Coarse.vote_inputs([{"start": 0.1, "end": 0.5}], [4], 1.0)[:3] == (np.array([5]), np.array([25]), np.array([0]))


# ----------------------------------------------------------------------------- the diarizer
class _Marker:
    """A speaker model whose embeddings alternate between two directions."""

    def __init__(self):
        self.calls = []

    def embed_windows(self, buf, starts, lengths, window):
        self.calls.append((buf, list(starts), list(lengths), window))
        e = np.zeros((len(starts), 8), np.float32)
        e[:, 0] = 1.0
        e[:, 1] = np.arange(len(starts)) % 2
        return torch.from_numpy(e)


class _StubVad:
    """A detector with ``run_uploaded`` / ``speech_frames_uploaded`` whose decisions are given per recording."""

    def __init__(self, flags_per_recording):
        self.flags, self.calls = flags_per_recording, 0

    def run_uploaded(self, flat, offsets, lens):
        self.calls += 1
        F = max(ops.vad_frames(n) for n in lens)
        out = torch.zeros((len(lens), F), dtype=torch.uint8)
        for r, f in enumerate(self.flags):
            assert len(f) == ops.vad_frames(lens[r])
            out[r, :len(f)] = torch.from_numpy(np.asarray(f, np.uint8))
        return torch.zeros((len(lens), F)), out, torch.tensor([ops.vad_frames(n) for n in lens], dtype=I32)

    def speech_frames_uploaded(self, flat, offsets, lens):
        _s, flags, nf = self.run_uploaded(flat, offsets, lens)
        return [np.asarray(f, bool) for f in self.flags], flags, nf


def _audio_and_flags(n=256 * 125 + 7):
    audio = (0.1 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)
    flags = np.zeros(len(range(0, n - 256, 256)), bool)
    flags[10:60] = True
    flags[70:90] = True
    return audio, flags


def test_diarize_post_device_launch_order_and_default_path(dry):
    audio, flags = _audio_and_flags()
    want = SpeakerDiarizer.diarize(audio, speech_frames=flags, speaker_model=_Marker())
    assert want and not dry.calls, "the default path launches nothing"
    got = SpeakerDiarizer.diarize(audio, speech_frames=flags, speaker_model=_Marker(), post_device="cpu")
    assert dry.calls == ["ta_spk_vote_i32", "ta_spk_merge_i32"] and got == [], "(the dry run computes no turns)"
    dry.calls.clear()
    vad = _StubVad([flags])
    assert LocalSpeakerDiarizer.diarize(audio, vad=vad, speaker_model=_Marker(), post_device="cpu") == []
    assert vad.calls == 1 and dry.calls == ["ta_spk_vote_i32", "ta_spk_merge_i32"]
    # a batch: one launch each for both recordings; a recording without speech is part of it and has no turns
    dry.calls.clear()
    short, _ = _audio_and_flags(256 * 40 + 1)
    vad = _StubVad([flags, np.zeros(40, bool)])
    got = SpeakerDiarizer.diarize_batch([audio, short], vad=vad, speaker_model=_Marker(), post_device="cpu")
    assert got == [[], []] and vad.calls == 1 and dry.calls == ["ta_spk_vote_i32", "ta_spk_merge_i32"]
    # without post_device the batch is the single calls
    dry.calls.clear()
    assert SpeakerDiarizer.diarize_batch([audio], speech_frames=[flags], speaker_model=_Marker()) == [want] and not dry.calls
    with pytest.raises(ValueError, match="2 lists for 1 recordings"):
        SpeakerDiarizer.diarize_batch([audio], speech_frames=[flags, flags])
    # the three functions' device= reach their operator
    LocalSpeakerDiarizer._merge_short_segments([{"speaker": "SPEAKER_0", "start": 0.0, "end": 1.0}], device="cpu")
    words = [{"word": "a", "start": 0.0, "end": 0.4}]
    assert LocalSpeakerDiarizer.assign_speakers_to_words(words, [], device="cpu")[0]["speaker"] is None
    SpeakerDiarizer.assign_speakers_to_words(words, [{"speaker": "SPEAKER_3", "start": 0.0, "end": 1.0}], device="cpu")
    assert dry.calls == ["ta_spk_merge_i32", "ta_spk_words_f64", "ta_spk_words_f64"] and words[0]["speaker"] == "SPEAKER_3"


# ----------------------------------------------------------------------------- transcribe_long
def _aligner(monkeypatch):
    from tiny_audio_amd.alignment import ForcedAligner

    def align_audio_batch(audios, texts, acoustic_model, **kw):
        return [[{"word": "w", "start": 0.25, "end": 0.5}, {"word": "v", "start": 0.5, "end": 0.75}] for _ in texts]

    monkeypatch.setattr(ForcedAligner, "align_audio_batch", staticmethod(align_audio_batch))


def test_transcribe_long_return_speakers_launch_order_and_keys(dry, monkeypatch):
    m = _model()
    n0, n1 = 160 * 700, 160 * 300
    _plans(monkeypatch, [0, 300, 700], [0, 300])
    _record(m, monkeypatch)
    _aligner(monkeypatch)
    f0 = np.zeros(ops.vad_frames(n0), bool)
    f0[20:150] = True
    f0[250:400] = True
    vad, spk = _StubVad([f0, np.zeros(ops.vad_frames(n1), bool)]), _Marker()
    res = m.transcribe_long([_ramp(n0, 5000), _ramp(n1, 7000)], vad=vad, speaker_model=spk, acoustic_model="AM", return_speakers=True)
    assert vad.calls == 1, "the detector runs once: its flags serve speech_s, the skipping and the diarizer"
    assert [c for c in dry.calls if c.startswith(("ta_spk_", "ta_vad"))] == ["ta_spk_vote_i32", "ta_spk_merge_i32", "ta_spk_words_f64"]
    assert len(spk.calls) == 1 and spk.calls[0][0].dim() == 1 and spk.calls[0][0].numel() == n0 + n1, "one embed_windows call on the uploaded buffer"
    for r in res:
        assert set(r) == {"text", "chunks", "words", "speaker_segments"} and r["speaker_segments"] == []
        assert all(set(w) == {"word", "start", "end", "speaker"} and w["speaker"] is None for w in r["words"])
    assert len(res[0]["words"]) == 4 and res[1]["words"] == [], "a recording without speech: no words, no segments, no error"
    # the same call without the flag: today's keys and values
    plain = m.transcribe_long([_ramp(n0, 5000), _ramp(n1, 7000)], vad=vad, acoustic_model="AM", return_timestamps=True)
    for a, b in zip(plain, res):
        assert set(a) == {"text", "chunks", "words"} and a["text"] == b["text"] and a["chunks"] == b["chunks"]
        assert a["words"] == [{k: v for k, v in w.items() if k != "speaker"} for w in b["words"]]


def test_transcribe_long_refusals_and_the_unchanged_default(dry, monkeypatch):
    m = _model()
    _plans(monkeypatch, [0, 300, 700])
    calls = _record(m, monkeypatch)
    _aligner(monkeypatch)
    audio = _ramp(160 * 700, 5000)
    vad = _StubVad([np.ones(ops.vad_frames(160 * 700), bool)])
    with pytest.raises(ValueError, match="return_speakers=True needs acoustic_model"):
        m.transcribe_long(audio, return_speakers=True, vad=vad, speaker_model=_Marker())
    with pytest.raises(ValueError, match="return_speakers=True needs speaker_model"):
        m.transcribe_long(audio, return_speakers=True, vad=vad, acoustic_model="AM")
    with pytest.raises(ValueError, match="return_speakers=True needs speaker_model"):
        m.transcribe_long(audio, return_speakers=True, vad=vad, acoustic_model="AM", speaker_model=object())
    with pytest.raises(ValueError, match="return_speakers=True needs vad"):
        m.transcribe_long(audio, return_speakers=True, acoustic_model="AM", speaker_model=_Marker())
    with pytest.raises(ValueError, match="run_uploaded"):
        m.transcribe_long(audio, return_speakers=True, acoustic_model="AM", speaker_model=_Marker(), vad=object())
    assert not calls and not dry.calls
    res = m.transcribe_long(audio)
    assert set(res) == {"text", "chunks"} and all(set(c) == {"text", "timestamp"} for c in res["chunks"])
    assert not [c for c in dry.calls if c.startswith("ta_spk_")]
    for k in ("return_speakers", "speaker_model", "num_speakers", "min_speakers", "max_speakers", "cluster_device"):
        assert k not in calls[0], "the new keywords are not generate keywords"
    res = m.transcribe_long(audio, return_timestamps=True, acoustic_model="AM", vad=vad)
    assert set(res) == {"text", "chunks", "words"} and all(set(w) == {"word", "start", "end"} for w in res["words"])
    assert all(set(c) == {"text", "timestamp", "speech_s"} for c in res["chunks"])

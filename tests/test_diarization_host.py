"""Speaker diarization, host side (no GPU): every result the reference returned for the inputs of tests/golden/diarization_recipe.py
(tests/golden/diarization.json), equal exactly -- labels as partitions, floats as the same Python floats; the assertions of the
reference's own tests/test_diarization.py, restated; the window plumbing of the device path against a recording stand-in; the
``ImportError`` paths."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.golden import diarization_recipe as D
from tiny_audio_amd import diarization as M
from tiny_audio_amd.diarization import LocalSpeakerDiarizer as L
from tiny_audio_amd.diarization import SpeakerClusterer, SpeakerDiarizer, SpectralCluster

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "diarization.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _clean_singletons():
    yield
    L._ten_vad_model = L._ecapa_model = L._device = None


# ----------------------------------------------------------------------------- the reference's recorded results
@pytest.mark.parametrize("name", list(D.embedding_sets()))
def test_clusterer_returns_the_reference_partition(gold, name):
    emb, k = D.embedding_sets()[name]
    want = gold["clusterer"][name]
    np.random.seed(D.NUMPY_SEED)
    if "raises" in want:
        with pytest.raises(ValueError, match="finite"):
            SpeakerClusterer()(emb.copy(), k)
        return
    labels = SpeakerClusterer()(emb.copy(), k)
    assert D.partition(labels) == want["partition"] and [int(x) for x in labels] == want["labels_in_order"]
    assert labels.dtype.kind == "i" and len(labels) == len(emb)


def test_clusterer_edges_and_oracle_reset():
    with pytest.raises(ValueError, match="Expected 2D array"):
        SpeakerClusterer()(np.zeros(5))
    c = SpeakerClusterer(min_num_spks=2, max_num_spks=10)
    emb = D.embedding_sets()["three"][0]
    np.random.seed(0)
    assert len(set(c(emb.copy(), 2).tolist())) == 2
    s = c._get_spectral_cluster()
    assert (s.min_num_spks, s.max_num_spks, s.pval) == (2, 10, 0.06) and c.merge_thr == 0.90        # the oracle count did not stick
    np.random.seed(0)
    assert len(set(c(emb.copy()).tolist())) == 3
    assert (SpectralCluster().min_num_spks, SpectralCluster().max_num_spks) == (1, 15)


def test_pruning_and_laplacian_work_in_place_as_the_reference_does():
    sc = SpectralCluster(pval=0.5)
    a = np.random.default_rng(1).uniform(0.1, 1.0, (20, 20))
    out = sc.p_pruning(a)
    assert out is a and (np.count_nonzero(a, axis=1) == 10).all()
    sym = 0.5 * (a + a.T)
    lap = sc.get_laplacian(sym)
    assert (np.diag(sym) == 0).all() and np.allclose(lap.sum(1), 0) and np.allclose(np.diag(lap), sym.sum(1))
    assert sc.get_eigen_gaps(np.array([0.0, 1.0, 4.0])).tolist() == [1.0, 3.0]


def test_hysteresis(gold):
    for name, segs in D.hysteresis_cases().items():
        assert L._apply_vad_hysteresis(segs) == gold["hysteresis"][name], name
    assert len(gold["hysteresis"]["mixed"]) == 4 and gold["hysteresis"]["single_short"] == []


class MarkerModel:
    def encode_batch(self, wavs):
        assert wavs.shape == (1, 12000)
        return torch.zeros(1, 1, 4) if float(wavs[0, 0]) == 0.5 else torch.ones(1, 1, 4)


class Recorder:
    """Stands in for EcapaTdnnMI355X: records the one embed_windows call and answers like MarkerModel."""

    def __init__(self):
        self.calls = []

    def embed_windows(self, audio, starts, lengths, window_samples):
        self.calls.append((np.array(audio), list(starts), list(lengths), window_samples))
        return torch.stack([torch.zeros(4) if audio[s] == 0.5 else torch.ones(4) for s in starts])


def _window_audio():
    audio = np.zeros(D.WINDOW_CASE_AUDIO, np.float32)
    audio[D.DROPPED_WINDOW_START] = 0.5
    return audio


def test_window_positions_and_the_embedding_filter(gold):
    want = gold["windows"]
    emb, wins = L._extract_embeddings(_window_audio(), copy.deepcopy(D.window_cases()), 16000, speaker_model=MarkerModel())
    assert wins == want["segments"] and np.asarray(emb).tolist() == want["embeddings"] and len(wins) == 25
    window, spans = L._window_positions(D.window_cases(), 16000)
    assert window == 12000 and len(spans) == 26                                    # one window (the marker's) is dropped by the filter
    assert spans[0] == (0, 7000) and spans[1] == (20000, 32000) and spans[2] == (40000, 52000)
    assert [s for s in spans if 60000 <= s[0] < 90000] == [(60000, 72000), (62400, 74400)]                       # remainder 1200: no tail
    assert [s for s in spans if 90000 <= s[0] < 120000] == [(90000, 102000), (92400, 104400), (93601, 105601)]   # remainder 1201: a tail
    assert L._extract_embeddings(_window_audio(), [], 16000, speaker_model=MarkerModel()) == (pytest.approx(np.array([])), [])


def test_device_path_sends_every_window_in_one_call(gold):
    rec = Recorder()
    emb, wins = L._extract_embeddings(_window_audio(), copy.deepcopy(D.window_cases()), 16000, speaker_model=rec)
    assert wins == gold["windows"]["segments"] and np.asarray(emb).tolist() == gold["windows"]["embeddings"]
    assert len(rec.calls) == 1
    audio, starts, lengths, window = rec.calls[0]
    assert window == 12000 and len(starts) == 26 and len(audio) == D.WINDOW_CASE_AUDIO       # 7000 >= pad + 1 = 5001: reflected on the device
    assert (starts[0], lengths[0]) == (0, 7000) and lengths[1:] == [12000] * 25
    # a chunk too short for one reflection (np.pad reflects repeatedly) is padded on the host and rides behind the audio
    short = [{"start": 0.0, "end": 0.25, "start_sample": 0, "end_sample": 4000}, {"start": 1.0, "end": 1.75, "start_sample": 16000, "end_sample": 28000}]
    ramp = np.arange(30000, dtype=np.float32)
    rec = Recorder()
    L._extract_embeddings(ramp, short, 16000, speaker_model=rec)
    audio, starts, lengths, window = rec.calls[0]
    assert starts == [30000, 16000] and lengths == [12000, 12000] and len(audio) == 42000
    assert np.array_equal(audio[30000:], np.pad(ramp[:4000], (0, 8000), mode="reflect"))
    # a segment that runs past the end of the audio is cut there, as the reference's slice is
    rec = Recorder()
    L._extract_embeddings(ramp, [{"start": 1.2, "end": 1.95, "start_sample": 19200, "end_sample": 31200}], 16000, speaker_model=rec)
    assert rec.calls[0][1:3] == ([19200], [10800])
    with pytest.raises(ValueError):
        L._extract_embeddings(ramp, [{"start": 2.0, "end": 2.5, "start_sample": 32000, "end_sample": 40000}], 16000, speaker_model=Recorder())


def test_resample_vad(gold):
    for name, (frames, n) in D.resample_vad_cases().items():
        got = L._resample_vad(list(frames), n)
        assert got.dtype == bool and got.tolist() == gold["resample_vad"][name], name


def test_postprocess_merge_and_words(gold):
    for name, (w, lb, dur, vad) in D.postprocess_cases().items():
        assert L._postprocess_segments(copy.deepcopy(w), np.asarray(lb), dur, list(vad)) == gold["postprocess"][name], name
    for name, segs in D.merge_cases().items():
        assert L._merge_short_segments(copy.deepcopy(segs)) == gold["merge"][name], name
    for name, (w, s) in D.word_cases().items():
        got = SpeakerDiarizer.assign_speakers_to_words(copy.deepcopy(w), copy.deepcopy(s))
        assert got == gold["words"][name], name
    assert [w["speaker"] for w in gold["words"]["no_segments"]] == [None, None]
    assert gold["postprocess"]["no_windows"] == [] and gold["postprocess"]["no_vad"] == []


def test_whole_run_equals_the_reference(gold):
    """The same CPU torch modules behind ``encode_batch`` and the same VAD decisions as the generator gave the reference."""
    audio, enc = D.run_audio(), D.TorchEncoder(D.GEOM, D.run_weights())
    segs, frames = L._get_speech_segments(audio, 16000, vad=D.ReplayVad(D.run_speech_frames()))
    assert frames == D.run_speech_frames() and segs == gold["run"]["vad_segments"]
    segs2, _ = L._get_speech_segments(audio, 16000, speech_frames=D.run_speech_frames())
    assert segs2 == segs
    np.random.seed(D.NUMPY_SEED)
    got = L.diarize(audio, speaker_model=enc, vad=D.ReplayVad(D.run_speech_frames()))
    assert got == gold["run"]["segments"]
    np.random.seed(D.NUMPY_SEED)
    assert SpeakerDiarizer.diarize(audio, num_speakers=2, speaker_model=enc, speech_frames=D.run_speech_frames()) == gold["run_oracle_two"]
    assert {s["speaker"] for s in got} == {"SPEAKER_0", "SPEAKER_1"} and len(got) == 4
    assert L.diarize(audio, speaker_model=enc, speech_frames=[False] * len(frames)) == []


# ----------------------------------------------------------------------------- the reference's own assertions, restated
def test_similarity_of_identical_and_orthogonal_rows():
    sc = SpectralCluster()
    sim = sc.get_sim_mat(np.array([[1.0, 0.0], [1.0, 0.0]]))
    assert sim.shape == (2, 2)
    np.testing.assert_allclose(sim, np.ones((2, 2)), atol=1e-6)
    sim = sc.get_sim_mat(np.array([[1.0, 0.0], [0.0, 1.0]]))
    assert sim[0, 0] == pytest.approx(1.0) and sim[1, 1] == pytest.approx(1.0) and sim[0, 1] == pytest.approx(0.0)


def test_pruning_keeps_the_top_k_of_every_row():
    n, pval = 20, 0.5
    sc = SpectralCluster(pval=pval)
    rng = np.random.default_rng(7)
    affinity = np.zeros((n, n))
    for i in range(n):
        vals = rng.uniform(0.0, 0.4, size=n)
        vals[rng.choice(n, size=10, replace=False)] = rng.uniform(0.7, 1.0, size=10)
        affinity[i] = vals
    pruned = sc.p_pruning(affinity.copy())
    k = max(1, int(max(pval, 6.0 / n) * n))
    assert k == 10 and all(int(np.sum(row > 0)) == k for row in pruned)


def test_two_distinct_clusters_and_a_single_oracle_cluster():
    rng = np.random.default_rng(42)
    emb = np.vstack([rng.normal(loc=[1.0, 1.0, 0.0, 0.0], scale=0.05, size=(5, 4)), rng.normal(loc=[0.0, 0.0, 1.0, 1.0], scale=0.05, size=(5, 4))])
    labels = SpectralCluster(min_num_spks=1, max_num_spks=4)(emb, oracle_num=2)
    assert labels.shape == (10,) and len(set(labels.tolist())) == 2
    assert len(set(labels[:5].tolist())) == 1 and len(set(labels[5:].tolist())) == 1 and labels[0] != labels[5]
    labels = SpectralCluster()(np.random.default_rng(0).normal(size=(8, 4)), oracle_num=1)
    assert len(set(labels.tolist())) == 1


def test_device_helper_and_constants():
    assert isinstance(L._get_device(), torch.device) and L._get_device().type in ("cuda", "cpu")
    assert (L.WINDOW_SIZE, L.STEP_SIZE, L.TAIL_COVERAGE_RATIO) == (0.75, 0.15, 0.1)
    assert (L.VAD_THRESHOLD, L.VAD_MIN_DURATION, L.VAD_MAX_GAP, L.VAD_PAD_ONSET, L.VAD_PAD_OFFSET) == (0.25, 0.05, 0.50, 0.05, 0.05)
    assert (L.VOTING_RATE, L.MIN_SEGMENT_DURATION, L.SHORT_SEGMENT_GAP, L.SAME_SPEAKER_GAP) == (0.01, 0.15, 0.1, 0.5)
    import inspect
    p = inspect.signature(L.diarize).parameters
    assert list(p)[:5] == ["audio", "sample_rate", "num_speakers", "min_speakers", "max_speakers"]
    assert (p["sample_rate"].default, p["min_speakers"].default, p["max_speakers"].default) == (16000, 2, 10)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("speaker_model", "speech_frames", "vad"))
    import tiny_audio_amd
    assert tiny_audio_amd.SpeakerDiarizer is SpeakerDiarizer and tiny_audio_amd.LocalSpeakerDiarizer is L
    assert tiny_audio_amd.SpectralCluster is SpectralCluster and tiny_audio_amd.SpeakerClusterer is SpeakerClusterer


# ----------------------------------------------------------------------------- what is not installed
def _absent(monkeypatch, name):
    for k in [k for k in sys.modules if k == name or k.startswith(name + ".")]:
        monkeypatch.delitem(sys.modules, k)
    monkeypatch.setitem(sys.modules, name, None)                    # import of a None entry raises ImportError


def test_import_errors(monkeypatch):
    audio = D.run_audio()[:32000]
    _absent(monkeypatch, "ten_vad")
    with pytest.raises(ImportError):
        L.diarize(audio, speaker_model=MarkerModel())
    _absent(monkeypatch, "speechbrain")
    with pytest.raises(ImportError):
        L.diarize(audio, speech_frames=[True] * 124)
    _absent(monkeypatch, "librosa")
    with pytest.raises(ImportError):
        L.diarize("speech.wav", speech_frames=[True] * 124, speaker_model=MarkerModel())
    with pytest.raises(ImportError):
        L.diarize(audio, sample_rate=8000, speech_frames=[True] * 124, speaker_model=MarkerModel())
    assert M.VAD_HOP == 256

"""-m gpu: the speaker-turn kernels (csrc/speaker_post.hip: ``spk_vote``, ``spk_merge``, ``spk_words``) against the host functions of
``tiny_audio_amd/diarization.py`` and their integer-frame restatement (tests/speaker_post_ref.py), and through the diarizer and
``ASRModel.transcribe_long(return_speakers=True)`` end to end.  Every comparison is ``==``: integers, or lists of dicts and so every
float.  tests/test_speaker_post_ref.py shows that the sweeps of (2) and (3) tell the float64 evaluation order from an integer shortcut,
a fused multiply-add and an integer VAD index."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import speaker_post_ref as P
from tests.golden import diarization_recipe as D
from tiny_audio_amd.diarization import LocalSpeakerDiarizer as L

DEV = "cuda"
OPT = P.OPTIONS
FIXTURE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "diarization.json")))
POISON = -77


def _ops():
    from tiny_audio_amd import ops
    return ops


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _cu(counts):
    return _i32(np.concatenate([[0], np.cumsum(counts)]))


def _capacity(rec):
    v = np.asarray(rec["vad"], bool)
    return min(2 * len(rec["first"]) + int(np.count_nonzero(v[1:] != v[:-1])) + 2, rec["n_frames"])


def vote(recs, S, options=OPT, caps=None):
    """recs: dicts of first / last / label / n_frames / vad -> (runs per recording, the raw poisoned buffers, n_runs, status, caps)."""
    ops = _ops()
    caps = [_capacity(r) for r in recs] if caps is None else caps
    ld = max(1, max(len(r["vad"]) for r in recs))
    flags = np.zeros((len(recs), ld), np.uint8)
    for k, r in enumerate(recs):
        flags[k, :len(r["vad"])] = np.asarray(r["vad"], np.uint8)
    cat = lambda key: np.concatenate([np.asarray(r[key], np.int64) for r in recs]) if recs else np.zeros(0)  # noqa: E731
    out = tuple(torch.full((sum(caps),), POISON, dtype=torch.int32, device=DEV) for _ in range(3))
    res = ops.spk_vote(_i32(cat("first")), _i32(cat("last")), _i32(cat("label")), _cu([len(r["first"]) for r in recs]), S,
                       _i32([r["n_frames"] for r in recs]), max(r["n_frames"] for r in recs), torch.from_numpy(flags).to(DEV),
                       _i32([len(r["vad"]) for r in recs]), _cu(caps), options, out=out)
    torch.cuda.synchronize()
    spk, f0, f1, n_runs, status = (t.cpu().numpy() for t in res)
    o = np.concatenate([[0], np.cumsum(caps)])
    runs = [list(zip(spk[o[k]:o[k] + n_runs[k]].tolist(), f0[o[k]:o[k] + n_runs[k]].tolist(), f1[o[k]:o[k] + n_runs[k]].tolist()))
            for k in range(len(recs))]
    return runs, (spk, f0, f1), n_runs, status, caps


def merge(run_lists, options=OPT):
    """run lists per recording -> (turns per recording, the raw poisoned buffers, n_seg)."""
    ops = _ops()
    flat = np.array([t for rl in run_lists for t in rl], np.int64).reshape(-1, 3)
    counts = [len(rl) for rl in run_lists]
    out = tuple(torch.full((len(flat),), POISON, dtype=torch.int32, device=DEV) for _ in range(3))
    res = ops.spk_merge(_i32(flat[:, 0]), _i32(flat[:, 1]), _i32(flat[:, 2]), _cu(counts), options, out=out)
    torch.cuda.synchronize()
    spk, f0, f1, n_seg = (t.cpu().numpy() for t in res)
    o = np.concatenate([[0], np.cumsum(counts)])
    turns = [list(zip(spk[o[k]:o[k] + n_seg[k]].tolist(), f0[o[k]:o[k] + n_seg[k]].tolist(), f1[o[k]:o[k] + n_seg[k]].tolist()))
             for k in range(len(run_lists))]
    return turns, (spk, f0, f1), n_seg


def want_runs(rec, S):
    return P.runs(P.owners(rec["first"], rec["last"], rec["label"], S, rec["n_frames"], rec["vad"]))


def rec(first, last, label, n_frames, vad):
    return dict(first=list(first), last=list(last), label=list(label), n_frames=int(n_frames), vad=list(vad))


# ============================================================================ (1) the fixture's cases
def test_fixture_cases_exactly():
    for name, case in D.postprocess_cases().items():
        assert L._postprocess_segments(*case, device=DEV) == FIXTURE["postprocess"][name], name
    for name, segs in D.merge_cases().items():
        assert L._merge_short_segments(copy.deepcopy(segs), device=DEV) == FIXTURE["merge"][name], name
    for name, (words, segs) in D.word_cases().items():
        assert L.assign_speakers_to_words(copy.deepcopy(words), segs, device=DEV) == FIXTURE["words"][name], name
    # all the postprocess cases as one ragged batch: one launch each
    cases = D.postprocess_cases()
    assert L.postprocess_batch(list(cases.values()), DEV) == [FIXTURE["postprocess"][n] for n in cases]


# ============================================================================ (2) the merge arithmetic
def test_merge_sweep_equals_the_host_function():
    """f0 in [0, 4096) x six gaps x nine lengths, 64 recordings in one launch: 221 184 patterns, every comparison of the rule at every
    position of the grid.  Each recording's turns equal ``_merge_short_segments`` on the same runs as dicts."""
    sweep = P.merge_sweep()
    assert len(sweep) == 64 and sum(len(r) for r in sweep) == 4096 * 54 * 3
    turns, _, n_seg = merge(sweep)
    for k, (rl, got) in enumerate(zip(sweep, turns)):
        want = L._merge_short_segments(P.to_dicts(rl))
        assert P.to_dicts(got) == want, (k, len(got), len(want))
        assert n_seg[k] == len(want) < len(rl)


def test_merge_further_cases():
    cases = [
        [(0, 0, 9), (0, 12, 60)],                                           # a first run that is short: dropped, nothing to extend
        [(0, 0, 100), (0, 120, 125), (0, 140, 300)],                        # short between two turns of one speaker, outer gap 0.4 s
        [(0, 0, 100), (0, 109, 114), (0, 160, 300)],                        # ... absorbed (gap 0.09 s), then the outer gap is 0.46 s
        [(0, 0, 100), (0, 130, 135), (0, 155, 300)],                        # ... dropped (gap 0.3 s), outer gap 0.55 s: two turns
        [(0, 0, 100), (0, 103, 108), (0, 170, 300)],                        # ... absorbed, and now 0.62 s: two turns
        [(0, 0, 100), (1, 100, 105), (0, 105, 300)],                        # a short run of another speaker: dropped, 0 joins across it
        [(0, 0, 100), (1, 100, 105), (1, 108, 200), (0, 200, 214)],         # a short run without a kept turn of its own, then a long one
        [],
        [(3, 5, 6)],
        [(2, 0, 10 ** 6), (2, 10 ** 6 + 49, 10 ** 6 + 64)],                  # at the far end of the grid
    ]
    turns, raw, n_seg = merge(cases)
    for rl, got in zip(cases, turns):
        assert P.to_dicts(got) == L._merge_short_segments(P.to_dicts(rl)), rl
    o = np.concatenate([[0], np.cumsum([len(c) for c in cases])])
    for k in range(len(cases)):                                              # beyond n_seg the buffers keep their poison
        for buf in raw:
            assert (buf[o[k] + n_seg[k]:o[k + 1]] == POISON).all()
    # other thresholds: a subclass's constants are honoured
    class Coarse(L):
        MIN_SEGMENT_DURATION = 0.3
        SHORT_SEGMENT_GAP = 0.2
        SAME_SPEAKER_GAP = 1.0

    rl = [(0, 0, 100), (0, 119, 140), (0, 230, 300), (1, 300, 329), (1, 340, 400)]
    got = merge([rl], Coarse.spk_options())[0][0]
    assert P.to_dicts(got) == Coarse._merge_short_segments(P.to_dicts(rl)) != L._merge_short_segments(P.to_dicts(rl))


# ============================================================================ (3) the VAD index
def test_vad_index_is_the_float64_expression():
    n = 65536
    alt = (np.arange(40960) % 2 == 0)
    one = rec([0], [n], [0], n, alt)
    recs = [one, dict(one, vad=[]), dict(one, vad=[True]), dict(one, vad=[False]), dict(one, vad=alt[:1001].tolist()),
            dict(one, vad=(np.arange(30000) % 3 != 0).tolist())]
    caps = [n] * len(recs)
    runs, _, n_runs, status, _ = vote(recs, 1, caps=caps)
    assert not status.any()
    for k, r in enumerate(recs):
        assert runs[k] == want_runs(r, 1), k
    assert n_runs[0] == 40960 // 2 and max(b - a for _, a, b in runs[0]) <= 2, "alternating decisions: a run of one or two frames per speech decision"
    assert runs[1] == [] and runs[2] == [(0, 0, n)] and runs[3] == []
    assert runs[4][-1][2] == n, "beyond a short VAD the index clips to its last decision (speech)"
    assert L._merge_short_segments(P.to_dicts(runs[0])) == [], "(every run is short: the merged result would be empty)"


# ============================================================================ (4) voting
def test_voting_edges():
    T = _ops().SPK_FRAME_TILE
    rng = np.random.default_rng(5)
    recs, Ss = [], []
    for n in (1, 2, T, T + 1, 2 * T + 1):
        ones = [True] * (n * 5 // 8 + 2)
        recs += [rec([0], [n], [0], n, ones),                                                    # one run that ends at n_frames
                 rec([0, 0], [n, n], [1, 0], n, ones),                                           # a tie: the lowest index
                 rec([n - 1, 0, n // 2, n // 2, n, n + 5, 0], [n + 9, n // 2, n // 2, n // 3, n + 3, n + 9, 1], [1, 0, 1, 0, 1, 0, 1], n, ones)]
    for r in recs:
        assert want_runs(r, 2) == vote([r], 2)[0][0], r["n_frames"]
    # windows out of order, overlapping, empty; S = 1 and S = 16 (the owner is the arg-max over all sixteen)
    n = 2 * T + 37
    first = rng.integers(0, n, 200)
    length = rng.choice([0, 1, 3, 40, 75, 300], 200)
    vad = np.repeat(rng.random(n // 40 + 2) < 0.8, 25)[:n * 5 // 8 + 1]
    for S in (1, 2, 16):
        r = rec(first, first + length, rng.integers(0, S, 200), n, vad)
        runs, raw, n_runs, status, caps = vote([r], S)
        assert runs[0] == want_runs(r, S) and status[0] == 0 and len(runs[0]) > 10
        assert all((buf[n_runs[0]:] == POISON).all() for buf in raw)
    # ties among many: speaker 3 and speaker 11 with equal counts, speaker 15 with fewer
    r = rec([0, 0, 5, 5, 9], [50, 50, 50, 50, 40], [11, 3, 3, 11, 15], 60, [True] * 40)
    assert vote([r], 16)[0][0] == want_runs(r, 16) == [(3, 0, 50)]
    # a capacity that is too small: status 1, the first runs that fit, nothing beyond
    r = rec([0, 10, 20, 30], [5, 15, 25, 35], [0, 0, 0, 0], 40, [True] * 30)
    runs, raw, n_runs, status, _ = vote([r], 1, caps=[3])
    assert status[0] == 1 and n_runs[0] == 3 and runs[0] == want_runs(r, 1)[:3] and len(raw[0]) == 3


# ============================================================================ (5) a ragged batch
def test_ragged_batch_alone_twice_and_poison():
    T = _ops().SPK_FRAME_TILE
    rng = np.random.default_rng(9)

    def rnd(n, nw, S=3):
        first = rng.integers(0, max(n, 1), nw)
        return rec(first, first + rng.choice([0, 2, 30, 75, 200], nw), rng.integers(0, S, nw), n,
                   np.repeat(rng.random(n // 30 + 2) < 0.75, 19)[:n * 5 // 8 + 1])

    recs = [rnd(3 * T + 5, 150), rec([], [], [], 500, [True] * 300), dict(rnd(700, 40), vad=[]), rnd(1, 3), rnd(T, 60), rnd(2 * T + 1, 90)]
    runs, raw, n_runs, status, caps = vote(recs, 3)
    again = vote(recs, 3)
    assert not status.any() and all(np.array_equal(a, b) for a, b in zip(raw, again[1])) and np.array_equal(n_runs, again[2])
    o = np.concatenate([[0], np.cumsum(caps)])
    for k, r in enumerate(recs):
        alone = vote([r], 3)
        assert alone[0][0] == runs[k] == want_runs(r, 3), k
        for buf in raw:
            assert (buf[o[k] + n_runs[k]:o[k + 1]] == POISON).all(), k
    assert runs[1] == [] and runs[2] == [] and sum(map(len, runs)) > 60
    # the same batch through merge: alone == in the batch == the host function, poison beyond n_seg
    turns, mraw, n_seg = merge(runs)
    assert all(np.array_equal(a, b) for a, b in zip(mraw, merge(runs)[1]))
    o = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    for k, rl in enumerate(runs):
        assert merge([rl])[0][0] == turns[k] and P.to_dicts(turns[k]) == L._merge_short_segments(P.to_dicts(rl))
        for buf in mraw:
            assert (buf[o[k] + n_seg[k]:o[k + 1]] == POISON).all()
    # and vote -> merge without a visit to the host: n_runs and cu_cap go in as they are
    ops = _ops()
    dev = lambda a: _i32(a)  # noqa: E731
    res = ops.spk_merge(dev(raw[0]), dev(raw[1]), dev(raw[2]), _cu(caps), OPT, n_run=dev(n_runs))
    spk, f0, f1, n2 = (t.cpu().numpy() for t in res)
    oc = np.concatenate([[0], np.cumsum(caps)])
    for k in range(len(recs)):
        assert n2[k] == n_seg[k] and list(zip(spk[oc[k]:oc[k] + n2[k]].tolist(), f0[oc[k]:oc[k] + n2[k]].tolist(),
                                              f1[oc[k]:oc[k] + n2[k]].tolist())) == turns[k]


# ============================================================================ (6) words
def _segments(rng, G):
    """Overlapping segments on a 0.5 s lattice (shared boundaries, equal midpoints), in no order."""
    a = rng.integers(0, 80, G) * 0.5
    return [{"speaker": f"SPEAKER_{int(k)}", "start": float(s), "end": float(s + w)}
            for s, w, k in zip(a, rng.choice([0.0, 0.5, 1.0, 3.0], G), rng.integers(0, 4, G))]


def _words(rng, W=300):
    """Midpoints on a 0.25 s lattice: many lie exactly on a boundary two segments share, or halfway between two segment midpoints;
    some lie outside everything."""
    mid = rng.integers(-20, 200, W) * 0.25
    half = rng.choice([0.0, 0.125, 0.25], W)
    return [{"word": f"w{i}", "start": float(m - h), "end": float(m + h)} for i, (m, h) in enumerate(zip(mid, half))]


def test_words_equal_the_host_function():
    Gt = _ops().SPK_SEG_TILE
    rng = np.random.default_rng(3)
    items = [(_words(rng), _segments(rng, G)) for G in (0, 1, Gt, Gt + 1, 2 * Gt + 3)]
    # boundaries shared by two segments, and a word equidistant from two segment midpoints, by hand
    segs = [{"speaker": "SPEAKER_1", "start": 2.0, "end": 3.0}, {"speaker": "SPEAKER_0", "start": 1.0, "end": 2.0},
            {"speaker": "SPEAKER_2", "start": 4.0, "end": 5.0}, {"speaker": "SPEAKER_3", "start": 6.0, "end": 7.0}]
    words = [{"word": "shared", "start": 1.9, "end": 2.1}, {"word": "between", "start": 5.4, "end": 5.6}, {"word": "before", "start": -3.0, "end": -2.0},
             {"word": "after", "start": 50.0, "end": 51.0}, {"word": "inside", "start": 4.2, "end": 4.4}]
    items.append((words, segs))
    want = [L.assign_speakers_to_words(copy.deepcopy(w), s) for w, s in items]
    assert [w["speaker"] for w in want[-1]] == ["SPEAKER_1", "SPEAKER_2", "SPEAKER_0", "SPEAKER_3", "SPEAKER_2"]
    for (w, s), ref in zip(items, want):                                     # each recording alone
        assert L.assign_speakers_to_words(copy.deepcopy(w), s, device=DEV) == ref, len(s)
    got = L.assign_speakers_batch([(copy.deepcopy(w), s) for w, s in items], DEV)      # recordings with different G in one call
    assert got == want
    contained = sum(any(s["start"] <= (w["start"] + w["end"]) / 2 <= s["end"] for s in items[2][1]) for w in items[2][0])
    assert 30 < contained < 300, "both rules are exercised"
    # the indices themselves, twice, with poison behind them
    ops = _ops()
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=DEV)  # noqa: E731
    w, s = items[4]
    args = (f64([x["start"] for x in w]), f64([x["end"] for x in w]), _cu([len(w)]), f64([x["start"] for x in s]), f64([x["end"] for x in s]), _cu([len(s)]))
    out = torch.full((len(w) + 7,), POISON, dtype=torch.int32, device=DEV)
    a = ops.spk_words(*args, out=out).cpu().numpy().copy()
    b = ops.spk_words(*args).cpu().numpy()
    assert a[:len(w)].tolist() == b.tolist() == P.words(*[[x[k] for x in seq] for seq in (w, s) for k in ("start", "end")]) and (a[len(w):] == POISON).all()


# ============================================================================ (7) through the diarizer
@pytest.fixture(scope="module")
def ecapa():
    from tests.golden import ecapa_recipe as ER
    from tiny_audio_amd import ecapa as E
    return E.EcapaTdnnMI355X(E.EcapaConfig(**ER.GEOMS["a"]), device=DEV).random_init(0)


def test_through_the_diarizer(ecapa):
    audio, frames = D.run_audio(), D.run_speech_frames()

    def run(fn, *a, **kw):
        np.random.seed(D.NUMPY_SEED)                                         # scikit-learn's k_means draws from the global state
        return fn(*a, speaker_model=ecapa, **kw)

    host = run(L.diarize, audio, speech_frames=frames)
    assert host, "the recording must give turns"
    assert run(L.diarize, audio, speech_frames=frames, post_device=DEV) == host
    short = audio[:int(1.2 * 16000)]
    short_frames = frames[:len(range(0, len(short) - 256, 256))]
    host_short = run(L.diarize, short, speech_frames=short_frames)
    assert host_short and run(L.diarize, short, speech_frames=short_frames, post_device=DEV) == host_short
    assert run(L.diarize_batch, [audio, short], speech_frames=[frames, short_frames], post_device=DEV) == [host, host_short]
    assert run(L.diarize_batch, [audio, short], speech_frames=[frames, short_frames]) == [host, host_short]
    # with a DeviceVAD the decisions stay on the device: the same turns as with its decisions handed over as a list
    from tests import vad_ref as VR
    from tiny_audio_amd.vad import DeviceVAD
    x = VR.synth(5, 12.0, 20, "white")[0]
    vad = DeviceVAD()
    want = run(L.diarize, x, speech_frames=vad.speech_frames(x))
    assert want and run(L.diarize, x, vad=vad, post_device=DEV) == want


# ============================================================================ (8) through long form
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


def test_through_long_form(model, ecapa, monkeypatch):
    from tests import vad_ref as VR
    from tiny_audio_amd import wav2vec2 as W
    from tiny_audio_amd.vad import DeviceVAD
    am = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(hidden_size=256, num_attention_heads=4, intermediate_size=512, conv_dim=128,
                                                 num_hidden_layers=1), device=DEV).random_init(0)
    x = VR.synth(5, 12.0, 20, "white")[0]
    quiet = (1e-4 * np.random.default_rng(1).standard_normal(40000)).astype(np.float32)          # a recording without speech
    captured = []
    real = L.postprocess_batch.__func__

    def spy(cls, items, device, **kw):
        captured.append(copy.deepcopy(items))
        return real(cls, items, device, **kw)

    monkeypatch.setattr(L, "postprocess_batch", classmethod(spy))
    kw = dict(max_window_s=4.0, min_window_s=1.0, max_new_tokens=5, vad=DeviceVAD(), acoustic_model=am)
    np.random.seed(D.NUMPY_SEED)
    res = model.transcribe_long([x, quiet], speaker_model=ecapa, return_speakers=True, **kw)
    plain = model.transcribe_long([x, quiet], return_timestamps=True, **kw)
    assert len(captured) == 1 and len(captured[0]) == 2, "one voting call for both recordings"
    for r, p, item in zip(res, plain, captured[0]):
        assert set(r) == {"text", "chunks", "words", "speaker_segments"} and set(p) == {"text", "chunks", "words"}
        assert r["text"] == p["text"] and r["chunks"] == p["chunks"]
        assert [{k: v for k, v in w.items() if k != "speaker"} for w in r["words"]] == p["words"]
        assert r["speaker_segments"] == L._postprocess_segments(*item), "the host function on the windows and labels of that call"
        stripped = [{k: v for k, v in w.items() if k != "speaker"} for w in r["words"]]
        assert r["words"] == L.assign_speakers_to_words(stripped, r["speaker_segments"])
    assert res[0]["speaker_segments"] and res[0]["words"] and all(w["speaker"] is not None for w in res[0]["words"])
    assert res[1]["speaker_segments"] == [] and all(w["speaker"] is None for w in res[1]["words"])

"""-m "not gpu": tests/speaker_post_ref.py (the speaker-turn stage in integer frames, which tests/test_gpu_speaker_post.py holds the
kernels to) against the host functions of ``tiny_audio_amd/diarization.py`` and the reference-generated fixture
tests/golden/diarization.json -- and the proof that the sweeps the GPU tests run can tell the float64 evaluation order from its
look-alikes: an integer shortcut, a fused multiply-add, an integer VAD index."""
import copy
import json
import os

import numpy as np

from tests import speaker_post_ref as P
from tests.golden import diarization_recipe as D
from tiny_audio_amd.diarization import LocalSpeakerDiarizer as L

FIXTURE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "diarization.json")))
RATE, _, MIN_SEG, SHORT_GAP, SAME_GAP = P.OPTIONS


def _merge_dicts(segments):
    triples, names = P.snap(segments)
    return P.to_dicts(P.merge(triples), names)


def _assign(words, segs):
    idx = P.words([w["start"] for w in words], [w["end"] for w in words], [s["start"] for s in segs], [s["end"] for s in segs])
    return [dict(w, speaker=segs[g]["speaker"] if g >= 0 else None) for w, g in zip(words, idx)]


def test_the_restatement_equals_the_host_functions_on_the_fixture_cases():
    for name, case in D.postprocess_cases().items():
        assert P.postprocess(*case) == L._postprocess_segments(*case) == FIXTURE["postprocess"][name], name
    for name, segs in D.merge_cases().items():
        assert _merge_dicts(segs) == L._merge_short_segments(copy.deepcopy(segs)) == FIXTURE["merge"][name], name
    for name, (words, segs) in D.word_cases().items():
        assert _assign(words, segs) == L.assign_speakers_to_words(copy.deepcopy(words), segs) == FIXTURE["words"][name], name
    for name, (frames, n) in D.resample_vad_cases().items():
        want = L._resample_vad(frames, n)
        got = np.asarray(frames, bool)[P.vad_index(n, len(frames))] if frames else np.zeros(n, bool)
        assert np.array_equal(got, want) and want.tolist() == FIXTURE["resample_vad"][name], name


def random_postprocess_case(rng):
    """Windows in any order (overlapping, empty, beyond the end), labels that are not 0 .. k - 1, a VAD with holes or none."""
    duration = float(rng.uniform(0.05, 12.0))
    n = int(rng.integers(1, 60))
    start = rng.uniform(0.0, duration + 0.5, n)
    wins = [{"start": float(a), "end": float(a + rng.choice([0.0, 0.004, 0.12, 0.75, 2.0]))} for a in start]
    labels = rng.choice(rng.choice(50, int(rng.integers(1, 6)), replace=False), n)
    n_vad = int(rng.choice([0, 1, int(duration / 0.016), int(duration / 0.016) + 7, max(1, int(duration / 0.032))]))
    vad = (np.repeat(rng.random(n_vad // 3 + 1) < 0.7, 3)[:n_vad]).tolist()
    return wins, labels, duration, vad


def random_runs(rng):
    """Runs in time order with gaps and lengths around the three thresholds, few speakers."""
    out, f = [], int(rng.integers(0, 5000))
    for _ in range(int(rng.integers(0, 40))):
        f += int(rng.choice([0, 1, 9, 10, 11, 30, 49, 50, 51, 80]))
        length = int(rng.choice([1, 5, 9, 10, 11, 14, 15, 16, 40, 200]))
        out.append((int(rng.integers(0, 3)), f, f + length))
        f += length
    return out


def random_words_case(rng):
    G, W = int(rng.integers(0, 12)), int(rng.integers(0, 30))
    s = np.round(rng.uniform(0, 20, G), 2)
    segs = [{"speaker": f"SPEAKER_{int(rng.integers(0, 3))}", "start": float(a), "end": float(a + rng.choice([0.0, 0.5, 1.0, 4.0]))} for a in s]
    a = np.round(rng.uniform(-1, 22, W), 2)
    return [{"word": "w", "start": float(x), "end": float(x + rng.choice([0.0, 0.1, 0.3, 1.0]))} for x in a], segs


def test_the_restatement_equals_the_host_functions_on_seeded_random_cases():
    rng = np.random.default_rng(7)
    seen_turns = 0
    for _ in range(300):
        case = random_postprocess_case(rng)
        got = P.postprocess(*case)
        assert got == L._postprocess_segments(*case)
        seen_turns += len(got)
    assert seen_turns > 300, "the random cases must produce turns"
    for _ in range(300):
        segs = P.to_dicts(random_runs(rng))
        assert _merge_dicts(segs) == L._merge_short_segments(copy.deepcopy(segs))
    for _ in range(300):
        words, segs = random_words_case(rng)
        assert _assign(words, segs) == L.assign_speakers_to_words(copy.deepcopy(words), segs)


def test_the_merge_sweep_of_the_gpu_test_equals_the_host_function():
    """The sweep itself, on a stride of the grid (the GPU test runs all of it against the host function): every recording's merged
    triples, as dicts, are what ``_merge_short_segments`` returns."""
    for rec in P.merge_sweep(range(0, 4096, 97), recordings=5):
        assert P.to_dicts(P.merge(rec)) == L._merge_short_segments(P.to_dicts(rec))


def _merge_with(run_list, less):
    """``speaker_post_ref.merge`` with the comparison ``b * r - a * r < t`` handed in as ``less(b, a, t)``."""
    out = []
    for spk, f0, f1 in run_list:
        short = less(f1, f0, MIN_SEG)
        near = SHORT_GAP if short else SAME_GAP
        if out and out[-1][0] == spk and less(f0, out[-1][2], near):
            out[-1] = (out[-1][0], out[-1][1], f1)
        elif not short:
            out.append((spk, f0, f1))
    return out


def test_the_sweeps_discriminate():
    """Conditions on the sweeps, not on any implementation: each look-alike of the float64 arithmetic decides differently from the host
    function on many of the swept cases, so a kernel that took it would fail tests/test_gpu_speaker_post.py.  A case is (f0, length);
    it disagrees when the turns of any of its six patterns (one per gap) differ from ``_merge_short_segments``'s."""
    import functools
    host = lambda b, a, t: b * RATE - a * RATE < t  # noqa: E731
    shortcut = lambda b, a, t: (b - a) * RATE < t  # noqa: E731
    fused = functools.lru_cache(maxsize=None)(lambda b, a, t: P.fma_less(b, a, RATE, t))
    patterns = [rec for rec in P.merge_sweep(recordings=4096 * len(P.SWEEP_GAPS) * len(P.SWEEP_LENGTHS))]
    assert len(patterns) == 4096 * 54 and all(len(p) == 3 for p in patterns)
    bad_shortcut, bad_fused = set(), set()
    for k, pat in enumerate(patterns):
        want = _merge_with(pat, host)
        if k % 61 == 0:
            assert P.to_dicts(want) == L._merge_short_segments(P.to_dicts(pat))       # the host function itself, on a stride
        f0, length = pat[0][1], pat[1][2] - pat[1][1]
        if _merge_with(pat, shortcut) != want:
            bad_shortcut.add((f0, length))
        if _merge_with(pat, fused) != want:
            bad_fused.add((f0, length))
    assert len(bad_shortcut) >= 1000, len(bad_shortcut)
    assert len(bad_fused) >= 1000, len(bad_fused)
    assert {n for _, n in bad_shortcut} >= {15} and {n for _, n in bad_fused} >= {15}
    # the VAD index: the integer shortcut f * 5 // 8 against _resample_vad's own arithmetic, read off an identity "VAD"
    n = 65536
    ident = L._resample_vad(list(range(1, 40961)), n) - 1          # decisions[at] with decisions = 1 .. n_vad: at itself
    assert np.array_equal(ident, P.vad_index(n, 40960))
    differ = int(np.count_nonzero(ident != np.minimum(np.arange(n) * 5 // 8, 40959)))
    assert differ >= 40, differ
    # and with alternating decisions every such frame flips the owner, which the run comparison of the GPU test sees
    alt = (np.arange(40960) % 2 == 0)
    assert int(np.count_nonzero(alt[ident] != alt[np.minimum(np.arange(n) * 5 // 8, 40959)])) >= 40

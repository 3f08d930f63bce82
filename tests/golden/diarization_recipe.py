"""The seeded and hand-made inputs of the diarization fixture (tests/golden/make_diarization_fixture.py) and of the tests that read it.
The fixture holds only what the reference's ``tiny_audio/diarization.py`` returned for them."""
import functools

import numpy as np

from tests.golden import ecapa_recipe as ER

NUMPY_SEED = 0                       # np.random.seed before every clusterer call: scikit-learn's k_means draws from the global state
GEOM = "a"                           # the ECAPA geometry of the whole-run case
SAMPLE_RATE = 16000


# ----------------------------------------------------------------------------- clusterer inputs
def embedding_sets():
    """name -> (embeddings [N, 192] float64, num_speakers argument): separated synthetic speakers (centroid + 0.35 noise), the
    oracle-count path, the fewer-than-six and 0 / 1 row edges, a NaN row."""
    rng = np.random.default_rng(0)
    out = {}
    for name, nspk, per in (("two", 2, 20), ("three", 3, 20), ("four", 4, 15)):
        cent = rng.standard_normal((nspk, 192))
        out[name] = (cent[np.repeat(np.arange(nspk), per)] + 0.35 * rng.standard_normal((nspk * per, 192)), None)
    out["oracle_three"] = (out["three"][0], 3)
    out["oracle_two_of_four"] = (out["four"][0], 2)
    out["five_rows"] = (out["two"][0][[0, 1, 20, 21, 22]], None)
    out["one_row"] = (out["two"][0][:1], None)
    out["zero_rows"] = (np.zeros((0, 192)), None)
    nan = out["two"][0].copy()
    nan[3] = np.nan
    nan[25, 7] = np.inf
    out["nan_row"] = (nan, None)
    return out


def partition(labels):
    """Labels as a partition: the sorted list of each cluster's row indices."""
    labels = np.asarray(labels)
    return sorted([int(i) for i in np.flatnonzero(labels == u)] for u in np.unique(labels))


# ----------------------------------------------------------------------------- helper inputs
def _seg(start, end):
    return {"start": start, "end": end, "start_sample": int(start * SAMPLE_RATE), "end_sample": int(end * SAMPLE_RATE)}


def hysteresis_cases():
    """Unsorted input; gaps under, at about and over VAD_MAX_GAP; a segment under VAD_MIN_DURATION that stays alone; one that starts
    inside the onset padding of 0; an empty list."""
    return {
        "empty": [],
        "mixed": [_seg(3.0, 3.4), _seg(0.016, 0.8), _seg(1.2, 1.9), _seg(2.4, 2.95), _seg(5.0, 5.032), _seg(6.2, 6.9), _seg(7.41, 8.0),
                  _seg(9.0, 9.048), _seg(9.06, 9.07)],
        "single_short": [_seg(1.0, 1.016)],
    }


def window_cases():
    """Segments for the window positions (16 kHz; window 12000, step 2400, tail rule at 1200 samples): shorter than a window, exactly
    one, one sample more, a remainder of exactly 1200 (no tail window) and of 1201 (one), an exact fit of the step grid, and a long one."""
    s = lambda a, n: {"start": a / SAMPLE_RATE, "end": (a + n) / SAMPLE_RATE, "start_sample": a, "end_sample": a + n}
    return [s(0, 7000), s(20000, 12000), s(40000, 12001), s(60000, 12000 + 2400 + 1200), s(90000, 12000 + 2400 + 1201),
            s(120000, 12000 + 4 * 2400), s(160000, 40000)]


WINDOW_CASE_AUDIO = 210000             # samples of the (silent but for a marker) audio behind window_cases()
DROPPED_WINDOW_START = 62400           # the stub model answers a window that starts here with a zero vector: the filter's branch


def resample_vad_cases():
    return {"empty": ([], 7), "short": ([True, False, True, True, False], 12), "long": ([i % 3 != 0 for i in range(40)], 50)}


def postprocess_cases():
    """(window segments, labels, total duration, vad frames): two speakers with a VAD hole; labels that are not 0 .. k - 1; a window
    past the end of the grid; no windows."""
    wins = [{"start": 0.15 * i, "end": 0.15 * i + 0.75} for i in range(40)]
    vad = [True] * 300 + [False] * 40 + [True] * 100
    return {
        "two_speakers": (wins, [0] * 20 + [1] * 20, 7.0, vad),
        "sparse_labels": (wins[:30], [7] * 8 + [3] * 10 + [7] * 4 + [9] * 8, 5.5, [True] * 400),
        "flicker": ([{"start": 0.1 * i, "end": 0.1 * i + 0.12} for i in range(30)], [0, 1] * 15, 3.2, [True] * 250),
        "past_the_end": ([{"start": 0.0, "end": 0.75}, {"start": 1.9, "end": 2.65}], [0, 1], 2.0, [True] * 200),
        "no_vad": (wins[:10], [0] * 10, 2.5, []),
        "no_windows": ([], [], 3.0, [True] * 100),
    }


def merge_cases():
    sp = lambda k, a, b: {"speaker": f"SPEAKER_{k}", "start": a, "end": b}
    return {
        "empty": [],
        "mixed": [sp(0, 0.0, 1.0), sp(0, 1.05, 1.1), sp(0, 1.3, 1.35), sp(1, 1.4, 1.45), sp(0, 1.7, 2.5), sp(1, 2.5, 3.0), sp(1, 3.6, 4.0),
                  sp(1, 4.05, 4.1), sp(0, 4.12, 4.2), sp(1, 4.2, 5.0)],
        "leading_short": [sp(2, 0.0, 0.1), sp(2, 0.12, 0.6)],
    }


def word_cases():
    segs = [{"speaker": "SPEAKER_0", "start": 0.0, "end": 1.0}, {"speaker": "SPEAKER_1", "start": 1.5, "end": 2.5},
            {"speaker": "SPEAKER_0", "start": 2.5, "end": 3.0}]
    words = [{"word": "in", "start": 0.2, "end": 0.4}, {"word": "edge", "start": 0.9, "end": 1.1}, {"word": "gap", "start": 1.1, "end": 1.3},
             {"word": "tie", "start": 1.2, "end": 1.3}, {"word": "shared", "start": 2.4, "end": 2.6}, {"word": "late", "start": 5.0, "end": 5.2}]
    return {"words": (words, segs), "no_segments": (words[:2], [])}


# ----------------------------------------------------------------------------- the whole run
# (speaker, from, to) in seconds.  The turns are 0.8 s of silence apart (more than VAD_MAX_GAP and the two paddings), so no window
# straddles two speakers and no label can hinge on how a half-and-half window rounds
TURNS = ((0, 0.0, 3.0), (1, 3.8, 7.0), (0, 7.8, 9.6), (1, 10.4, 12.0))
DURATION = 12.0


def speaker_signal(k, t, seed):
    """Speaker k on the time axis t.  The features lose every static spectral shape to the sentence-mean normalisation, so the two
    sources differ in their DYNAMICS, and fast enough that any 0.75 s window holds many periods and a speaker's windows embed alike:
    speaker 0 is a low harmonic stack under a 13 Hz amplitude modulation, speaker 1 a higher stack with a wide 8 Hz vibrato."""
    noise = 0.003 * np.random.default_rng(seed).standard_normal(len(t))
    if k == 0:
        phase = 2 * np.pi * 120.0 * t
        x = sum(np.sin((h + 1) * phase + h) / (h + 1) for h in range(8))
        return 0.15 * x * (0.6 + 0.4 * np.sin(2 * np.pi * 13.0 * t)) + noise
    phase = 2 * np.pi * 300.0 * t + 6.0 * np.sin(2 * np.pi * 8.0 * t)
    return 0.12 * sum(np.sin((h + 1) * phase + h) / (h + 1) for h in range(10)) + noise


@functools.lru_cache(maxsize=None)
def _run_audio():
    n = int(DURATION * SAMPLE_RATE)
    t = np.arange(n) / SAMPLE_RATE
    audio = 1e-4 * np.random.default_rng(99).standard_normal(n)
    for i, (k, a, b) in enumerate(TURNS):
        lo, hi = int(a * SAMPLE_RATE), int(b * SAMPLE_RATE)
        audio[lo:hi] += speaker_signal(k, t[lo:hi], 500 + i)
    return audio.astype(np.float32)


def run_audio():
    """About 12 s: two synthetic sources in turn with silent gaps between the turns."""
    return _run_audio().copy()


def run_speech_frames():
    """The stub VAD's decisions, one per 256 samples, for ``range(0, n - 256, 256)``: speech inside the turns."""
    n = int(DURATION * SAMPLE_RATE)
    mid = (np.arange(0, n - 256, 256) + 128) / SAMPLE_RATE
    return [bool(any(a <= m < b for _, a, b in TURNS)) for m in mid]


@functools.lru_cache(maxsize=None)
def _run_weights():
    """ecapa_recipe's drawn weights with asp_bn calibrated on windows of BOTH sources of the run (as training would have)."""
    from tests import ecapa_ref as REF
    sd = ER._draw(GEOM, 0)
    t = np.arange(12000) / SAMPLE_RATE
    wins = [speaker_signal(k, t + 0.3 * j, 900 + 10 * k + j).astype(np.float32) for k in (0, 1) for j in range(4)]
    pooled = np.stack([REF.forward(sd, REF.fbank(w), ER.DILATIONS)["pooled"] for w in wins])
    sd["asp_bn.norm.running_mean"] = pooled.mean(0).astype(np.float32)
    sd["asp_bn.norm.running_var"] = np.ones(pooled.shape[1], np.float32)       # (no whitening: it would amplify the within-speaker noise)
    return sd


def run_weights():
    return dict(_run_weights())


class ReplayVad:
    """TEN-VAD's ``process(frame) -> (probability, flag)`` replaying recorded decisions."""

    def __init__(self, frames):
        self.frames, self.i = list(frames), 0

    def process(self, frame):
        assert len(frame) == 256
        flag = self.frames[self.i]
        self.i += 1
        return (0.9 if flag else 0.1), flag


class TorchEncoder:
    """The recipe's CPU torch modules behind SpeechBrain's ``encode_batch(wavs [1, L]) -> [1, 1, D]``."""

    def __init__(self, geom, sd):
        self.model = ER.torch_model(geom, sd)

    def encode_batch(self, wavs):
        import torch
        with torch.no_grad():
            out = [self.model(ER.torch_fbank(w.numpy()).T[None])["emb"][0] for w in wavs]
        return torch.stack(out)[:, None, :]

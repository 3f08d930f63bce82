"""The speaker-turn stage in integer frames: what csrc/speaker_post.hip computes, restated in numpy and plain Python.

The definition is the host code of ``tiny_audio_amd/diarization.py`` (``_resample_vad``, ``_postprocess_segments``,
``_merge_short_segments``, ``assign_speakers_to_words``), which tests/test_diarization_host.py pins to reference-generated fixtures.  This
file says the same with frames instead of seconds -- every time the host functions put out is ``f * VOTING_RATE`` for an integer ``f``
-- so that the kernels' integer outputs can be compared without a detour through floats; tests/test_speaker_post_ref.py holds it to the
host functions.  The comparisons stay float64 in the order Python evaluates them: ``f1 * r - f0 * r`` is two products and a
difference, three roundings, and the VAD index is a product, a divide and a truncation.
"""
import numpy as np

from tiny_audio_amd.diarization import LocalSpeakerDiarizer

# (voting_rate, vad_frame_s, min_segment_s, short_gap_s, same_gap_s): ta_spk_post_options
OPTIONS = LocalSpeakerDiarizer.spk_options()


def vad_index(n_frames, n_vad, options=OPTIONS):
    """The VAD frame every voting frame reads, as ``_resample_vad`` computes it; int64 [n_frames]."""
    r, v = options[0], options[1]
    return np.clip(((np.arange(n_frames) * r) / v).astype(int), 0, n_vad - 1)


def owners(first, last, label, S, n_frames, vad, options=OPTIONS):
    """Windows [first, last) with labels in [0, S) -> the owner of every frame, int64 [n_frames]; -1 is silence.  ``vad``: the
    decisions, one per VAD frame; an empty one silences everything."""
    votes = np.zeros((n_frames, S), np.int64)
    for a, b, k in zip(first, last, label):
        a, b = int(a), min(int(b), n_frames)
        if a < b:
            votes[a:b, int(k)] += 1
    who = np.argmax(votes, axis=1)                           # the lowest index among the maxima
    who[votes.max(axis=1) == 0] = -1
    vad = np.asarray(vad, dtype=bool).reshape(-1)
    if len(vad) == 0:
        return np.full(n_frames, -1, np.int64)
    who[~vad[vad_index(n_frames, len(vad), options)]] = -1
    return who


def runs(owner):
    """Maximal stretches of one owner != -1 -> [(speaker, f0, f1)], f1 the first frame of the next owner or len(owner)."""
    out, current, since = [], -1, 0
    for f, who in enumerate(np.asarray(owner).tolist()):
        if who != current:
            if current != -1:
                out.append((current, since, f))
            current, since = who, f
    if current != -1:
        out.append((current, since, len(owner)))
    return out


def merge(run_list, options=OPTIONS):
    """``_merge_short_segments`` on frames."""
    r, _, min_seg, short_gap, same_gap = options
    out = []
    for spk, f0, f1 in run_list:
        start, end = f0 * r, f1 * r
        short = end - start < min_seg
        near = short_gap if short else same_gap
        if out and out[-1][0] == spk and start - out[-1][2] * r < near:
            out[-1] = (out[-1][0], out[-1][1], f1)
        elif not short:
            out.append((spk, f0, f1))
    return out


def words(word_start, word_end, seg_start, seg_end):
    """-> for every word the index of the first segment that holds its midpoint, else of the first nearest midpoint, else -1."""
    out = []
    for a, b in zip(word_start, word_end):
        mid = (a + b) / 2
        g = next((i for i, (s, e) in enumerate(zip(seg_start, seg_end)) if s <= mid <= e), None)
        if g is None and len(seg_start):
            g = min(range(len(seg_start)), key=lambda i: abs(mid - (seg_start[i] + seg_end[i]) / 2))
        out.append(-1 if g is None else g)
    return out


def to_dicts(triples, names=None, rate=OPTIONS[0]):
    return [{"speaker": names[k] if names else f"SPEAKER_{k}", "start": a * rate, "end": b * rate} for k, a, b in triples]


def postprocess(window_segments, labels, total_duration, vad_frames, cls=LocalSpeakerDiarizer):
    """``_postprocess_segments`` through the restatement: the host's share (``vote_inputs``) and then frames only."""
    if not window_segments or len(labels) == 0:
        return []
    first, last, rank, names, n_frames = cls.vote_inputs(window_segments, labels, total_duration)
    return to_dicts(merge(runs(owners(first, last, rank, len(names), n_frames, vad_frames, cls.spk_options())), cls.spk_options()), names,
                    cls.VOTING_RATE)


def snap(segments, rate=OPTIONS[0]):
    """Turn dicts on the voting grid -> (triples, names): what ``_merge_short_segments(device=)`` hands to the kernel."""
    names = list(dict.fromkeys(s["speaker"] for s in segments))
    return [(names.index(s["speaker"]), int(round(s["start"] / rate)), int(round(s["end"] / rate))) for s in segments], names


# ----------------------------------------------------------------------------- the sweeps of the GPU tests
SWEEP_LENGTHS = (9, 10, 11, 14, 15, 16, 49, 50, 51)
SWEEP_GAPS = (9, 10, 11, 49, 50, 51)


def merge_sweep(f0_range=range(4096), recordings=64):
    """The merge arithmetic, swept: for every f0, gap and length a kept turn [f0, f0 + 20) and, ``gap`` frames behind its end, the
    run under test of ``length`` frames, both of a speaker of the pattern's own -- ``_merge_short_segments`` compares speakers and
    nothing else about them, so patterns that share a recording cannot touch each other, and the walk sees ``start - end < near`` and
    ``end - start < MIN_SEGMENT_DURATION`` at every position of the grid below 42 s.  A third run of a further speaker, one frame long,
    follows each pattern: short, without a predecessor, dropped.  -> ``recordings`` run lists, patterns dealt round robin."""
    out, p = [[] for _ in range(recordings)], 0
    for f0 in f0_range:
        for gap in SWEEP_GAPS:
            for length in SWEEP_LENGTHS:
                a = f0 + 20 + gap
                out[p % recordings] += [(2 * p, f0, f0 + 20), (2 * p, a, a + length), (2 * p + 1, a + length, a + length + 1)]
                p += 1
    return out


def fma_less(f1, f0, rate, threshold):
    """``fma(f1, rate, -(f0 * rate)) < threshold`` with exact rational arithmetic: ONE rounding of f1 * rate - fl(f0 * rate)."""
    from fractions import Fraction
    exact = Fraction(f1) * Fraction(rate) - Fraction(f0 * rate)
    return float(exact) < threshold                            # float(Fraction) rounds to nearest even, as the fused operation does

"""Writes tests/golden/diarization.json: what the REFERENCE's ``tiny_audio/diarization.py`` returns for the inputs of
diarization_recipe.py.  It needs a checkout of the reference and runs only where one is at hand; no test imports it:

    python tests/golden/make_diarization_fixture.py /path/to/reference/tiny_audio/diarization.py

Recorded: the clusterer's labels (as partitions, ``np.random.seed`` fixed) for the seeded embedding sets; ``_apply_vad_hysteresis``,
the window positions of ``_extract_embeddings`` (a stub model stands in), ``_resample_vad``, ``_postprocess_segments``,
``_merge_short_segments`` and ``assign_speakers_to_words`` on the hand-made inputs; and one whole ``LocalSpeakerDiarizer.diarize``
run whose two model loaders are replaced by the recipe's CPU torch modules behind an ``encode_batch`` and by a VAD replaying
recorded decisions.  The generator asserts that on that run the windows' within-speaker cosines exceed 0.9 and the cosine between the
two centroids is below 0.6, so that the partition cannot hinge on bf16.
"""
import copy
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import diarization_recipe as D  # noqa: E402


class MarkerModel:
    """Stands in for SpeechBrain in the window-position case: a window whose first sample is the marker embeds to zero (dropped)."""

    def encode_batch(self, wavs):
        assert wavs.shape == (1, 12000)
        return torch.zeros(1, 1, 4) if float(wavs[0, 0]) == 0.5 else torch.ones(1, 1, 4)


def main(path):
    spec = importlib.util.spec_from_file_location("reference_diarization", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    L = ref.LocalSpeakerDiarizer
    out = {}

    out["clusterer"] = {}
    for name, (emb, k) in D.embedding_sets().items():
        np.random.seed(D.NUMPY_SEED)
        try:
            labels = ref.SpeakerClusterer()(emb.copy(), k)
        except ValueError as e:            # (the NaN row: its zeroed embedding ends up alone and its centroid has no direction)
            out["clusterer"][name] = {"raises": "ValueError", "message": str(e)}
            print("clusterer", name, "-> ValueError:", e)
            continue
        out["clusterer"][name] = {"partition": D.partition(labels), "labels_in_order": [int(x) for x in labels]}
        print("clusterer", name, "->", len(out["clusterer"][name]["partition"]), "speakers")

    out["hysteresis"] = {k: L._apply_vad_hysteresis(copy.deepcopy(v)) for k, v in D.hysteresis_cases().items()}

    audio = np.zeros(D.WINDOW_CASE_AUDIO, np.float32)
    audio[D.DROPPED_WINDOW_START] = 0.5
    L._ecapa_model = MarkerModel()
    emb, wins = L._extract_embeddings(audio, copy.deepcopy(D.window_cases()), 16000)
    out["windows"] = {"segments": wins, "embeddings": np.asarray(emb).tolist()}
    print("windows:", len(wins))

    out["resample_vad"] = {k: [bool(x) for x in L._resample_vad(list(f), n)] for k, (f, n) in D.resample_vad_cases().items()}
    out["postprocess"] = {k: L._postprocess_segments(copy.deepcopy(w), np.asarray(lb), dur, list(vad))
                          for k, (w, lb, dur, vad) in D.postprocess_cases().items()}
    out["merge"] = {k: L._merge_short_segments(copy.deepcopy(v)) for k, v in D.merge_cases().items()}
    out["words"] = {k: L.assign_speakers_to_words(copy.deepcopy(w), copy.deepcopy(s)) for k, (w, s) in D.word_cases().items()}

    # the whole run
    audio = D.run_audio()
    enc = D.TorchEncoder(D.GEOM, D.run_weights())
    L._ecapa_model = enc
    L._ten_vad_model = D.ReplayVad(D.run_speech_frames())
    segments, frames = L._get_speech_segments(audio, 16000)
    assert frames == D.run_speech_frames()
    emb, wins = L._extract_embeddings(audio, segments, 16000)
    mid = lambda w: (w["start"] + w["end"]) / 2
    who = np.asarray([next((k for k, a, b in D.TURNS if a <= mid(w) < b), -1) for w in wins])
    pure = np.asarray([any(a <= w["start"] and w["end"] <= b for _, a, b in D.TURNS) for w in wins])
    cents = []
    for k in (0, 1):
        e = emb[(who == k) & pure]
        c = e.mean(0) / np.linalg.norm(e.mean(0))
        cents.append(c)
        within = float((e @ e.T).min())
        print(f"speaker {k}: {len(e)} windows inside its turns, smallest within-speaker cosine {within:.4f}")
        assert within > 0.9, within
    between = float(cents[0] @ cents[1])
    print(f"cosine between the centroids {between:.4f}")
    assert between < 0.6, between
    L._ten_vad_model = D.ReplayVad(D.run_speech_frames())
    np.random.seed(D.NUMPY_SEED)
    out["run"] = {"segments": L.diarize(audio), "n_windows": len(wins), "vad_segments": segments}
    L._ten_vad_model = D.ReplayVad(D.run_speech_frames())
    np.random.seed(D.NUMPY_SEED)
    out["run_oracle_two"] = L.diarize(audio, num_speakers=2)
    print("run:", out["run"]["segments"])

    dst = os.path.join(HERE, "diarization.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

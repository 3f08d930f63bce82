"""-m gpu: a whole ``LocalSpeakerDiarizer.diarize`` run with the device's ECAPA-TDNN (one ``embed_windows`` call for every window of every
segment) against what the REFERENCE returned for the same audio with the recipe's CPU torch modules behind its one-window-per-call
loop (tests/golden/diarization.json).  The generator made sure the partition cannot hinge on bf16: on this audio the windows'
within-speaker cosines exceed 0.9 and the cosine between the two centroids is below 0.6; the device's embeddings are held to the same
two conditions here before the segments are compared."""
import json
import os

import numpy as np
import pytest

from tests.golden import diarization_recipe as D
from tests.golden import ecapa_recipe as ER
from tiny_audio_amd import ecapa as E
from tiny_audio_amd.diarization import LocalSpeakerDiarizer as L
from tiny_audio_amd.diarization import SpeakerDiarizer

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_whole_run_on_the_device_equals_the_reference():
    with open(os.path.join(GOLD, "diarization.json")) as f:
        gold = json.load(f)
    m = E.EcapaTdnnMI355X(E.EcapaConfig(**ER.GEOMS[D.GEOM]), device="cuda").load_state_dict_speechbrain(D.run_weights())
    audio, frames = D.run_audio(), D.run_speech_frames()
    segs, _ = L._get_speech_segments(audio, 16000, speech_frames=frames)
    assert segs == gold["run"]["vad_segments"]
    emb, wins = L._extract_embeddings(audio, segs, 16000, speaker_model=m)
    assert len(wins) == gold["run"]["n_windows"] and emb.shape == (len(wins), ER.GEOMS[D.GEOM]["lin_neurons"])
    who = np.asarray([next((k for k, a, b in D.TURNS if a <= w["start"] and w["end"] <= b), -1) for w in wins])
    cents = []
    for k in (0, 1):
        e = emb[who == k]
        cents.append(e.mean(0) / np.linalg.norm(e.mean(0)))
        print(f"speaker {k}: {len(e)} windows inside its turns, smallest within-speaker cosine {float((e @ e.T).min()):.4f}")
        assert (e @ e.T).min() > 0.9
    print(f"cosine between the centroids {float(cents[0] @ cents[1]):.4f}")
    assert cents[0] @ cents[1] < 0.6
    np.random.seed(D.NUMPY_SEED)
    assert L.diarize(audio, speaker_model=m, speech_frames=frames) == gold["run"]["segments"]
    np.random.seed(D.NUMPY_SEED)
    assert SpeakerDiarizer.diarize(audio, num_speakers=2, speaker_model=m, vad=D.ReplayVad(frames)) == gold["run_oracle_two"]

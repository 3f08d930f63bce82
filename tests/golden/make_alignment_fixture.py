"""Writes tests/golden/alignment.npz and alignment.json: the outputs of the REFERENCE's forced aligner on small inputs.

Run on a CPU box that has the reference checkout (nothing of it is copied; only the numbers its functions return are stored):

    python tests/golden/make_alignment_fixture.py --reference <path of the reference checkout>

It loads ``tiny_audio/alignment.py`` of the reference by path and calls its own ``ForcedAligner._get_trellis`` and ``_backtrack``
(a Python double loop: the (300, 130) case takes over a second).  For ``align`` it puts a stub ``torchaudio`` into ``sys.modules``
and presets ``_bundle`` / ``_model`` / ``_labels`` / ``_dictionary`` so that the "model" returns the fixture's logits -- the
reference's own tests mock the model the same way.

alignment.npz, per case ``<name>``: ``<name>.emission`` f32 [T, C], ``<name>.tokens`` i32 [J], ``<name>.trellis`` f32 [T + 1, J + 1],
``<name>.spans`` f64 [J, 3] = (token, start_frame, end_frame) as the reference returned them.
alignment.json: ``cases`` (the names in order) and ``words``: [{key, text, emission: array name, words: the reference's return}].
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = ("-", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'",
          "X", "J", "Q", "Z")


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_alignment", os.path.join(root, "tiny_audio", "alignment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gaussian(rng, T, C):
    return torch.log_softmax(torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32)), dim=-1)


def quantised(rng, T, C):
    """Multiples of 0.5 in [-3, 0]: sums of them are exact in f32, so equal path scores are exactly equal and ties are frequent."""
    return torch.from_numpy((-0.5 * rng.integers(0, 7, (T, C))).astype(np.float32))


def tokens_for(rng, J, C):
    return rng.integers(1, C, J).astype(np.int32)


def build_cases():
    rng = np.random.default_rng(20251)
    cases = {}
    for T, J in ((1, 1), (3, 3), (2, 3), (0, 2), (65, 1), (64, 64), (70, 65), (300, 130)):
        cases[f"g_{T}x{J}"] = (gaussian(rng, T, 29), tokens_for(rng, J, 29))
    for T, J in ((40, 12), (70, 65), (130, 40)):
        cases[f"q_{T}x{J}"] = (quantised(rng, T, 6), tokens_for(rng, J, 6))
    # -inf entries (a class the model rules out in a frame) that leave a path: a third of the non-blank entries
    e = gaussian(rng, 60, 29)
    mask = torch.from_numpy(rng.random((60, 29)) < 0.33)
    mask[:, 0] = False
    cases["inf_60x10"] = (e.masked_fill(mask, -float("inf")), tokens_for(rng, 10, 29))
    # one token's class is -inf in every frame: no path
    e, tk = gaussian(rng, 20, 29), tokens_for(rng, 5, 29)
    e[:, int(tk[2])] = -float("inf")
    cases["dead_20x5"] = (e, tk)
    return cases


WORD_TEXTS = (("plain", "hello world", 120), ("spaces", "the  quick   fox", 120), ("edges", "  padded text  ", 120),
              ("apostrophe", "don't stop", 120), ("digits", "take 42 steps", 120), ("lower", "lower case words", 120),
              ("empty", "", 120), ("unalignable", "42!!", 120), ("only_separator", "42 !!", 120), ("fallback", "hello world", 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TINY_AUDIO_REFERENCE"), required="TINY_AUDIO_REFERENCE" not in os.environ)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    FA = ref.ForcedAligner
    arrays, names = {}, []
    for name, (e, tk) in build_cases().items():
        tokens = [int(x) for x in tk]
        tr = FA._get_trellis(e, tokens, blank_id=0)
        sp = FA._backtrack(tr, e, tokens, blank_id=0)
        arrays[f"{name}.emission"] = e.numpy()
        arrays[f"{name}.tokens"] = np.asarray(tokens, np.int32)
        arrays[f"{name}.trellis"] = tr.numpy()
        arrays[f"{name}.spans"] = np.asarray(sp, np.float64).reshape(len(tokens), 3)
        names.append(name)
        print(name, tuple(e.shape), len(tokens), "score", float(tr[-1, -1]))
    assert np.isfinite(arrays["inf_60x10.trellis"][-1, -1]) and np.isneginf(arrays["dead_20x5.trellis"][-1, -1])

    # ForcedAligner.align of the reference with the acoustic model mocked
    stub = types.ModuleType("torchaudio")
    stub.functional = types.SimpleNamespace(resample=lambda w, a, b: w)
    sys.modules["torchaudio"] = stub
    FA._bundle = types.SimpleNamespace(sample_rate=16000)
    FA._labels = LABELS
    FA._dictionary = {c: i for i, c in enumerate(LABELS)}
    rng = np.random.default_rng(20252)
    words = []
    logits = {T: torch.from_numpy(rng.standard_normal((T, 29)).astype(np.float32) * 3) for T in (120, 4)}    # shared by the texts
    for T, l in logits.items():
        arrays[f"w_{T}.emission"] = torch.log_softmax(l[None], dim=-1)[0].numpy()      # what the reference aligns
    for key, text, T in WORD_TEXTS:
        FA._model = lambda w, _l=logits[T]: (_l[None], None)
        got = FA.align(np.zeros(16000, np.float32), text)
        words.append(dict(key=key, text=text, emission=f"w_{T}", words=got))
        print(key, repr(text), got)
    np.savez_compressed(os.path.join(HERE, "alignment.npz"), **arrays)
    with open(os.path.join(HERE, "alignment.json"), "w") as f:
        json.dump(dict(cases=names, words=words), f, indent=1)
    print("alignment.npz", os.path.getsize(os.path.join(HERE, "alignment.npz")), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/text_align.json: the pairs the REFERENCE's ``align_words_to_reference`` returns on small word lists.

Run on a CPU box that has the reference checkout (nothing of it is copied; only the indices its function returns are stored):

    python tests/golden/make_text_align_fixture.py --reference <path of the reference checkout>

It loads ``scripts/eval/evaluators/alignment.py`` of the reference by path.  That module imports the evaluator package's audio
helpers and its ``base`` module (soundfile, transformers' Whisper normaliser, an API client) at import time, none of which the
function under test uses, so empty stand-ins for those modules are put into ``sys.modules`` first.  The normaliser handed to the
function is a stub that lower-cases and strips, as the tests' own stub does.

text_align.json: ``cases``: [{name, pred: [word, ...], ref: [word, ...], pairs: [[pred_index, ref_index], ...]}] -- the words are the
``"word"`` fields of the dicts passed in (each dict also carried its index, which is how the returned dicts are identified).
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class StubNormalizer:
    def normalize(self, text):
        return text.lower().strip()


def load_reference(root):
    for name in ("scripts", "scripts.eval", "scripts.eval.audio", "scripts.eval.evaluators", "scripts.eval.evaluators.base"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["scripts.eval.audio"].TextNormalizer = StubNormalizer
    sys.modules["scripts.eval.audio"].prepare_wav_bytes = None
    for attr in ("AlignmentResult", "console", "setup_assemblyai"):
        setattr(sys.modules["scripts.eval.evaluators.base"], attr, None)
    path = os.path.join(root, "scripts", "eval", "evaluators", "alignment.py")
    spec = importlib.util.spec_from_file_location("scripts.eval.evaluators.alignment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_cases():
    rng = np.random.default_rng(20261)
    vocab = ["the", "a", "of", "cat", "dog", "sat", "mat", "on", "ran", "to"]
    cases = [
        ("identical", "the cat sat on the mat".split(), "the cat sat on the mat".split()),
        ("repeats_ta", ["the", "a"] * 6, ["a", "the"] * 5 + ["the"]),
        ("repeats_at", ["a", "the", "a", "a", "the"] * 3, ["the", "a", "the", "the"] * 4),
        ("case_and_space", ["The", " CAT ", "sat"], ["the", "cat", "Sat", "down"]),
        ("unk_and_empty", ["the", "", "cat", " ", "sat"], ["the", "<unk>", "cat", "<unk>", "", "sat"]),
        ("pred_unk_kept", ["<unk>", "cat"], ["<UNK>", "cat"]),
        ("disjoint", ["x", "y", "z"], ["a", "b"]),
        ("no_pred", [], ["a", "b"]),
        ("no_ref", ["a"], []),
        ("only_unk_ref", ["a"], ["<unk>"]),
        ("insert_delete", "a b c d e f g".split(), "a c x d f g h".split()),
    ]
    for k, (n_pred, n_ref, v) in enumerate(((70, 65, 2), (64, 64, 3), (130, 100, 4), (33, 129, 10))):
        cases.append((f"random_{k}", [vocab[i] for i in rng.integers(0, v, n_pred)], [vocab[i] for i in rng.integers(0, v, n_ref)]))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TINY_AUDIO_REFERENCE"), required="TINY_AUDIO_REFERENCE" not in os.environ)
    args = ap.parse_args()
    fn = load_reference(args.reference).align_words_to_reference
    out = []
    for name, pred, ref in build_cases():
        pw = [dict(word=w, index=i) for i, w in enumerate(pred)]
        rw = [dict(word=w, index=i) for i, w in enumerate(ref)]
        got = fn(pw, rw, StubNormalizer())
        pairs = [[p["index"], r["index"]] for p, r in got]
        out.append(dict(name=name, pred=pred, ref=ref, pairs=pairs))
        print(name, len(pred), len(ref), len(pairs))
    with open(os.path.join(HERE, "text_align.json"), "w") as f:
        json.dump(dict(cases=out), f, indent=1)
    print("text_align.json", os.path.getsize(os.path.join(HERE, "text_align.json")), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/wav2vec2_sln_{c,d}.npz: what transformers' ``Wav2Vec2ForCTC`` of the layer-norm / stable family computes on the
CPU from the seeded weights and clips of wav2vec2_sln_recipe.py, each clip alone and unpadded, its input brought to zero mean and
unit variance as ``Wav2Vec2FeatureExtractor`` does.  Run from the repository root:  python tests/golden/make_wav2vec2_sln_fixture.py

Per geometry and clip i:
  logits_f32_i   [T, 32] float32   the fp32 module's logits
  logits_bf16_i  [T, 32] uint16    the raw bits of the SAME module cast to bfloat16 on the same input: the tests' yardstick
  feat_i / pos_i / layer0_i  (geometry c)  fp32 hidden state behind the feature extractor [T, C], behind the positional-conv add
                 (hidden_states[0]: no LayerNorm there in this family) and behind layer 0 (hidden_states[1], the raw residual stream)
and for clip RAW_CLIP the same two logits on the RAW waveform: logits_f32_raw, logits_bf16_raw.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import wav2vec2_sln_recipe as R  # noqa: E402


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    torch.manual_seed(0)
    for geom in R.GEOMS:
        sd = R.weights(geom)
        m = R.hf_model(geom, sd)
        mb = R.hf_model(geom, sd).to(torch.bfloat16)
        raw = R.waves()
        inputs = [(str(i), R.normalize_hf(w)) for i, w in enumerate(raw)] + [("raw", raw[R.RAW_CLIP])]
        out = {}
        for tag, w in inputs:
            x = torch.from_numpy(w)[None]
            with torch.no_grad():
                r = m(x, output_hidden_states=True)
                lb = mb(x.to(torch.bfloat16)).logits[0]
            out[f"logits_f32_{tag}"] = r.logits[0].numpy().astype(np.float32)
            out[f"logits_bf16_{tag}"] = bits(lb)
            if geom == "c" and tag != "raw":
                with torch.no_grad():
                    out[f"feat_{tag}"] = m.wav2vec2.feature_extractor(x)[0].transpose(0, 1).contiguous().numpy()
                out[f"pos_{tag}"] = r.hidden_states[0][0].numpy()
                out[f"layer0_{tag}"] = r.hidden_states[1][0].numpy()
            lf, lbf = out[f"logits_f32_{tag}"].astype(np.float64), lb.double().numpy()
            print(geom, tag, lf.shape, "logit range", float(lf.min()), float(lf.max()), "bf16 module relmax",
                  float(np.abs(lbf - lf).max() / np.abs(lf).max()),
                  "cos", float((lbf * lf).sum() / np.sqrt((lbf * lbf).sum() * (lf * lf).sum())))
        path = os.path.join(HERE, f"wav2vec2_sln_{geom}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/wav2vec2_{a,b}.npz: what transformers' ``Wav2Vec2ForCTC`` computes on the CPU from the seeded weights and clips of
wav2vec2_recipe.py, each clip alone and unpadded.  Run from the repository root:  python tests/golden/make_wav2vec2_fixture.py

Per geometry and clip i:
  logits_f32_i   [T, 32] float32   the fp32 module's logits
  logits_bf16_i  [T, 32] uint16    the raw bits of the SAME module cast to bfloat16 on the same input: the tests' yardstick
  feat_i / pos_i / layer0_i  (geometry a)  fp32 hidden state behind the feature extractor [T, C], behind the positional-conv block
                 (encoder.layer_norm's output, hidden_states[0]) and behind layer 0 (hidden_states[1])
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import wav2vec2_recipe as R  # noqa: E402


def main():
    torch.manual_seed(0)
    for geom in R.GEOMS:
        sd = R.weights(geom)
        m = R.hf_model(geom, sd)
        out = {}
        for i, w in enumerate(R.waves()):
            x = torch.from_numpy(w)[None]
            with torch.no_grad():
                r = m(x, output_hidden_states=True)
                out[f"logits_f32_{i}"] = r.logits[0].numpy().astype(np.float32)
                if geom == "a":
                    out[f"feat_{i}"] = m.wav2vec2.feature_extractor(x)[0].transpose(0, 1).contiguous().numpy()
                    out[f"pos_{i}"] = r.hidden_states[0][0].numpy()
                    out[f"layer0_{i}"] = r.hidden_states[1][0].numpy()
        mb = R.hf_model(geom, sd).to(torch.bfloat16)
        for i, w in enumerate(R.waves()):
            with torch.no_grad():
                lb = mb(torch.from_numpy(w)[None].to(torch.bfloat16)).logits[0]
            out[f"logits_bf16_{i}"] = lb.contiguous().view(torch.int16).numpy().view(np.uint16)
            lf, lbf = out[f"logits_f32_{i}"].astype(np.float64), lb.double().numpy()
            print(geom, i, lf.shape, "logit range", float(lf.min()), float(lf.max()), "bf16 module relmax",
                  float(np.abs(lbf - lf).max() / np.abs(lf).max()),
                  "cos", float((lbf * lf).sum() / np.sqrt((lbf * lbf).sum() * (lf * lf).sum())))
        path = os.path.join(HERE, f"wav2vec2_{geom}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

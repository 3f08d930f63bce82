"""Writes tests/golden/ecapa_{a,full}.npz: what a composition of torch's own modules (ecapa_recipe.torch_model) computes on the CPU from
the seeded weights and windows of ecapa_recipe.py, each window alone.  Run from the repository root:
    python tests/golden/make_ecapa_fixture.py

Per geometry and window i:
  emb_f32_i    [D] float32    the fp32 module's embedding of the fp32 torch.stft features
  emb_bf16_i   [D] uint16     the raw bits of the SAME modules cast to bfloat16 on the same fp32 features: the tests' yardstick
  feat_i / block0_i / blk1_i / blk2_i / blk3_i / mfa_i / attn_i / pooled_i   (geometry a)  the fp32 intermediates, time-major
Geometry a also holds feat_yardstick_db [4]: max |torch.stft f32 features - float64 definition| in dB on ecapa_recipe.feature_windows().

The generator asserts that the fixtures can see a broken softmax or a kernel that ignores its input: (a) the largest attention weight
of the 76-frame window is at least 5 / 76, (b) the cosine between the embeddings of different windows is below 0.9.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ecapa_ref as REF  # noqa: E402
from tests.golden import ecapa_recipe as R  # noqa: E402

INTERMEDIATES = ("block0", "blk1", "blk2", "blk3", "mfa", "attn", "pooled")


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(16)
    for geom in R.GEOMS:
        sd = R.weights(geom)
        m = R.torch_model(geom, sd)
        out, embs = {}, []
        feats = [R.torch_fbank(w) for w in R.windows()]
        for i, f in enumerate(feats):
            with torch.no_grad():
                r = m(f.T[None])
            out[f"emb_f32_{i}"] = r["emb"][0].numpy().astype(np.float32)
            embs.append(r["emb"][0].double().numpy())
            if geom == "a":
                out[f"feat_{i}"] = f.numpy()
                for k in INTERMEDIATES:
                    out[f"{k}_{i}"] = r[k][0].numpy().astype(np.float32)
            T = f.shape[0]
            wmax = float(r["attn"].max())
            print(geom, i, "T", T, "emb absmax", float(np.abs(embs[-1]).max()), "largest attention weight", wmax, "against 1/T", 1.0 / T)
            if T == 76:
                assert wmax >= 5.0 / T, f"condition (a): the attention is too flat ({wmax} < {5.0 / T})"
        for i in range(len(embs)):
            for j in range(i + 1, len(embs)):
                c = float(embs[i] @ embs[j] / np.sqrt((embs[i] @ embs[i]) * (embs[j] @ embs[j])))
                print(geom, f"cosine between windows {i} and {j}: {c:.4f}")
                assert c < 0.9, f"condition (b): windows {i} and {j} embed alike (cosine {c})"
        mb = R.torch_model(geom, sd).to(torch.bfloat16)
        for i, f in enumerate(feats):
            with torch.no_grad():
                eb = mb(f.T[None].to(torch.bfloat16))["emb"][0]
            out[f"emb_bf16_{i}"] = bits(eb)
            ef, ebd = embs[i], eb.double().numpy()
            print(geom, i, "bf16 module relmax", float(np.abs(ebd - ef).max() / np.abs(ef).max()), "1 - cos",
                  float(1.0 - (ebd @ ef) / np.sqrt((ebd @ ebd) * (ef @ ef))))
        if geom == "a":
            ys = []
            for chunk, L in R.feature_windows():
                wav = REF.reflect_extend(chunk, L).astype(np.float32)
                ys.append(float(np.abs(R.torch_fbank(wav).double().numpy() - REF.fbank(wav)).max()))
            out["feat_yardstick_db"] = np.asarray(ys, np.float64)
            print("feature yardstick (dB):", ys)
        path = os.path.join(HERE, f"ecapa_{geom}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

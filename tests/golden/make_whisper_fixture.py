"""Writes the Whisper-tower fixtures from transformers on the CPU (run from the repository root:
``python tests/golden/make_whisper_fixture.py``).  No program text is stored, only arrays transformers produced:

* ``whisper_logmel80.npz``          ``WhisperFeatureExtractor(feature_size=80)`` features [2, 80, 3000] and masks [2, 3000] of the two
                                    clips of ``whisper_recipe.waves()`` with its default ("max_length") padding;
* ``whisper_encoder_small_f32_{0,1}.npz``  fp32 ``last_hidden_state`` [1500, 128] of clip 0 / 1 from a random-weight ``WhisperEncoder``
                                    (``whisper_recipe.encoder_weights()``: the weights are rebuilt from the seed, not stored) fed those features;
* ``whisper_encoder_small_bf16.npz``  the same module cast ``.to(torch.bfloat16)`` on the same input (the raw bf16 bits as uint16 [2, 1500, 128]):
                                    the yardstick for how far a bf16 implementation sits from the fp32 one.

One array set per file keeps every file under the 1 MiB limit for committed files.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import whisper_recipe as R  # noqa: E402


def main():
    from transformers import WhisperFeatureExtractor
    torch.manual_seed(0)
    fe = WhisperFeatureExtractor(feature_size=80)
    f = fe(R.waves(), sampling_rate=16000, return_attention_mask=True, return_tensors="np")
    feats, mask = f["input_features"].astype(np.float32), f["attention_mask"].astype(np.int32)
    assert feats.shape == (2, 80, 3000) and mask.sum(-1).tolist() == [1000, 301], (feats.shape, mask.sum(-1))
    np.savez_compressed(os.path.join(HERE, "whisper_logmel80.npz"), input_features=feats, attention_mask=mask)
    enc = R.hf_encoder(R.SMALL, R.encoder_weights())
    x = torch.from_numpy(feats)
    with torch.no_grad():
        y32 = enc(x).last_hidden_state.float().numpy()
        yb = enc.to(torch.bfloat16)(x.to(torch.bfloat16)).last_hidden_state
    for b in range(2):
        np.savez_compressed(os.path.join(HERE, f"whisper_encoder_small_f32_{b}.npz"), last_hidden_state=y32[b])
    np.savez_compressed(os.path.join(HERE, "whisper_encoder_small_bf16.npz"), last_hidden_state_bf16_bits=yb.view(torch.int16).numpy().view(np.uint16))
    a, r = yb.float().numpy().ravel().astype(np.float64), y32.ravel().astype(np.float64)
    print(f"bf16 module vs fp32 module: relmax {np.abs(a - r).max() / np.abs(r).max():.5f} cosine {a @ r / np.linalg.norm(a) / np.linalg.norm(r):.6f}")
    for n in sorted(os.listdir(HERE)):
        if n.startswith("whisper_"):
            print(n, os.path.getsize(os.path.join(HERE, n)))


if __name__ == "__main__":
    main()

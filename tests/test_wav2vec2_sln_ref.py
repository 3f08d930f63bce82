"""tests/wav2vec2_sln_ref.py IS transformers' Wav2Vec2ForCTC with feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True:
pinned on the CPU fixtures (tests/golden/wav2vec2_sln_{c,d}.npz, written by make_wav2vec2_sln_fixture.py from the seeded weights of
wav2vec2_sln_recipe.py) to 1e-4 of each array's maximum, the base model's pin.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import wav2vec2_sln_ref as REF
from tests.golden import wav2vec2_sln_recipe as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, top = np.abs(got - want).max(), np.abs(want).max()
    assert err <= 1e-4 * top, f"{what}: max |d| {err:.3e} against 1e-4 * {top:.3e}"


@pytest.mark.parametrize("geom", ["c", "d"])
def test_definition_matches_transformers(geom):
    """Normalised input (the definition normalises the raw clip itself, in float64), every stored stage of geometry c, and the one
    clip stored without normalisation."""
    fx = np.load(os.path.join(GOLD, f"wav2vec2_sln_{geom}.npz"))
    sd, cfg = R.weights(geom), R.GEOMS[geom]
    nh, nl = cfg["num_attention_heads"], cfg["num_hidden_layers"]
    for i, wav in enumerate(R.waves()):
        want = ("feat", "pos", "layer0") if geom == "c" else ("feat",)
        logits, inter = REF.forward(sd, wav, nh, nl, want=want, normalize="hf")
        assert logits.shape == (R.frames_of(len(wav)), R.N_CLASSES)
        _close(logits, fx[f"logits_f32_{i}"], f"{geom} clip {i} logits")
        if geom == "c":
            for k in want:
                _close(inter[k], fx[f"{k}_{i}"], f"{geom} clip {i} {k}")
    _close(REF.forward(sd, R.waves()[R.RAW_CLIP], nh, nl), fx["logits_f32_raw"], f"{geom} raw clip logits")


def test_fixture_logits_are_not_flat_and_the_raw_clip_differs():
    for geom in R.GEOMS:
        fx = np.load(os.path.join(GOLD, f"wav2vec2_sln_{geom}.npz"))
        for tag in ("0", "1", "raw"):
            l = fx[f"logits_f32_{tag}"]
            assert l.max() - l.min() > 16.0 and np.abs(l).max() < 64.0
        assert np.abs(fx["logits_f32_raw"] - fx[f"logits_f32_{R.RAW_CLIP}"]).max() > 1.0, "normalisation changed nothing"


def test_input_normalisation_definition():
    """Both published forms: transformers' numpy line (eps 1e-7) and torchaudio's layer_norm(waveform, waveform.shape) (eps 1e-5)."""
    w = R.waves()[0]
    np.testing.assert_allclose(REF.normalize_input(w, 1e-7).numpy(), R.normalize_hf(w), rtol=0, atol=2e-5)
    x = torch.from_numpy(w)[None].double()
    np.testing.assert_allclose(REF.normalize_input(w, 1e-5).numpy(), torch.nn.functional.layer_norm(x, x.shape)[0].numpy(), rtol=0, atol=1e-12)
    z = REF.normalize_input(np.zeros(400, np.float32), 1e-7)
    assert torch.isfinite(z).all() and not z.any()


def test_conv_layer_definition_is_torch():
    """conv + bias -> LayerNorm over the channels -> GELU against torch's own modules in float64, layer 0 and a k = 3 layer."""
    g = torch.Generator().manual_seed(9)
    for cin, k, s in ((1, 10, 5), (16, 3, 2)):
        x = torch.randn(97, cin, generator=g, dtype=torch.float64)
        w = torch.randn(32, cin, k, generator=g, dtype=torch.float64) * 0.3
        b, lw, lb = (torch.randn(32, generator=g, dtype=torch.float64) for _ in range(3))
        y = torch.nn.functional.conv1d(x.T[None], w, b, stride=s)[0].T
        want = torch.nn.functional.gelu(torch.nn.functional.layer_norm(y, (32,), lw, lb, 1e-5))
        np.testing.assert_allclose(REF.conv_ln_gelu(x, w, b, lw, lb, s).numpy(), want.numpy(), rtol=1e-10, atol=1e-12)

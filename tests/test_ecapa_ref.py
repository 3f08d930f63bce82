"""The float64 definition (tests/ecapa_ref.py) against what torch's own modules computed (tests/golden/ecapa_{a,full}.npz): every array
of the fixtures to 1e-4 of its own maximum.  This pins the definition the device tests measure against; it needs no GPU."""
import os

import numpy as np
import pytest

from tests import ecapa_ref as REF
from tests.golden import ecapa_recipe as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= TOL * np.abs(want).max(), f"{what}: max |d| {err:.3e} against {TOL} x {np.abs(want).max():.3e}"


@pytest.fixture(scope="module")
def forwards():
    """geometry -> [the definition's outputs per window]: computed once, shared, left unchanged."""
    return {geom: [REF.forward(R.weights(geom), REF.fbank(w), R.DILATIONS) for w in R.windows()] for geom in R.GEOMS}


def test_features_match_torch_stft():
    fx = np.load(os.path.join(GOLD, "ecapa_a.npz"))
    for i, w in enumerate(R.windows()):
        f = REF.fbank(w)
        assert f.shape == (R.frames_of(len(w)), 80)
        close(f, fx[f"feat_{i}"], f"features of window {i}")
        assert np.abs(f.mean(0)).max() < 1e-9


def test_reflect_extension_is_numpy_reflect():
    x = np.arange(10.0)
    assert REF.reflect_extend(x, 14).tolist() == list(range(10)) + [8, 7, 6, 5]
    assert REF.reflect_extend(x, 10) is not None and len(REF.reflect_extend(x, 19)) == 19
    with pytest.raises(AssertionError):
        REF.reflect_extend(x, 20)


def test_intermediates_match_the_torch_modules(forwards):
    fx = np.load(os.path.join(GOLD, "ecapa_a.npz"))
    for i, out in enumerate(forwards["a"]):
        for k in ("block0", "blk1", "blk2", "blk3", "mfa", "attn", "pooled"):
            close(out[k], fx[f"{k}_{i}"], f"{k} of window {i}")
        assert np.abs(out["attn"].sum(0) - 1).max() < 1e-12


@pytest.mark.parametrize("geom", ["a", "full"])
def test_embeddings_match_the_torch_modules(forwards, geom):
    fx = np.load(os.path.join(GOLD, f"ecapa_{geom}.npz"))
    for i, out in enumerate(forwards[geom]):
        close(out["emb"], fx[f"emb_f32_{i}"], f"embedding of window {i}")


def test_the_fixture_can_see_a_flat_attention_and_a_deaf_model(forwards):
    """The generator's two conditions, re-checked on the definition: (a) the largest attention weight of the 76-frame window is at
    least 5 / 76; (b) different windows embed with a cosine below 0.9."""
    for geom, outs in forwards.items():
        assert outs[0]["attn"].shape[0] == 76 and outs[0]["attn"].max() >= 5.0 / 76
        e = [o["emb"] for o in outs]
        for i in range(3):
            for j in range(i + 1, 3):
                assert e[i] @ e[j] / np.sqrt((e[i] @ e[i]) * (e[j] @ e[j])) < 0.9

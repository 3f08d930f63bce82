"""tests/wav2vec2_ref.py IS transformers' Wav2Vec2ForCTC: pinned on the CPU fixtures (tests/golden/wav2vec2_{a,b}.npz, written by
make_wav2vec2_fixture.py from the seeded weights of wav2vec2_recipe.py), to fp32-rounding distance.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import wav2vec2_ref as REF
from tests.golden import wav2vec2_recipe as R
from tiny_audio_amd import wav2vec2 as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, top = np.abs(got - want).max(), np.abs(want).max()
    assert err <= 1e-4 * top, f"{what}: max |d| {err:.3e} against 1e-4 * {top:.3e}"


@pytest.mark.parametrize("geom", ["a", "b"])
def test_definition_matches_transformers(geom):
    fx = np.load(os.path.join(GOLD, f"wav2vec2_{geom}.npz"))
    sd, cfg = R.weights(geom), R.GEOMS[geom]
    for i, wav in enumerate(R.waves()):
        want = ("feat", "pos", "layer0") if geom == "a" else ("feat",)
        logits, inter = REF.forward(sd, wav, cfg["num_attention_heads"], cfg["num_hidden_layers"], want=want)
        assert logits.shape == (R.frames_of(len(wav)), R.N_CLASSES)
        _close(logits, fx[f"logits_f32_{i}"], f"{geom} clip {i} logits")
        if geom == "a":
            for k in want:
                _close(inter[k], fx[f"{k}_{i}"], f"{geom} clip {i} {k}")


def test_fixture_logits_are_not_flat():
    """The head gain does its job: the fixtures' emissions are far from uniform (a uniform model would pass any softmax test)."""
    for geom in R.GEOMS:
        fx = np.load(os.path.join(GOLD, f"wav2vec2_{geom}.npz"))
        for i in range(len(R.CLIP_SAMPLES)):
            l = fx[f"logits_f32_{i}"]
            assert l.max() - l.min() > 16.0 and np.abs(l).max() < 64.0


@pytest.mark.parametrize("L,T", [(399, 0), (400, 1), (719, 1), (720, 2), (16000, 49), (480000, 1499)])
def test_length_formula(L, T):
    assert REF.frames_of(L) == T and W.frames_of(L) == T and R.frames_of(L) == T
    if L >= 400:
        assert T == (L - 400) // 320 + 1


def test_weight_norm_fold():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(32, 2, 128, generator=g)
    gg = torch.rand(1, 1, 128, generator=g) + 0.5
    conv = torch.nn.Conv1d(32, 32, 128, padding=64, groups=16)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(gg)
        conv.parametrizations.weight.original1.copy_(v)
    want = conv.weight.detach().double().numpy()
    np.testing.assert_allclose(REF.fold_weight_norm(gg.numpy(), v.numpy()).numpy(), want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(W.fold_weight_norm(gg, v).double().numpy(), want, rtol=1e-6, atol=1e-7)
    # every tap of the folded weight has norm g[tap]
    w = W.fold_weight_norm(gg, v)
    np.testing.assert_allclose(w.pow(2).sum(dim=(0, 1)).sqrt().numpy(), gg.reshape(-1).numpy(), rtol=1e-5)


def test_pos_conv_definition_is_torch_conv1d_without_its_last_frame():
    g = torch.Generator().manual_seed(5)
    for T in (1, 2, 64, 65, 130):
        x = torch.randn(T, 128, generator=g, dtype=torch.float64)
        w = torch.randn(128, 8, 128, generator=g, dtype=torch.float64) * 0.05
        b = torch.randn(128, generator=g, dtype=torch.float64)
        y = torch.nn.functional.conv1d(x.T[None], w, b, padding=64, groups=16)[0, :, :-1].T
        want = x + torch.nn.functional.gelu(y)
        np.testing.assert_allclose(REF.pos_conv_add(x, w, b).numpy(), want.numpy(), rtol=1e-10, atol=1e-12)


def test_hf_head_to_torchaudio_labels():
    """labels="torchaudio": rows 1, 2, 3 (<s>, </s>, <unk>) of the 32-class HF head leave, blank (<pad>) stays at 0 and '|' lands on
    1: the 29 classes of alignment.LABELS."""
    from tiny_audio_amd.alignment import LABELS
    rows = W.head_rows(32, "torchaudio")
    assert rows == [0] + list(range(4, 32)) == REF.head_rows(32, "torchaudio") and len(rows) == len(LABELS) == 29
    hf_vocab = ["<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G",
                "Y", "P", "B", "V", "K", "'", "X", "J", "Q", "Z"]          # facebook/wav2vec2-base-960h vocab.json, by id
    assert tuple(hf_vocab[r] for r in rows)[1:] == LABELS[1:]
    assert W.head_rows(32, "hf") == list(range(32))
    with pytest.raises(ValueError):
        W.head_rows(29, "torchaudio")
    with pytest.raises(ValueError):
        W.head_rows(32, "fairseq")
    sd = R.weights("a")
    cfg = W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=29)
    b = W.pack_state_dict(sd, cfg, labels="torchaudio")
    assert b["head_w"].shape == (W.HEAD_PAD, 256) and not b["head_w"][29:].any()
    np.testing.assert_array_equal(b["head_w"][:29].float().numpy(), torch.from_numpy(sd["lm_head.weight"][rows]).bfloat16().float().numpy())
    np.testing.assert_array_equal(b["head_b"].numpy(), sd["lm_head.bias"][rows])
    with pytest.raises(ValueError):
        W.pack_state_dict(sd, W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=32), labels="torchaudio")


def _to_torchaudio(sd):
    """transformers names -> the torchaudio names the issue lists (weight norm in its older weight_g / weight_v form)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("lm_head."):
            out["aux." + k[len("lm_head."):]] = v
            continue
        k = k[len("wav2vec2."):]
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        if k.startswith("feature_projection."):
            k = "encoder." + k
        elif k.startswith("encoder."):
            k = "encoder.transformer." + k[len("encoder."):]
        out[k] = v
    return out


def test_torchaudio_renaming_round_trip():
    sd = R.weights("a")
    ta = _to_torchaudio(sd)
    for name in ("feature_extractor.conv_layers.3.conv.weight", "encoder.feature_projection.projection.bias",
                 "encoder.transformer.pos_conv_embed.conv.weight_g", "encoder.transformer.pos_conv_embed.conv.weight_v",
                 "encoder.transformer.layers.1.attention.k_proj.bias", "encoder.transformer.layer_norm.weight", "aux.weight"):
        assert name in ta, name
    back = W.rename_torchaudio(ta)
    cfg = W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=32)
    a, b = W.pack_state_dict(sd, cfg), W.pack_state_dict(back, cfg)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(KeyError):
        W.rename_torchaudio({"mask_generator.mask_embedding": 0})

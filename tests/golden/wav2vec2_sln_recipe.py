"""The seeded inputs of the layer-norm / stable wav2vec2 fixtures (tests/golden/make_wav2vec2_sln_fixture.py) and of the tests that read
them: ``Wav2Vec2ForCTC`` with feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True -- the family of
wav2vec2-large-960h-lv60, XLSR-53, XLS-R 300M and MMS 300M.  The clips, the class count and the head gain are those of
wav2vec2_recipe.py; the weights are numpy ``Generator`` draws, so the fixtures hold only what transformers computed from them.
"""
import numpy as np

from tests.golden.wav2vec2_recipe import CLIP_SAMPLES, CONV_KERNEL, CONV_STRIDE, HEAD_GAIN, N_CLASSES, frames_of, waves  # noqa: F401

# (c) 16 channels per positional-conv group, (d) the true width of the large models: 64 per group, the kernel's upper limit; two layers each
GEOMS = {
    "c": dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, conv_dim=128, num_hidden_layers=2),
    "d": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, conv_dim=512, num_hidden_layers=2),
}
FAMILY = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
HF_NORM_EPS = 1e-7       # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm
RAW_CLIP = 0             # the clip that is also stored WITHOUT input normalisation


def normalize_hf(x):
    """``Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm`` on one unpadded float32 clip, as transformers writes it."""
    x = np.asarray(x, np.float32)
    return ((x - x.mean()) / np.sqrt(x.var() + HF_NORM_EPS)).astype(np.float32)


def weights(geom, seed=0):
    """``Wav2Vec2ForCTC.state_dict()`` names -> float32 arrays: O(1 / sqrt(fan_in)) matrices, perturbed norm gains on EVERY norm
    (the seven conv LayerNorms included), non-zero conv biases, a weight-normed positional conv whose g is NOT the norm of v,
    and the head gain -- nothing is near-uniform."""
    cfg = GEOMS[geom]
    H, F, C, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["conv_dim"], cfg["num_hidden_layers"]
    cg = H // 16
    g = np.random.default_rng(1000 * seed + (13 if geom == "c" else 17))
    rn = lambda *s, std=1.0: (g.standard_normal(s) * std).astype(np.float32)
    sd = {}
    fe = "wav2vec2.feature_extractor.conv_layers."
    for i in range(7):
        cin = 1 if i == 0 else C
        sd[fe + f"{i}.conv.weight"] = rn(C, cin, CONV_KERNEL[i], std=np.sqrt((1.0 if i == 0 else 2.0) / (CONV_KERNEL[i] * cin)))
        sd[fe + f"{i}.conv.bias"] = rn(C, std=0.1)
        sd[fe + f"{i}.layer_norm.weight"], sd[fe + f"{i}.layer_norm.bias"] = 1 + rn(C, std=0.1), rn(C, std=0.1)
    fp = "wav2vec2.feature_projection."
    sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"] = 1 + rn(C, std=0.1), rn(C, std=0.02)
    sd[fp + "projection.weight"], sd[fp + "projection.bias"] = rn(H, C, std=1 / np.sqrt(C)), rn(H, std=0.02)
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    sd[pc + "parametrizations.weight.original1"] = rn(H, cg, 128, std=1.0)
    sd[pc + "parametrizations.weight.original0"] = (np.sqrt(H / 128.0) * (1 + 0.3 * g.standard_normal((1, 1, 128)))).astype(np.float32)
    sd[pc + "bias"] = rn(H, std=0.05)
    sd["wav2vec2.encoder.layer_norm.weight"], sd["wav2vec2.encoder.layer_norm.bias"] = 1 + rn(H, std=0.1), rn(H, std=0.02)
    for i in range(L):
        p = f"wav2vec2.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj"):
            sd[p + f"attention.{n}.weight"], sd[p + f"attention.{n}.bias"] = rn(H, H, std=1 / np.sqrt(H)), rn(H, std=0.05)
        sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"] = rn(H, H, std=0.5 / np.sqrt(H)), rn(H, std=0.02)
        sd[p + "feed_forward.intermediate_dense.weight"] = rn(F, H, std=1 / np.sqrt(H))
        sd[p + "feed_forward.intermediate_dense.bias"] = rn(F, std=0.02)
        sd[p + "feed_forward.output_dense.weight"] = rn(H, F, std=0.5 / np.sqrt(F))
        sd[p + "feed_forward.output_dense.bias"] = rn(H, std=0.02)
        for n in ("layer_norm", "final_layer_norm"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + rn(H, std=0.1), rn(H, std=0.02)
    sd["lm_head.weight"] = (rn(N_CLASSES, H, std=1 / np.sqrt(H)) * HEAD_GAIN).astype(np.float32)
    sd["lm_head.bias"] = rn(N_CLASSES, std=0.5)
    return sd


def hf_config_dict(geom):
    """The ``Wav2Vec2Config`` fields of a geometry, as ``config.json`` would carry them."""
    cfg = GEOMS[geom]
    return dict(vocab_size=N_CLASSES, hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                conv_dim=(cfg["conv_dim"],) * 7, conv_kernel=CONV_KERNEL, conv_stride=CONV_STRIDE, num_conv_pos_embeddings=128,
                num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, hidden_act="gelu", feat_extract_activation="gelu", **FAMILY)


def hf_model(geom, sd):
    """A transformers ``Wav2Vec2ForCTC`` (CPU, fp32, eval, eager attention) of the family carrying ``sd``."""
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    m = Wav2Vec2ForCTC(Wav2Vec2Config(attn_implementation="eager", **hf_config_dict(geom))).eval()
    r = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not r.unexpected_keys and set(r.missing_keys) <= {"wav2vec2.masked_spec_embed"}, r
    return m

"""The seeded inputs of the wav2vec2 fixtures (tests/golden/make_wav2vec2_fixture.py) and of the tests that read them.

The weights are plain numpy ``Generator`` draws, so the fixtures hold only what transformers computed from them: the tests rebuild the
very same arrays from the seed instead of carrying them in git.
"""
import numpy as np

CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
N_CLASSES = 32
HEAD_GAIN = 8.0          # lm_head.weight is multiplied by this: at unit gain the emissions are nearly uniform and test nothing
# (a) 16 channels per positional-conv group, (b) the true width of wav2vec2-base (48 per group), two layers each
GEOMS = {
    "a": dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, conv_dim=128, num_hidden_layers=2),
    "b": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, conv_dim=512, num_hidden_layers=2),
}
CLIP_SAMPLES = (8123, 45011)          # 25 and 140 frames: one clip inside a single attention tile, one across three


def frames_of(n):
    for k, s in zip(CONV_KERNEL, CONV_STRIDE):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def waves():
    """Two deterministic 16 kHz clips: three drifting tones under an envelope plus noise, peak about 0.3."""
    out = []
    for b, n in enumerate(CLIP_SAMPLES):
        g = np.random.default_rng(4321 + b)
        t = np.arange(n) / 16000.0
        x = sum(a * np.sin(2 * np.pi * (f0 + 40.0 * b) * t * (1 + 0.1 * t) + p)
                for a, f0, p in ((0.12, 180.0, 0.3), (0.08, 740.0, 1.1), (0.05, 2310.0, 2.0)))
        x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.03 * g.standard_normal(n)
        out.append(x.astype(np.float32))
    return out


def weights(geom, seed=0):
    """``Wav2Vec2ForCTC.state_dict()`` names -> float32 arrays: O(1 / sqrt(fan_in)) matrices, perturbed norm gains, a weight-normed
    positional conv whose g is NOT the norm of v (so a fold that ignores g fails), and the head gain."""
    cfg = GEOMS[geom]
    H, F, C, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["conv_dim"], cfg["num_hidden_layers"]
    cg = H // 16
    g = np.random.default_rng(1000 * seed + (7 if geom == "a" else 11))
    rn = lambda *s, std=1.0: (g.standard_normal(s) * std).astype(np.float32)
    sd = {}
    fe = "wav2vec2.feature_extractor.conv_layers."
    sd[fe + "0.conv.weight"] = rn(C, 1, 10, std=1 / np.sqrt(10))
    sd[fe + "0.layer_norm.weight"], sd[fe + "0.layer_norm.bias"] = 1 + rn(C, std=0.1), rn(C, std=0.1)
    for i in range(1, 7):
        sd[fe + f"{i}.conv.weight"] = rn(C, C, CONV_KERNEL[i], std=np.sqrt(2.0 / (CONV_KERNEL[i] * C)))
    fp = "wav2vec2.feature_projection."
    sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"] = 1 + rn(C, std=0.1), rn(C, std=0.02)
    sd[fp + "projection.weight"], sd[fp + "projection.bias"] = rn(H, C, std=1 / np.sqrt(C)), rn(H, std=0.02)
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    v = rn(H, cg, 128, std=1.0)
    sd[pc + "parametrizations.weight.original1"] = v
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


def hf_model(geom, sd):
    """A transformers ``Wav2Vec2ForCTC`` (CPU, fp32, eval, eager attention) carrying ``sd``."""
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    cfg = GEOMS[geom]
    c = Wav2Vec2Config(vocab_size=N_CLASSES, hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                       num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                       conv_dim=(cfg["conv_dim"],) * 7, conv_kernel=CONV_KERNEL, conv_stride=CONV_STRIDE, feat_extract_norm="group",
                       conv_bias=False, do_stable_layer_norm=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                       layer_norm_eps=1e-5, hidden_act="gelu", feat_extract_activation="gelu", attn_implementation="eager")
    m = Wav2Vec2ForCTC(c).eval()
    r = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not r.unexpected_keys and set(r.missing_keys) <= {"wav2vec2.masked_spec_embed"}, r
    return m

"""The seeded inputs of the Whisper-tower fixtures (tests/golden/make_whisper_fixture.py) and of the tests that read them.

The weights are plain numpy draws, so the fixtures hold only what transformers computed from them: the tests rebuild the very same
arrays from the seed instead of carrying 2 MB of random numbers in git.
"""
import numpy as np

SMALL = dict(d_model=128, encoder_attention_heads=2, encoder_ffn_dim=256, encoder_layers=2, num_mel_bins=80, max_source_positions=1500)
CLIP_SAMPLES = (160000, 3 * 16000 + 77)          # a 10 s clip and a 3 s + 77 sample clip


def waves():
    """0.1 * N(0, 1), RandomState(1234 + b): the synthetic clips the other fixtures use (oracle/weights.py synthetic_wave)."""
    return [(0.1 * np.random.RandomState(1234 + b).standard_normal(n)).astype(np.float32) for b, n in enumerate(CLIP_SAMPLES)]


def sinusoids(length, channels, max_timescale=10000.0):
    inc = np.log(max_timescale) / (channels // 2 - 1)
    inv = np.exp(-inc * np.arange(channels // 2))
    t = np.arange(length)[:, None] * inv[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32)


def encoder_weights(cfg=SMALL, seed=0, perturb_positions=True):
    """``WhisperEncoder.state_dict()`` names -> float32 arrays.  O(1 / sqrt(fan_in)) matrices and perturbed LayerNorm gains (HF's
    std-0.02 init would hide errors behind the residual), and a position table that is NOT symmetric under a shift or a transpose."""
    rs = np.random.RandomState(seed)
    H, F, M, L, P = cfg["d_model"], cfg["encoder_ffn_dim"], cfg["num_mel_bins"], cfg["encoder_layers"], cfg["max_source_positions"]
    rn = lambda *s, std=1.0: (rs.standard_normal(s) * std).astype(np.float32)
    sd = {"conv1.weight": rn(H, M, 3, std=1 / np.sqrt(3 * M)), "conv1.bias": rn(H, std=0.02),
          "conv2.weight": rn(H, H, 3, std=1 / np.sqrt(3 * H)), "conv2.bias": rn(H, std=0.02),
          "layer_norm.weight": 1 + rn(H, std=0.1), "layer_norm.bias": rn(H, std=0.02)}
    pos = sinusoids(P, H)
    if perturb_positions:
        pos = pos + rn(P, H, std=0.1)
    sd["embed_positions.weight"] = pos.astype(np.float32)
    for i in range(L):
        p, a = f"layers.{i}.", f"layers.{i}.self_attn."
        for n in ("q_proj", "k_proj", "v_proj"):
            sd[a + n + ".weight"] = rn(H, H, std=1 / np.sqrt(H))
        sd[a + "q_proj.bias"], sd[a + "v_proj.bias"] = rn(H, std=0.02), rn(H, std=0.02)
        sd[a + "out_proj.weight"], sd[a + "out_proj.bias"] = rn(H, H, std=0.5 / np.sqrt(H)), rn(H, std=0.02)
        sd[p + "fc1.weight"], sd[p + "fc1.bias"] = rn(F, H, std=1 / np.sqrt(H)), rn(F, std=0.02)
        sd[p + "fc2.weight"], sd[p + "fc2.bias"] = rn(H, F, std=0.5 / np.sqrt(F)), rn(H, std=0.02)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + rn(H, std=0.1), rn(H, std=0.02)
    return sd


def hf_encoder(cfg, sd):
    """A transformers ``WhisperEncoder`` (CPU, fp32, eval) carrying ``sd``."""
    import torch
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    c = WhisperConfig(**cfg, decoder_layers=1, decoder_attention_heads=cfg["encoder_attention_heads"], decoder_ffn_dim=64)
    c._attn_implementation = "eager"
    enc = WhisperEncoder(c).eval()
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    return enc

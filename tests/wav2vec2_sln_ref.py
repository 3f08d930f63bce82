"""The definition of the layer-norm / stable wav2vec2 CTC model the library computes ("wav2vec2 acoustic model:
the layer-norm / stable family"): a float64 restatement of ``Wav2Vec2ForCTC`` (TF:models/wav2vec2/modeling_wav2vec2.py) with
feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, no attention mask, on ONE unpadded clip, with the optional
zero-mean / unit-variance input.  The pieces the two families share come from tests/wav2vec2_ref.py.
"""
import numpy as np
import torch

from tests.wav2vec2_ref import (CONV_STRIDE, F64, _t, conv_valid, frames_of, gelu, head_rows, layer_norm, pos_conv_add,  # noqa: F401
                                pos_conv_weight)

CONV_LN_EPS = 1e-5                      # nn.LayerNorm's default: Wav2Vec2LayerNormConvLayer does not pass config.layer_norm_eps
INPUT_NORM_EPS = {"hf": 1e-7, "torchaudio": 1e-5}


def normalize_input(wav, eps):
    """(x - mean) / sqrt(var + eps) over the clip's own samples, biased variance."""
    x = _t(wav)
    m = x.mean()
    return (x - m) / torch.sqrt(((x - m) ** 2).mean() + eps)


def conv_ln_gelu(x, w, b, ln_w, ln_b, stride, eps=CONV_LN_EPS):
    """One ``Wav2Vec2LayerNormConvLayer`` on time-major x [T, Cin]: conv + bias, LayerNorm over the channels of each frame, GELU."""
    return gelu(layer_norm(conv_valid(x, w, stride) + _t(b), ln_w, ln_b, eps))


def conv0_ln_gelu(wav, w0, b0, ln_w, ln_b, eps=CONV_LN_EPS):
    return conv_ln_gelu(_t(wav).reshape(-1, 1), w0, b0, ln_w, ln_b, CONV_STRIDE[0], eps)


def feature_extractor(sd, wav):
    fe = "wav2vec2.feature_extractor.conv_layers."
    x = _t(wav).reshape(-1, 1)
    for i in range(7):
        p = fe + f"{i}."
        x = conv_ln_gelu(x, sd[p + "conv.weight"], sd[p + "conv.bias"], sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], CONV_STRIDE[i])
    return x


def encoder_layer(sd, i, x, heads, eps=1e-5):
    """``Wav2Vec2EncoderLayerStableLayerNorm``: x += out_proj(attn(layer_norm(x))); x += ffn(final_layer_norm(x))."""
    p = f"wav2vec2.encoder.layers.{i}."
    T, H = x.shape
    hd = H // heads
    lin = lambda n, v: v @ _t(sd[p + n + ".weight"]).T + _t(sd[p + n + ".bias"])
    h = layer_norm(x, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], eps)
    q = (lin("attention.q_proj", h) * hd ** -0.5).reshape(T, heads, hd).transpose(0, 1)
    k = lin("attention.k_proj", h).reshape(T, heads, hd).transpose(0, 1)
    v = lin("attention.v_proj", h).reshape(T, heads, hd).transpose(0, 1)
    a = torch.softmax(q @ k.transpose(1, 2), -1) @ v
    x = x + lin("attention.out_proj", a.transpose(0, 1).reshape(T, H))
    h = layer_norm(x, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)
    return x + lin("feed_forward.output_dense", gelu(lin("feed_forward.intermediate_dense", h)))


def forward(sd, wav, heads, n_layers, labels="hf", want=(), normalize=None, eps=1e-5):
    """One clip -> logits [T, n_classes] float64 (and, in a dict, the intermediates named in ``want``: feat, pos, layer0).
    ``normalize``: None | "hf" | "torchaudio"."""
    inter = {}
    x = normalize_input(wav, INPUT_NORM_EPS[normalize]) if normalize is not None else _t(wav)
    feat = feature_extractor(sd, x)
    inter["feat"] = feat
    fp = "wav2vec2.feature_projection."
    x = layer_norm(feat, sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"], eps) @ _t(sd[fp + "projection.weight"]).T + _t(sd[fp + "projection.bias"])
    x = pos_conv_add(x, pos_conv_weight(sd), sd["wav2vec2.encoder.pos_conv_embed.conv.bias"])          # no LayerNorm here
    inter["pos"] = x
    for i in range(n_layers):
        x = encoder_layer(sd, i, x, heads, eps)
        if i == 0:
            inter["layer0"] = x
    x = layer_norm(x, sd["wav2vec2.encoder.layer_norm.weight"], sd["wav2vec2.encoder.layer_norm.bias"], eps)
    rows = head_rows(np.asarray(sd["lm_head.weight"]).shape[0], labels)
    logits = x @ _t(sd["lm_head.weight"])[rows].T + _t(sd["lm_head.bias"])[rows]
    return (logits, {k: inter[k] for k in want}) if want else logits


def emissions(sd, wav, heads, n_layers, labels="hf", normalize=None):
    return torch.log_softmax(forward(sd, wav, heads, n_layers, labels, normalize=normalize), -1)

"""The definition of the wav2vec2 CTC acoustic model the library computes ("wav2vec2 acoustic model"): a float64
restatement of ``Wav2Vec2ForCTC`` (TF:models/wav2vec2/modeling_wav2vec2.py) with feat_extract_norm="group", conv_bias=False,
do_stable_layer_norm=False, no attention mask, no input normalisation, on ONE unpadded clip.  Weights come under transformers'
parameter names as numpy arrays (tests/golden/wav2vec2_recipe.py); everything is plain index arithmetic and matmuls in float64.
"""
import math

import numpy as np
import torch

CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
POS_KERNEL, POS_GROUPS = 128, 16
F64 = torch.float64


def frames_of(n):
    """(T - k) // s + 1 per convolution; 0 once a layer has fewer inputs than taps."""
    for k, s in zip(CONV_KERNEL, CONV_STRIDE):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def _t(a):
    return torch.as_tensor(np.asarray(a)).to(F64)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps=1e-5):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * _t(w) + _t(b)


def conv_valid(x, w, stride):
    """x [T, Cin] time-major, w [Cout, Cin, k] -> [(T - k) // stride + 1, Cout]: out[t, co] = sum_{tap, ci} x[t stride + tap, ci] w[co, ci, tap]."""
    w = _t(w)
    k = w.shape[2]
    T = (x.shape[0] - k) // stride + 1
    win = torch.stack([x[tap: tap + (T - 1) * stride + 1: stride] for tap in range(k)], 0)       # [k, T, Cin]
    return torch.einsum("ktc,ock->to", win, w)


def conv0_gn_gelu(wav, w0, gn_w, gn_b, eps=1e-5):
    """Conv layer 0 on a 1-D clip, GroupNorm with one group per channel (statistics over the clip's own frames, biased variance), GELU."""
    y = conv_valid(_t(wav).reshape(-1, 1), w0, CONV_STRIDE[0])
    m = y.mean(0, keepdim=True)
    v = ((y - m) ** 2).mean(0, keepdim=True)
    return gelu((y - m) / torch.sqrt(v + eps) * _t(gn_w) + _t(gn_b))


def feature_extractor(sd, wav):
    fe = "wav2vec2.feature_extractor.conv_layers."
    x = conv0_gn_gelu(wav, sd[fe + "0.conv.weight"], sd[fe + "0.layer_norm.weight"], sd[fe + "0.layer_norm.bias"])
    for i in range(1, 7):
        x = gelu(conv_valid(x, sd[fe + f"{i}.conv.weight"], CONV_STRIDE[i]))
    return x


def fold_weight_norm(g, v):
    """weight_norm(dim=2): w[:, :, tap] = g[tap] v[:, :, tap] / ||v[:, :, tap]||."""
    g, v = _t(g), _t(v)
    return v * (g.reshape(1, 1, -1) / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True)))


def pos_conv_weight(sd):
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    if pc + "parametrizations.weight.original0" in sd:
        return fold_weight_norm(sd[pc + "parametrizations.weight.original0"], sd[pc + "parametrizations.weight.original1"])
    if pc + "weight_g" in sd:
        return fold_weight_norm(sd[pc + "weight_g"], sd[pc + "weight_v"])
    return _t(sd[pc + "weight"])


def pos_conv_add(x, w, bias):
    """x [T, H] -> x + gelu(conv(x) + b): Conv1d(H, H, 128, padding 64, groups 16) keeps T + 1 frames, the last is dropped, so
    out[t, g cg + co] = sum_{tap, ci} x[t + tap - 64, g cg + ci] w[g cg + co, ci, tap] over 0 <= t + tap - 64 < T, t in [0, T)."""
    x, w = _t(x), _t(w)
    T, H = x.shape
    cg = H // POS_GROUPS
    xp = torch.zeros(T + POS_KERNEL, H, dtype=F64)
    xp[POS_KERNEL // 2: POS_KERNEL // 2 + T] = x
    win = torch.stack([xp[tap: tap + T] for tap in range(POS_KERNEL)], 0).reshape(POS_KERNEL, T, POS_GROUPS, cg)     # [tap, t, g, ci]
    y = torch.einsum("ktgc,gock->tgo", win, w.reshape(POS_GROUPS, cg, cg, POS_KERNEL)).reshape(T, H)
    return x + gelu(y + _t(bias))


def encoder_layer(sd, i, x, heads):
    p = f"wav2vec2.encoder.layers.{i}."
    T, H = x.shape
    hd = H // heads
    lin = lambda n, v: v @ _t(sd[p + n + ".weight"]).T + _t(sd[p + n + ".bias"])
    q = (lin("attention.q_proj", x) * hd ** -0.5).reshape(T, heads, hd).transpose(0, 1)
    k = lin("attention.k_proj", x).reshape(T, heads, hd).transpose(0, 1)
    v = lin("attention.v_proj", x).reshape(T, heads, hd).transpose(0, 1)
    a = torch.softmax(q @ k.transpose(1, 2), -1) @ v
    x = x + lin("attention.out_proj", a.transpose(0, 1).reshape(T, H))
    x = layer_norm(x, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"])
    x = x + lin("feed_forward.output_dense", gelu(lin("feed_forward.intermediate_dense", x)))
    return layer_norm(x, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"])


def head_rows(n_rows, labels):
    if labels == "hf":
        return list(range(n_rows))
    assert labels == "torchaudio" and n_rows == 32
    return [0] + list(range(4, 32))


def forward(sd, wav, heads, n_layers, labels="hf", want=()):
    """One clip -> logits [T, n_classes] float64 (and, in a dict, the intermediates named in ``want``: feat, pos, layer0)."""
    inter = {}
    feat = feature_extractor(sd, wav)
    inter["feat"] = feat
    fp = "wav2vec2.feature_projection."
    x = layer_norm(feat, sd[fp + "layer_norm.weight"], sd[fp + "layer_norm.bias"]) @ _t(sd[fp + "projection.weight"]).T + _t(sd[fp + "projection.bias"])
    x = pos_conv_add(x, pos_conv_weight(sd), sd["wav2vec2.encoder.pos_conv_embed.conv.bias"])
    x = layer_norm(x, sd["wav2vec2.encoder.layer_norm.weight"], sd["wav2vec2.encoder.layer_norm.bias"])
    inter["pos"] = x
    for i in range(n_layers):
        x = encoder_layer(sd, i, x, heads)
        if i == 0:
            inter["layer0"] = x
    rows = head_rows(np.asarray(sd["lm_head.weight"]).shape[0], labels)
    logits = x @ _t(sd["lm_head.weight"])[rows].T + _t(sd["lm_head.bias"])[rows]
    return (logits, {k: inter[k] for k in want}) if want else logits


def emissions(sd, wav, heads, n_layers, labels="hf"):
    return torch.log_softmax(forward(sd, wav, heads, n_layers, labels), -1)

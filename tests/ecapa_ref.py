"""The definition of the ECAPA-TDNN speaker-embedding model the library computes ("Speaker diarization"): a numpy
float64 restatement of SpeechBrain's Fbank + sentence-mean normalisation + ``ECAPA_TDNN`` at the ``spkrec-ecapa-voxceleb``
hyper-parameters, on ONE window.  Weights come under SpeechBrain's parameter names as numpy arrays (tests/golden/ecapa_recipe.py);
activations are time-major [T, C]; everything is plain index arithmetic and matmuls in float64.
"""
import numpy as np

N_FFT, HOP, N_BINS, N_MELS, SAMPLE_RATE = 400, 160, 201, 80, 16000
SCALE = 8
BN_EPS = 1e-5


def frames_of(n):
    return n // HOP + 1


def _a(x):
    return np.asarray(x, dtype=np.float64)


# ----------------------------------------------------------------------------- features
def reflect_extend(chunk, window_samples):
    """A chunk shorter than the window, extended on the right by reflection: sample len + i = sample len - 2 - i."""
    chunk = _a(chunk)
    pad = window_samples - len(chunk)
    assert 0 <= pad <= len(chunk) - 1
    return np.pad(chunk, (0, pad), mode="reflect") if pad else chunk


def hamming_window():
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def mel_filterbank():
    """[201, 80]: edges equally spaced on 2595 log10(1 + f / 700) from 0 to 8000 Hz; triangles built in Hz."""
    mel_hi = 2595.0 * np.log10(1.0 + (SAMPLE_RATE / 2.0) / 700.0)
    hz = 700.0 * (10.0 ** (np.linspace(0.0, mel_hi, N_MELS + 2) / 2595.0) - 1.0)
    band, centre = (hz[1:] - hz[:-1])[:-1], hz[1:-1]
    f = np.linspace(0.0, SAMPLE_RATE / 2.0, N_BINS)
    slope = (f[:, None] - centre[None, :]) / band[None, :]
    return np.maximum(0.0, np.minimum(slope + 1.0, -slope + 1.0))


def log_mel(wav):
    """wav [L] -> [T, 80] dB, T = L // 160 + 1: centred STFT with ZERO padding, power, mel, 10 log10(max(x, 1e-10)), floor at the
    window's own maximum - 80 dB."""
    wav = _a(wav)
    T = frames_of(len(wav))
    x = np.concatenate([np.zeros(N_FFT // 2), wav, np.zeros(N_FFT // 2)])
    frames = np.stack([x[t * HOP:t * HOP + N_FFT] for t in range(T)]) * hamming_window()
    spec = np.fft.rfft(frames, axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    db = 10.0 * np.log10(np.maximum(power @ mel_filterbank(), 1e-10))
    return np.maximum(db, db.max() - 80.0)


def fbank(wav):
    """Normalised features [T, 80]: ``log_mel`` minus each mel bin's mean over the window's frames."""
    db = log_mel(wav)
    return db - db.mean(0, keepdims=True)


# ----------------------------------------------------------------------------- network
def fold_bn(sd, prefix, eps=BN_EPS):
    scale = _a(sd[prefix + "weight"]) / np.sqrt(_a(sd[prefix + "running_var"]) + eps)
    return scale, _a(sd[prefix + "bias"]) - _a(sd[prefix + "running_mean"]) * scale


def conv1d(x, w, b, dilation=1):
    """x [T, Cin], w [Cout, Cin, k], reflect padding (k - 1) d / 2 -> [T, Cout]."""
    x, w = _a(x), _a(w)
    k = w.shape[2]
    pad = (k - 1) * dilation // 2
    xp = np.pad(x, ((pad, pad), (0, 0)), mode="reflect") if pad else x
    T = x.shape[0]
    out = np.zeros((T, w.shape[0])) + (_a(b) if b is not None else 0.0)
    for tap in range(k):
        out += xp[tap * dilation:tap * dilation + T] @ w[:, :, tap].T
    return out


def relu(x):
    return np.maximum(x, 0.0)


def tdnn(x, sd, prefix, dilation=1):
    """Conv1d (reflect), ReLU, eval-mode BatchNorm."""
    s, t = fold_bn(sd, prefix + "norm.norm.")
    return relu(conv1d(x, sd[prefix + "conv.conv.weight"], sd[prefix + "conv.conv.bias"], dilation)) * s + t


def res2net(x, sd, prefix, dilation):
    w = x.shape[1] // SCALE
    ys = []
    for i in range(SCALE):
        xi = x[:, i * w:(i + 1) * w]
        if i == 0:
            y = xi
        elif i == 1:
            y = tdnn(xi, sd, prefix + "blocks.0.", dilation)
        else:
            y = tdnn(xi + y, sd, prefix + f"blocks.{i - 1}.", dilation)
        ys.append(y)
    return np.concatenate(ys, 1)


def se_gate(mean, sd, prefix):
    h = relu(_a(sd[prefix + "conv1.conv.weight"])[:, :, 0] @ mean + _a(sd[prefix + "conv1.conv.bias"]))
    return 1.0 / (1.0 + np.exp(-(_a(sd[prefix + "conv2.conv.weight"])[:, :, 0] @ h + _a(sd[prefix + "conv2.conv.bias"]))))


def se_res2net_block(x, sd, prefix, dilation):
    y = tdnn(res2net(tdnn(x, sd, prefix + "tdnn1."), sd, prefix + "res2net_block.", dilation), sd, prefix + "tdnn2.")
    return x + y * se_gate(y.mean(0), sd, prefix + "se_block.")[None, :]


def softmax_time(z):
    e = np.exp(z - z.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def weighted_stats(h, a):
    """a-weighted mean and sqrt(max(variance, 1e-12)) over time, per channel."""
    m = (a * h).sum(0)
    return m, np.sqrt(np.maximum((a * (h - m) ** 2).sum(0), 1e-12))


def attentive_pool(h, sd):
    """-> (pooled [6C] = weighted mean | std, attention weights [T, 3C])."""
    T = h.shape[0]
    m, s = weighted_stats(h, np.full_like(h, 1.0 / T))
    att_in = np.concatenate([h, np.tile(m, (T, 1)), np.tile(s, (T, 1))], 1)
    a = softmax_time(conv1d(np.tanh(tdnn(att_in, sd, "asp.tdnn.")), sd["asp.conv.conv.weight"], sd["asp.conv.conv.bias"]))
    return np.concatenate(weighted_stats(h, a)), a


def forward(sd, feats, dilations=(2, 3, 4)):
    """feats [T, 80] -> dict: block0, blk1, blk2, blk3 [T, C], mfa [T, 3C], attn [T, 3C], pooled [6C], emb [D]."""
    out = {}
    x = out["block0"] = tdnn(_a(feats), sd, "blocks.0.")
    xs = []
    for i, d in enumerate(dilations, start=1):
        x = out[f"blk{i}"] = se_res2net_block(x, sd, f"blocks.{i}.", d)
        xs.append(x)
    h = out["mfa"] = tdnn(np.concatenate(xs, 1), sd, "mfa.")
    out["pooled"], out["attn"] = attentive_pool(h, sd)
    s, t = fold_bn(sd, "asp_bn.norm.")
    out["emb"] = _a(sd["fc.conv.weight"])[:, :, 0] @ (out["pooled"] * s + t) + _a(sd["fc.conv.bias"])
    return out


def embed(sd, wav, dilations=(2, 3, 4)):
    return forward(sd, fbank(wav), dilations)["emb"]


def conv3_reflect(u, w, b, dilation):
    """The k = 3 dilated convolution of one Res2Net sub-band on a given operand u [T, w] (pre-activation, float64)."""
    return conv1d(u, w, b, dilation)

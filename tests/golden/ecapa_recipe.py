"""The seeded inputs of the ECAPA-TDNN fixtures (tests/golden/make_ecapa_fixture.py) and of the tests that read them.

The weights and windows are plain numpy ``Generator`` draws, so the fixtures hold only what torch computed from them: the tests rebuild
the very same arrays from the seed instead of carrying them in git.  ``torch_model`` is a composition of torch's own modules
(``nn.Conv1d(padding_mode="reflect")``, ``nn.BatchNorm1d``) whose attribute names follow SpeechBrain's ``ECAPA_TDNN`` layout, so that
a SpeechBrain-named state dict loads into it strictly; SpeechBrain itself is not installed where the fixtures are made.
"""
import functools

import numpy as np

N_MELS, SCALE = 80, 8
DILATIONS = (2, 3, 4)
ATTENTION_GAIN = 3.0      # asp.conv.weight is multiplied by this: at unit gain the attention is nearly flat and a broken softmax invisible
FC_GAIN = 1.0
# (a) 16 channels per Res2Net sub-band, with intermediates; (full) the widths of speechbrain/spkrec-ecapa-voxceleb, embeddings only
GEOMS = {
    "a": dict(channels=128, se_channels=32, attention_channels=64, lin_neurons=64),
    "full": dict(channels=1024, se_channels=128, attention_channels=128, lin_neurons=192),
}
WINDOW_SAMPLES = (12000, 3333, 640)       # T = 76; 21 (not a multiple of the hop); 5 (the minimum for the reflect padding of 4)
FEATURE_CHUNK = 7000                      # the feature test's fourth input: a 7000-sample chunk reflected to 12000


def frames_of(n):
    return n // 160 + 1


def _voice(n, seed, f0, noise):
    """A deterministic 16 kHz signal: three gliding, amplitude-modulated partials over a noise floor."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = sum(a * np.sin(2 * np.pi * f * t * (1 + r * t) + p) * (0.55 + 0.45 * np.sin(2 * np.pi * fm * t + p))
            for a, f, r, fm, p in ((0.20, f0, 0.6, 7.0, 0.3), (0.12, 3.1 * f0, -0.4, 11.0, 1.1), (0.07, 7.3 * f0, 0.9, 17.0, 2.0)))
    return x + noise * g.standard_normal(n)


def windows():
    """Three windows for the whole-model fixtures (a 0.03 noise floor keeps every mel bin far above f32 cancellation); window 1 rides
    on a DC offset."""
    out = []
    for i, n in enumerate(WINDOW_SAMPLES):
        x = _voice(n, 4321 + i, (170.0, 260.0, 390.0)[i], 0.03)
        out.append((x + (0.1 if i == 1 else 0.0)).astype(np.float32))
    return out


def feature_windows():
    """The feature test's inputs as (chunk, window_samples): the three window lengths and a 7000-sample chunk that is reflected to
    12000, all over a 1e-3 noise floor (no bin sits on the 1e-10 clamp); window 1 rides on a DC offset."""
    out = []
    for i, n in enumerate(WINDOW_SAMPLES + (FEATURE_CHUNK,)):
        x = _voice(n, 8765 + i, (150.0, 230.0, 410.0, 190.0)[i], 1e-3)
        out.append(((x + (0.05 if i == 1 else 0.0)).astype(np.float32), 12000 if n == FEATURE_CHUNK else n))
    return out


@functools.lru_cache(maxsize=None)
def _weights(geom, seed):
    sd = _draw(geom, seed)
    # asp_bn's running mean is calibrated on the recipe's own windows, as training would have: with a drawn mean the pooled vector's
    # input-independent part dominates and every window embeds alike (cosine 0.99).  The running variance stays 1: dividing by the
    # variance over three windows would blow up the directions in which the windows barely differ and with them the rounding noise
    # (on the CPU the bf16 module's 1 - cosine was 3.4e-3 .. 1.5e-2 with var + 0.05 against 0.9e-3 .. 7.6e-3 without whitening).
    # What is left is the centring itself: the windows differ by about a seventh of the pooled vector's norm, so every rounding
    # upstream shows about seven times as large in the embedding -- the yardstick's relmax is 5 to 14 %, not the 0.5 % of an
    # uncentred model, and the device is held to 1.5x of THAT
    from tests import ecapa_ref as REF
    pooled = np.stack([REF.forward(sd, REF.fbank(w), DILATIONS)["pooled"] for w in windows()])
    sd["asp_bn.norm.running_mean"] = pooled.mean(0).astype(np.float32)
    sd["asp_bn.norm.running_var"] = np.ones(pooled.shape[1], np.float32)
    return sd


def weights(geom, seed=0):
    """SpeechBrain ``ECAPA_TDNN.state_dict()`` names -> float32 arrays: He-scaled convolutions, biases, BatchNorm layers with
    perturbed gains and running statistics (so a fold that ignores one of the four fails), the attention gain, and ``asp_bn``
    calibrated on ``windows()``.  The arrays are shared between callers: do not write into them."""
    return dict(_weights(geom, seed))


def _draw(geom, seed):
    cfg = GEOMS[geom]
    C, se, A, D = cfg["channels"], cfg["se_channels"], cfg["attention_channels"], cfg["lin_neurons"]
    w = C // SCALE
    g = np.random.default_rng(1000 * seed + (7 if geom == "a" else 11))
    rn = lambda *s, std=1.0: (g.standard_normal(s) * std).astype(np.float32)
    sd = {}

    def conv(name, o, i, k, gain=1.0):
        sd[name + "weight"], sd[name + "bias"] = rn(o, i, k, std=gain * np.sqrt(2.0 / (i * k))), rn(o, std=0.1)

    def bn(name, n):
        sd[name + "weight"], sd[name + "bias"] = (0.8 + 0.4 * g.random(n)).astype(np.float32), rn(n, std=0.1)
        sd[name + "running_mean"], sd[name + "running_var"] = rn(n, std=0.1), (0.5 + g.random(n)).astype(np.float32)

    def tdnn(p, o, i, k, gain=1.0):
        conv(p + "conv.conv.", o, i, k, gain)
        bn(p + "norm.norm.", o)

    tdnn("blocks.0.", C, N_MELS, 5, gain=0.1)            # the features are dB values of order 10
    for b in (1, 2, 3):
        p = f"blocks.{b}."
        tdnn(p + "tdnn1.", C, C, 1)
        for m in range(SCALE - 1):
            tdnn(p + f"res2net_block.blocks.{m}.", w, w, 3)
        tdnn(p + "tdnn2.", C, C, 1)
        conv(p + "se_block.conv1.conv.", se, C, 1)
        conv(p + "se_block.conv2.conv.", C, se, 1)
    tdnn("mfa.", 3 * C, 3 * C, 1)
    tdnn("asp.tdnn.", A, 9 * C, 1)
    conv("asp.conv.conv.", 3 * C, A, 1, gain=ATTENTION_GAIN)
    bn("asp_bn.norm.", 6 * C)
    conv("fc.conv.", D, 6 * C, 1, gain=FC_GAIN)
    return sd


def torch_model(geom, sd):
    """The network as a composition of torch modules (CPU, fp32, eval) carrying ``sd``; ``model(feats [N, 80, T]) -> dict`` with
    time-major intermediates of window 0 .. N - 1."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    cfg = GEOMS[geom]
    C, se, A, D = cfg["channels"], cfg["se_channels"], cfg["attention_channels"], cfg["lin_neurons"]

    class Conv(nn.Module):
        def __init__(s, i, o, k, d=1):
            super().__init__()
            s.conv = nn.Conv1d(i, o, k, dilation=d, padding=(k - 1) * d // 2, padding_mode="reflect")

        def forward(s, x):
            return s.conv(x)

    class Norm(nn.Module):
        def __init__(s, n):
            super().__init__()
            s.norm = nn.BatchNorm1d(n)

        def forward(s, x):
            return s.norm(x)

    class TDNN(nn.Module):
        def __init__(s, i, o, k, d=1):
            super().__init__()
            s.conv, s.norm = Conv(i, o, k, d), Norm(o)

        def forward(s, x):
            return s.norm(F.relu(s.conv(x)))

    class Res2Net(nn.Module):
        def __init__(s, c, d):
            super().__init__()
            s.blocks = nn.ModuleList([TDNN(c // SCALE, c // SCALE, 3, d) for _ in range(SCALE - 1)])

        def forward(s, x):
            ys = []
            for i, xi in enumerate(torch.chunk(x, SCALE, 1)):
                y = xi if i == 0 else s.blocks[i - 1](xi if i == 1 else xi + y)
                ys.append(y)
            return torch.cat(ys, 1)

    class SE(nn.Module):
        def __init__(s, c, n):
            super().__init__()
            s.conv1, s.conv2 = Conv(c, n, 1), Conv(n, c, 1)

        def forward(s, x):
            return x * torch.sigmoid(s.conv2(F.relu(s.conv1(x.mean(2, keepdim=True)))))

    class Block(nn.Module):
        def __init__(s, c, n, d):
            super().__init__()
            s.tdnn1, s.res2net_block, s.tdnn2, s.se_block = TDNN(c, c, 1), Res2Net(c, d), TDNN(c, c, 1), SE(c, n)

        def forward(s, x):
            return x + s.se_block(s.tdnn2(s.res2net_block(s.tdnn1(x))))

    class ASP(nn.Module):
        def __init__(s, c, a):
            super().__init__()
            s.tdnn, s.conv = TDNN(3 * c, a, 1), Conv(a, c, 1)

        def forward(s, x):
            m = x.mean(2, keepdim=True)
            sd_ = (x - m).pow(2).mean(2, keepdim=True).clamp(1e-12).sqrt()
            w = torch.softmax(s.conv(torch.tanh(s.tdnn(torch.cat([x, m.expand_as(x), sd_.expand_as(x)], 1)))), 2)
            m = (w * x).sum(2)
            sd_ = (w * (x - m[..., None]).pow(2)).sum(2).clamp(1e-12).sqrt()
            return torch.cat([m, sd_], 1)[..., None], w

    class Ecapa(nn.Module):
        def __init__(s):
            super().__init__()
            s.blocks = nn.ModuleList([TDNN(N_MELS, C, 5)] + [Block(C, se, d) for d in DILATIONS])
            s.mfa, s.asp, s.asp_bn, s.fc = TDNN(3 * C, 3 * C, 1), ASP(3 * C, A), Norm(6 * C), Conv(6 * C, D, 1)

        def forward(s, f):
            out = {}
            x = out["block0"] = s.blocks[0](f)
            xs = []
            for i in (1, 2, 3):
                x = out[f"blk{i}"] = s.blocks[i](x)
                xs.append(x)
            h = out["mfa"] = s.mfa(torch.cat(xs, 1))
            p, out["attn"] = s.asp(h)
            out["pooled"] = p[..., 0]
            out["emb"] = s.fc(s.asp_bn(p))[..., 0]
            return {k: (v.transpose(1, 2) if v.dim() == 3 else v) for k, v in out.items()}

    m = Ecapa().eval()
    r = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    assert not r.unexpected_keys and all(k.endswith("num_batches_tracked") for k in r.missing_keys), r
    return m


def torch_fbank(wav):
    """f32 features of one window through ``torch.stft`` (centre, zero padding, periodic Hamming) -> tensor [T, 80]: the feature
    kernel's yardstick is this against the float64 definition on the same input."""
    import torch
    from tests import ecapa_ref as REF
    x = torch.as_tensor(np.asarray(wav, np.float32))
    win = torch.from_numpy(REF.hamming_window()).float()
    spec = torch.stft(x, 400, hop_length=160, win_length=400, window=win, center=True, pad_mode="constant", return_complex=True)
    power = (spec.real ** 2 + spec.imag ** 2).T                                   # [T, 201]
    db = 10.0 * torch.log10(torch.clamp(power @ torch.from_numpy(REF.mel_filterbank()).float(), min=1e-10))
    db = torch.maximum(db, db.max() - 80.0)
    return db - db.mean(0, keepdim=True)

"""-m gpu: the wav2vec2 CTC acoustic model on the device (csrc/wav2vec2.hip, tiny_audio_amd/wav2vec2.py) against the float64 definition
(tests/wav2vec2_ref.py) and against transformers' own outputs (tests/golden/wav2vec2_{a,b}.npz).

Bounds.  The new kernels are measured against the definition evaluated on the very operands the kernel reads, so what is left is the
output rounding (bf16 keeps 8 significant bits: half an ulp is up to 2^-8 of the value) plus f32 arithmetic; each test states its own.  The whole model is measured against
the fp32 fixture with transformers' bf16 module ON THE SAME INPUT as the yardstick (read from the fixture, never from the code under
test): the device keeps fp32 accumulators, norms and softmax but has three roundings that module lacks (the table GELU, the log2(e)
fold, the bf16 conv activations), so it gets 1.5x the yardstick's relmax, 1.5x its (1 - cosine) and 1.5x its max |d log-prob|.

Figures measured on MI355X (profiles/wav2vec2.md has the full table): see ``test_whole_model_against_transformers``.
"""
import os

import numpy as np
import pytest
import torch

from tests import align_ref
from tests import wav2vec2_ref as REF
from tests.golden import wav2vec2_recipe as R
from tiny_audio_amd import ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import ForcedAligner

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
MARGIN = 1.5


def bf16_round(a):
    return torch.as_tensor(np.asarray(a)).to(F32).to(BF16).to(F64)


def model(geom, res_f32=False, n_classes=32, labels="hf"):
    m = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**R.GEOMS[geom], n_classes=n_classes), device=DEV)
    m.load_state_dict_hf(R.weights(geom), labels=labels)
    m.res_f32 = res_f32
    return m


def clip(n, seed):
    """A deterministic 16 kHz clip of n samples: two tones, noise and a DC offset."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.15 * np.sin(2 * np.pi * 220.0 * t + seed) + 0.07 * np.sin(2 * np.pi * 1900.0 * t) + 0.03 * g.standard_normal(n) + 0.02).astype(np.float32)


# ----------------------------------------------------------------------------- conv 0 + GroupNorm + GELU
def test_conv0_groupnorm_gelu_each_clip_alone():
    """C = 128; lengths 400 (T0 = 79), 401, 3217, 48000 in one launch.  A DC offset of 0.5 on the longest clip makes every channel's
    mean large against its deviation: statistics taken as E[x^2] - E[x]^2 in f32 would lose the variance there.
    Bound: bf16 output rounding, half an ulp <= 2^-8 |y|, + 2e-4 absolute for the f32 conv (10 MACs), the normalisation (rstd up to ~30 on quiet channels) and erff."""
    sd = R.weights("a")
    fe = "wav2vec2.feature_extractor.conv_layers.0."
    w0, gw, gb = sd[fe + "conv.weight"], sd[fe + "layer_norm.weight"], sd[fe + "layer_norm.bias"]
    lens = [400, 401, 3217, 48000]
    clips = [clip(n, 10 + i) for i, n in enumerate(lens)]
    clips[3] = clips[3] + np.float32(0.5)
    Ls, Cd = max(lens), 128
    wav = torch.full((len(lens), Ls), 7.0)                                  # what lies behind a clip's end must never be read
    for i, c in enumerate(clips):
        wav[i, :len(c)] = torch.from_numpy(c)
    T0max = (Ls - 10) // 5 + 1
    rpb = T0max + 3                                                          # three guard rows behind the longest clip too
    sentinel = torch.tensor(-1234.0, dtype=BF16)
    out = torch.full((len(lens), rpb, Cd), -1234.0, dtype=BF16, device=DEV)
    got = ops.w2v_conv0_gn_gelu(wav.to(DEV), torch.tensor(lens, dtype=I32, device=DEV), torch.from_numpy(w0.reshape(Cd, 10)).to(DEV),
                                torch.from_numpy(gw).to(DEV), torch.from_numpy(gb).to(DEV), out=out, out_rpb=rpb)
    torch.cuda.synchronize()
    got = got.cpu()
    for i, c in enumerate(clips):
        T0 = (len(c) - 10) // 5 + 1
        want = REF.conv0_gn_gelu(c, w0, gw, gb)
        assert want.shape == (T0, Cd)
        err = (got[i, :T0].to(F64) - want).abs()
        bound = 2.0 ** -8 * want.abs() + 2e-4
        print(f"conv0 L={len(c)} T0={T0}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), f"clip {i} (L = {len(c)}): max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f}"
        assert (got[i, T0:] == sentinel).all(), f"clip {i}: rows behind its {T0} frames were written"


# ----------------------------------------------------------------------------- positional convolution
POS_T = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def _pos_inputs(H, seed, Ts=POS_T):
    g = torch.Generator().manual_seed(seed)
    cg = H // 16
    x = torch.randn(sum(Ts), H, generator=g)
    w = (torch.randn(H, cg, 128, generator=g) / (cg * 128) ** 0.5 * 2.0)
    b = torch.randn(H, generator=g) * 0.3
    cu = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=I32)
    return x, w, b, cu


def _pos_want(x_conv, x_res, w, b, Ts):
    """The definition per clip on the operands the kernel multiplies (bf16 x and w), residual from the stream's own x."""
    out, r = [], 0
    for T in Ts:
        xc = x_conv[r:r + T]
        out.append(x_res[r:r + T] + (REF.pos_conv_add(xc, w, b) - xc))
        r += T
    return torch.cat(out)


def _abs_products(xa, wa, Ts):
    """sum |x| |w| behind every output element (per clip): what the f32 accumulation error scales with."""
    out, r = [], 0
    for T in Ts:
        out.append(torch.nn.functional.conv1d(xa[r:r + T].T[None], wa, padding=64, groups=16)[0, :, :-1].T)
        r += T
    return torch.cat(out)


@pytest.mark.parametrize("H,stream", [(256, BF16), (768, BF16), (768, F32), (256, F32)])
def test_pos_conv_ragged_against_the_definition(H, stream):
    """16 and 48 channels per group; T = 1, 2 (inside the zero padding), 63, 64, 65 (the first frame with a full left window is 64),
    127, 128, 129 and 200 < 256 in one ragged launch -- and a 300-frame clip in a second one for the tile boundary at 256.
    Bound: the f32 accumulation of K = 128 cg exact bf16 products with sum |a b| = S (computed per element from the operands): the
    running sum is rounded once per 32-wide MFMA step (K / 32 of them) and at most 32 times inside a step, so (K / 32 + 32) 2^-24 S
    worst case; + the output rounding (bf16 stream: 2^-8 |y|, f32 stream: 2^-22 |y|) + 1e-5 for bias, erff and the add."""
    for Ts, seed in ((POS_T, 1), ((300, 5), 2)):
        x, w, b, cu = _pos_inputs(H, seed + H, Ts)
        xs = x.to(stream)
        wq = bf16_round(w)
        want = _pos_want(bf16_round(x), xs.to(F64), wq, b, Ts)
        S = _abs_products(bf16_round(x).abs(), wq.abs(), Ts)
        K = 128 * (H // 16)
        got = ops.w2v_pos_conv(xs.to(DEV), W.pack_pos_conv(w).to(DEV), b.to(DEV), cu.to(DEV), max(Ts))
        torch.cuda.synchronize()
        err = (got.cpu().to(F64) - want).abs()
        bound = (2.0 ** -8 if stream == BF16 else 2.0 ** -22) * want.abs() + S * (K / 32 + 32) * 2.0 ** -24 + 1e-5
        print(f"pos conv H={H} {stream} Ts={Ts}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), f"max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f} at {np.unravel_index(int((err / bound).argmax()), err.shape)}"


@pytest.mark.parametrize("cg", [8, 24, 40, 64])
def test_pos_conv_other_group_widths(cg):
    """The widths the two model geometries do not reach: 8 (half an MFMA column block), 24 and 40 (a partly filled last block, whose
    zero weight rows must not be stored into the next group's channels) and 64 (four blocks, the largest LDS window).  Same bound
    as above, f32 stream."""
    H, Ts = 16 * cg, (65, 130)
    x, w, b, cu = _pos_inputs(H, 100 + cg, Ts)
    wq = bf16_round(w)
    want = _pos_want(bf16_round(x), x.to(F64), wq, b, Ts)
    S = _abs_products(bf16_round(x).abs(), wq.abs(), Ts)
    got = ops.w2v_pos_conv(x.to(DEV), W.pack_pos_conv(w).to(DEV), b.to(DEV), cu.to(DEV), max(Ts))
    torch.cuda.synchronize()
    err = (got.cpu().to(F64) - want).abs()
    bound = 2.0 ** -22 * want.abs() + S * (128 * cg / 32 + 32) * 2.0 ** -24 + 1e-5
    print(f"pos conv cg={cg}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f}"


@pytest.mark.parametrize("H", [256, 768])
def test_pos_conv_unit_impulse_reproduces_the_taps(H):
    """x = one 1 at (frame t*, channel g cg + ci): out[t, g cg + co] - x = gelu(w[co, ci, t* - t + 64]) for t* - 63 <= t <= t* + 64
    and gelu(0) = 0 elsewhere, exactly the taps (bf16 values through an f32 stream: 1e-6).  An impulse on a clip's LAST frame would
    show in the frame T that the even kernel produces and the model drops: the next clip, all zeros, must stay all zeros; an impulse
    on a clip's FIRST frame must not reach the clip before it."""
    cg = H // 16
    g = torch.Generator().manual_seed(H)
    w = torch.randn(H, cg, 128, generator=g) * 0.5
    wq = bf16_round(w)
    Ts = (200, 130, 70, 90)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=I32)
    grp, ci = 5, cg - 3
    hits = ((0, 100), (1, 129), (3, 0))                                     # (clip, frame): interior, last frame, first frame
    x = torch.zeros(sum(Ts), H)
    for c, t in hits:
        x[int(cu[c]) + t, grp * cg + ci] = 1.0
    got = ops.w2v_pos_conv(x.to(DEV), W.pack_pos_conv(w).to(DEV), torch.zeros(H, device=DEV), cu.to(DEV), max(Ts))
    torch.cuda.synchronize()
    pe = got.cpu().to(F64) - x.to(F64)
    want = torch.zeros(sum(Ts), H, dtype=F64)
    for c, ts in hits:
        for t in range(Ts[c]):
            tap = ts - t + 64
            if 0 <= tap < 128:
                want[int(cu[c]) + t, grp * cg:(grp + 1) * cg] = REF.gelu(wq[grp * cg:(grp + 1) * cg, ci, tap])
    assert (pe - want).abs().max() <= 1e-6, (pe - want).abs().max()
    assert not pe[int(cu[2]):int(cu[3])].any(), "an impulse leaked into the all-zero clip between its neighbours"
    other = torch.ones(H, dtype=torch.bool)
    other[grp * cg:(grp + 1) * cg] = False
    assert not pe[:, other].any(), "an impulse leaked into another group"


# ----------------------------------------------------------------------------- head
@pytest.mark.parametrize("nc", [29, 32])
def test_head_log_softmax(nc):
    g = torch.Generator().manual_seed(nc)
    rows = 37
    logits = torch.randn(rows, 64, generator=g) * 6.0
    logits[:, nc:] = 100.0                                                  # the GEMM's padding columns: must never enter
    bias = torch.randn(nc, generator=g)
    out = torch.full((rows + 2, nc), 55.0, device=DEV)
    ops.w2v_head_logsoftmax(logits.to(DEV), bias.to(DEV), nc, out=out)
    torch.cuda.synchronize()
    got = out.cpu().to(F64)
    assert (got[rows:] == 55.0).all(), "rows behind the last one were written"
    p = got[:rows].exp().sum(-1)
    assert (p - 1.0).abs().max() <= 1e-5, (p - 1.0).abs().max()
    want = torch.log_softmax(logits[:, :nc].to(F64) + bias.to(F64), -1)
    assert (got[:rows] - want).abs().max() <= 1e-5, (got[:rows] - want).abs().max()


# ----------------------------------------------------------------------------- whole model
def _figures(got, want):
    """(relmax, 1 - cosine) of logits and max |d| of their log-probabilities, all in float64."""
    got, want = torch.as_tensor(got).to(F64), torch.as_tensor(want).to(F64)
    relmax = float((got - want).abs().max() / want.abs().max())
    cos = float((got * want).sum() / ((got * got).sum() * (want * want).sum()).sqrt())
    dlp = float((torch.log_softmax(got, -1) - torch.log_softmax(want, -1)).abs().max())
    return relmax, 1.0 - cos, dlp


def _yardstick(fx, i):
    bits = torch.from_numpy(fx[f"logits_bf16_{i}"].astype(np.int32) << 16).to(torch.int32).view(F32)
    return _figures(bits, fx[f"logits_f32_{i}"])


@pytest.fixture(scope="module")
def fixtures():
    return {g: np.load(os.path.join(GOLD, f"wav2vec2_{g}.npz")) for g in R.GEOMS}


@pytest.mark.parametrize("res_f32", [False, True])
@pytest.mark.parametrize("geom", ["a", "b"])
def test_whole_model_against_transformers(fixtures, geom, res_f32):
    """Both fixture clips in one ragged call.  Yardstick (transformers' bf16 module against its fp32 one, from the fixture):
    relmax 1.1e-2 .. 1.9e-2, 1 - cosine 7e-5 .. 9e-5, max |d log-prob| printed per clip.  Measured on MI355X: see profiles/wav2vec2.md."""
    fx = fixtures[geom]
    m = model(geom, res_f32)
    waves = R.waves()
    em, frames = m(waves)
    torch.cuda.synchronize()
    logits = m.logits_of_last_call().cpu()
    em = em.cpu()
    assert frames == [R.frames_of(len(w)) for w in waves] and em.shape == (sum(frames), R.N_CLASSES)
    assert (em.to(F64).exp().sum(-1) - 1).abs().max() <= 1e-5
    assert (torch.log_softmax(logits.to(F64), -1) - em.to(F64)).abs().max() <= 1e-5      # the emissions ARE the log-softmax of those logits
    r = 0
    for i, T in enumerate(frames):
        got, yard = _figures(logits[r:r + T], fx[f"logits_f32_{i}"]), _yardstick(fx, i)
        print(f"wav2vec2 {geom} res_f32={int(res_f32)} clip {i}: device relmax {got[0]:.3e} 1-cos {got[1]:.3e} dlogp {got[2]:.3e} | "
              f"bf16 module relmax {yard[0]:.3e} 1-cos {yard[1]:.3e} dlogp {yard[2]:.3e}")
        for name, a, b in zip(("relmax", "1 - cosine", "max |d log-prob|"), got, yard):
            assert a <= MARGIN * b, f"{geom} clip {i} {name}: device {a:.3e} > {MARGIN} x yardstick {b:.3e}"
        r += T


# ----------------------------------------------------------------------------- ragged batch
RAGGED = (8000, 24000, 43200)          # 0.5 s, 1.5 s, 2.7 s: 24, 74 and 134 frames


def test_ragged_batch_is_every_clip_alone(fixtures):
    """Three clips in one call against each clip through the definition, within the whole-model bound of this geometry (the larger of
    its fixture clips' yardsticks x 1.5).  Clip 1's samples do not reach the rows of clips 0 and 2 (bit-identical after overwriting
    them), what lies behind a clip's end in the padded tensor is never read, and rows behind sum T stay untouched."""
    geom, cfg = "a", R.GEOMS["a"]
    sd = R.weights(geom)
    m = model(geom)
    clips = [clip(n, 40 + i) for i, n in enumerate(RAGGED)]
    frames = [24, 74, 134]
    yard = [max(v) for v in zip(*(_yardstick(fixtures[geom], i) for i in range(len(R.CLIP_SAMPLES))))]
    wav = torch.full((3, max(RAGGED)), 3.0)
    for i, c in enumerate(clips):
        wav[i, :len(c)] = torch.from_numpy(c)
    rows = sum(frames)
    out = torch.full((rows + 3, 32), 55.0, device=DEV)
    em = m._forward_impl(wav.to(DEV), list(RAGGED), out=out)
    torch.cuda.synchronize()
    logits = m.logits_of_last_call().cpu()
    assert em.shape == (rows, 32) and (out[rows:] == 55.0).all(), "rows behind sum T were written"
    em_list, fr = m(clips)
    assert fr == frames and torch.equal(em_list, em), "a list of clips and the padded tensor with lengths disagree"
    r = 0
    for i, T in enumerate(frames):
        want = REF.forward(sd, clips[i], cfg["num_attention_heads"], cfg["num_hidden_layers"])
        got = _figures(logits[r:r + T], want)
        print(f"ragged clip {i} ({T} frames): relmax {got[0]:.3e} 1-cos {got[1]:.3e} dlogp {got[2]:.3e} | bound {MARGIN} x {yard}")
        for name, a, b in zip(("relmax", "1 - cosine", "max |d log-prob|"), got, yard):
            assert a <= MARGIN * b, f"clip {i} {name}: {a:.3e} > {MARGIN} x {b:.3e}"
        r += T
    before = em.clone()
    wav[1, :RAGGED[1]] = torch.from_numpy(clip(RAGGED[1], 99))
    after = m._forward_impl(wav.to(DEV), list(RAGGED))
    torch.cuda.synchronize()
    assert torch.equal(after[:24], before[:24]) and torch.equal(after[98:], before[98:]), "clip 1's samples reached another clip's rows"
    assert not torch.equal(after[24:98], before[24:98])


# ----------------------------------------------------------------------------- chain
TEXTS = ("hello world", "it's a test of alignment", "one two three four")


def test_chain_into_the_trellis_kernel():
    """ctc_align on the device's emissions == tests/align_ref.py on those same emissions, exactly; align(audio, acoustic_model=m) ==
    align(emission=m([audio])[0]); align_audio_batch == per-clip align."""
    m = model("a", n_classes=29, labels="torchaudio")
    clips = [clip(n, 60 + i) for i, n in enumerate(RAGGED)]
    em, frames = m(clips)
    torch.cuda.synchronize()
    assert em.shape == (sum(frames), 29)
    dictionary = ForcedAligner._dict()
    cu = np.concatenate([[0], np.cumsum(frames)])
    for n, text in enumerate(TEXTS):
        tokens = [dictionary[c] if c != " " else dictionary["|"] for c in text.upper()]
        e = em[cu[n]:cu[n + 1]]
        want = align_ref.align(e.cpu().numpy(), tokens, fast=True)
        tr = ForcedAligner._get_trellis(e, tokens)
        assert np.array_equal(tr.numpy(), np.asarray(want["trellis"], np.float32)), f"clip {n}: trellis differs from align_ref"
        spans = ForcedAligner._backtrack(tr, e, tokens)
        assert spans == align_ref.spans(tokens, want["status"], want["frames"], e.shape[0]), f"clip {n}: path differs from align_ref"
    per_clip = []
    for n, text in enumerate(TEXTS):
        a = ForcedAligner.align(clips[n], text, acoustic_model=m)
        b = ForcedAligner.align(None, text, emission=m([clips[n]])[0])
        assert a == b and len(a) == len(text.split()), (a, b)
        per_clip.append(a)
    assert ForcedAligner.align_audio_batch(clips, list(TEXTS), m) == per_clip

"""-m gpu: the layer-norm / stable wav2vec2 family on the device (csrc/wav2vec2.hip, csrc/norm.hip, tiny_audio_amd/wav2vec2.py) against
its float64 definition (tests/wav2vec2_sln_ref.py) and against transformers' own outputs (tests/golden/wav2vec2_sln_{c,d}.npz), and the
aligner on a vocabulary of its own.

Bounds.  The new kernels are measured against the definition evaluated on the very operands the kernel reads, so what is left is the
bf16 output rounding (8 significant bits: half an ulp is up to 2^-8 of the value) plus f32 arithmetic, whose size each test derives
from the reference's own quantities.  The whole model is measured against the fp32 fixture with transformers' bf16 module ON THE SAME
INPUT as the yardstick (read from the fixture, never from the code under test) and the margin of tests/test_gpu_wav2vec2.py: 1.5 x
the yardstick's relmax, 1.5 x its (1 - cosine) and 1.5 x its max |d log-prob|.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import align_ref
from tests import wav2vec2_sln_ref as REF
from tests.golden import wav2vec2_recipe as RB
from tests.golden import wav2vec2_sln_recipe as R
from tiny_audio_amd import _lib, alignment, ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import ForcedAligner
from tiny_audio_amd.ops import ptr, stream

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
MARGIN = 1.5
U = 2.0 ** -24                                   # unit roundoff of f32
GELU_LIP = 1.13                                  # max |gelu'|


def bf16_round(a):
    return torch.as_tensor(np.asarray(a)).to(F32).to(BF16).to(F64)


def config(geom, n_classes=32, normalize_input="hf", **kw):
    return W.Wav2Vec2CtcConfig(**{**R.GEOMS[geom], **kw}, n_classes=n_classes, normalize_input=normalize_input, **R.FAMILY)


def model(geom, res_f32=False, normalize_input="hf", sd=None, **kw):
    m = W.Wav2Vec2CtcMI355X(config(geom, normalize_input=normalize_input, **kw), device=DEV)
    m.load_state_dict_hf(sd if sd is not None else WEIGHTS(geom))
    m.res_f32 = res_f32
    return m


_W = {}


def WEIGHTS(geom):
    """The recipe's weights, drawn once per geometry and never changed."""
    if geom not in _W:
        _W[geom] = R.weights(geom)
    return _W[geom]


def clip(n, seed):
    """A deterministic 16 kHz clip of n samples: two tones, noise and a small DC offset."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.15 * np.sin(2 * np.pi * 220.0 * t + seed) + 0.07 * np.sin(2 * np.pi * 1900.0 * t) + 0.03 * g.standard_normal(n) + 0.02).astype(np.float32)


# ----------------------------------------------------------------------------- conv 0 + LayerNorm + GELU
def _conv0_bound(c, w0, b0, gw, want):
    """|device - definition| <= 2^-8 |y| (the bf16 store) + the f32 arithmetic, derived from the reference's own quantities.
    Per frame t and channel c, v = b + sum_j w_j x_j is 10 FMAs onto the bias: 11 roundings of partial sums bounded by
    S_tc = |b_c| + sum_j |w_cj| |x_tj|, so |dv| <= 11 u S_tc <= E_t := 12 u max_c S_tc.  The mean over the channels carries at most E_t
    again plus its own summation (log2(C) + C / 64 <= 17 roundings of values <= S: inside 2 E_t in all), so the deviation d = v - m is
    off by at most 3 E_t.  rstd is relatively off by (3 E_t) rstd from the deviations (d(var) / var ~ 2 dd / sigma, halved by the
    square root) plus 2^-20 for rsqrtf and the mean of squares.  z = d rstd g + beta therefore moves by
    |g_c| rstd_t 3 E_t (1 + |d rstd|) + 2^-20 (|z| + |beta|), GELU stretches that by at most 1.13, and erff adds 2^-20 absolute."""
    x = REF._t(c)
    T0 = (len(c) - 10) // 5 + 1
    win = torch.stack([x[j: j + (T0 - 1) * 5 + 1: 5] for j in range(10)], 1).abs()                    # [T0, 10]
    S = win @ REF._t(w0).reshape(-1, 10).abs().T + REF._t(b0).abs()                                     # [T0, C]
    E = 12 * U * S.max(1, keepdim=True).values
    v = REF.conv_valid(x.reshape(-1, 1), w0, 5) + REF._t(b0)
    m = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - m) ** 2).mean(1, keepdim=True) + REF.CONV_LN_EPS)
    h = (v - m) * rstd
    z = h * REF._t(gw)
    return 2.0 ** -8 * want.abs() + GELU_LIP * (REF._t(gw).abs() * rstd * 3 * E * (1 + h.abs()) + 2.0 ** -20 * (z.abs() + 1.0)) + 2.0 ** -20


@pytest.mark.parametrize("geom", ["c", "d"])
def test_conv0_layernorm_gelu_each_clip_alone(geom):
    """C = 128 and 512 (2 and 8 channels per lane).  Clips of 400 samples (79 conv-0 frames, one final frame), 8123 and 45011 samples
    (the fixture clips: 7 and 36 chunks of 256 frames, both with a ragged last chunk), one clip riding on a DC offset of 0.5 and a
    silent one, in one launch.  Output and what lies behind a clip's end are pre-filled with NaN: rows t >= T0_b still hold it, and
    overwriting the middle clip leaves its neighbours' rows bit-identical."""
    sd, Cd = WEIGHTS(geom), R.GEOMS[geom]["conv_dim"]
    fe = "wav2vec2.feature_extractor.conv_layers.0."
    w0, b0, gw, gb = sd[fe + "conv.weight"], sd[fe + "conv.bias"], sd[fe + "layer_norm.weight"], sd[fe + "layer_norm.bias"]
    fix = R.waves()
    clips = [clip(400, 1), fix[0], clip(3217, 2) + np.float32(0.5), np.zeros(2000, np.float32), fix[1]]
    lens = [len(c) for c in clips]
    Ls = max(lens)
    wav = torch.full((len(lens), Ls), float("nan"))                         # what lies behind a clip's end must never be read
    for i, c in enumerate(clips):
        wav[i, :len(c)] = torch.from_numpy(c)
    rpb = (Ls - 10) // 5 + 1 + 3                                             # three guard rows behind the longest clip too
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (dev(w0.reshape(Cd, 10)), dev(b0), dev(gw), dev(gb))
    lens_d = torch.tensor(lens, dtype=I32, device=DEV)
    out = torch.full((len(lens), rpb, Cd), float("nan"), dtype=BF16, device=DEV)
    got = ops.w2v_conv0_ln_gelu(wav.to(DEV), lens_d, *args, out=out, out_rpb=rpb)
    torch.cuda.synchronize()
    got = got.cpu()
    for i, c in enumerate(clips):
        T0 = (len(c) - 10) // 5 + 1
        want = REF.conv0_ln_gelu(c, w0, b0, gw, gb)
        assert want.shape == (T0, Cd)
        err = (got[i, :T0].to(F64) - want).abs()
        bound = _conv0_bound(c, w0, b0, gw, want)
        print(f"conv0+LN C={Cd} L={len(c)} T0={T0}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}, abs term up to {float((bound - 2.0 ** -8 * want.abs()).max()):.2e}")
        assert torch.isfinite(got[i, :T0]).all() and (err <= bound).all(), f"clip {i} (L = {len(c)}): max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f}"
        assert torch.isnan(got[i, T0:]).all(), f"clip {i}: rows behind its {T0} frames were written"
    wav2 = wav.clone()
    wav2[2, :lens[2]] = torch.from_numpy(clip(lens[2], 77))
    out2 = torch.full_like(out, float("nan"))
    got2 = ops.w2v_conv0_ln_gelu(wav2.to(DEV), lens_d, *args, out=out2, out_rpb=rpb).cpu()
    as_bits = lambda t: t.view(torch.int16)
    for i in (0, 1, 3, 4):
        assert torch.equal(as_bits(got2[i]), as_bits(got[i])), f"clip 2's samples reached clip {i}"
    assert not torch.equal(as_bits(got2[2]), as_bits(got[2]))


# ----------------------------------------------------------------------------- LayerNorm + GELU, row-wise
def _ln_gelu_case(M, H, seed, equal_row=None):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, H, generator=g) * (0.5 + torch.rand(M, 1, generator=g) * 3) + torch.randn(M, 1, generator=g)).to(BF16)
    if equal_row is not None:
        x[equal_row] = 3.0
    w, b = 1 + 0.2 * torch.randn(H, generator=g), 0.3 * torch.randn(H, generator=g)
    out = torch.full((M + 2, H), float("nan"), dtype=BF16, device=DEV)
    ops.layernorm_gelu(x.to(DEV), w.to(DEV), b.to(DEV), out=out[:M])
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[M:]).all(), "rows behind the last one were written"
    xd = x.to(F64)
    m = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - m) ** 2).mean(1, keepdim=True) + 1e-5)
    h = (xd - m) * rstd
    z = h * w.to(F64) + b.to(F64)
    want = REF.gelu(z)
    # The operands are exact (bf16), so what is left is f32 arithmetic.  The row sum is H additions of values <= X = max |x| of the row:
    # the mean is off by at most (log2(64) + H / 64 + 1) u X <= E := 16 u X at H <= 512, and so is every deviation (plus its own
    # rounding: 2 E).  As for conv 0: rstd relatively off by 2 E rstd + 2^-20, z by |g| rstd 2 E (1 + |h|) + 2^-20 (|z| + 1),
    # x 1.13 through GELU, + 2^-20 for erff, + the bf16 store.
    E = 16 * U * xd.abs().max(1, keepdim=True).values
    bound = 2.0 ** -8 * want.abs() + GELU_LIP * (w.to(F64).abs() * rstd * 2 * E * (1 + h.abs()) + 2.0 ** -20 * (z.abs() + 1.0)) + 2.0 ** -20
    err = (got[:M].to(F64) - want).abs()
    print(f"LN+GELU M={M} H={H}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f}"
    return got[:M], want


@pytest.mark.parametrize("M", [1, 63, 1000, 4100, 8200])
def test_layernorm_gelu_rows(M):
    """C = 512 (the half-wave kernel): 1 row, 63 (a partly filled last workgroup of 8) and 1000, plus 4100 and 8200 rows, where the
    kernel walks 2 and 4 rows per half wave (at 8200 the last half wave has only 2 of its 4).  Row 0 of the 63-row case holds 512
    equal values: variance 0, every output gelu(beta)."""
    got, _ = _ln_gelu_case(M, 512, 100 + M, equal_row=0 if M == 63 else None)
    assert torch.isfinite(got).all()


def test_layernorm_gelu_other_width_and_nan_rows_stay_in_their_row():
    """C = 128 takes the wave-per-row kernel (geometry c's conv layers).  A row of NaN -- what a slab row behind a clip's length may
    hold -- gives a row of NaN and leaves its neighbours' bits alone."""
    _ln_gelu_case(63, 128, 7, equal_row=5)
    for H in (128, 512):
        g = torch.Generator().manual_seed(H)
        x = torch.randn(40, H, generator=g).to(BF16)
        w, b = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
        clean = ops.layernorm_gelu(x.to(DEV), w, b).cpu()
        x2 = x.clone()
        x2[17] = float("nan")
        x2[18, 3] = float("inf")
        dirty = ops.layernorm_gelu(x2.to(DEV), w, b).cpu()
        keep = [i for i in range(40) if i not in (17, 18)]
        assert torch.equal(clean[keep].view(torch.int16), dirty[keep].view(torch.int16)) and torch.isnan(dirty[17]).all()


# ----------------------------------------------------------------------------- input normalisation
@pytest.mark.parametrize("eps", [1e-7, 1e-5])
def test_input_normalisation(eps):
    """Lengths 400 (one partly filled chunk) and 480 000 (118 chunks of 4096, the last ragged: two per lane of the merge), a clip of
    deviation 0.01 riding on a DC offset of 0.5 (E[x^2] - E[x]^2 in f32 would lose its variance), and a silent clip, in one launch;
    the samples behind a clip's end hold NaN before and after.
    Bound, from the reference's quantities: a chunk mean is a sum of up to 4096 values in 16 + 8 additions per lane and tree level,
    off by at most 24 u X (X = max |x|), so is the merged mean (the merge is in f64) and one more u X for its cast to f32; the
    deviation adds its own rounding u |d|.  The variance is a sum of squares of those deviations: relatively off by 2 (25 u X) / sigma
    (second order otherwise) + 24 u, i.e. rstd by half of that, + 2^-22 for the division and the product."""
    g = np.random.default_rng(5)
    clips = [clip(400, 3), clip(480000, 4), (0.5 + 0.01 * g.standard_normal(100000)).astype(np.float32), np.zeros(5000, np.float32)]
    lens = [len(c) for c in clips]
    wav = torch.full((len(clips), max(lens)), float("nan"))
    for i, c in enumerate(clips):
        wav[i, :len(c)] = torch.from_numpy(c)
    got = ops.w2v_input_norm(wav.to(DEV), torch.tensor(lens, dtype=I32, device=DEV), eps, out=torch.full_like(wav, float("nan"), device=DEV))
    torch.cuda.synchronize()
    got = got.cpu()
    for i, c in enumerate(clips):
        want = REF.normalize_input(c, eps)
        x = REF._t(c)
        d = x - x.mean()
        var = (d * d).mean()
        rstd = 1.0 / torch.sqrt(var + eps)
        X = x.abs().max()
        bound = rstd * (25 * U * X + U * d.abs()) + want.abs() * (25 * U * X * torch.sqrt(var) / (var + eps) + 12 * U + 2.0 ** -22)
        err = (got[i, :len(c)].to(F64) - want).abs()
        print(f"input norm eps={eps} L={len(c)}: max |d| {err.max():.3e}, worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, rstd {float(rstd):.3e}")
        assert torch.isfinite(got[i, :len(c)]).all() and (err <= bound).all(), f"clip {i}: max |d| {err.max():.3e}"
        assert torch.isnan(got[i, len(c):]).all(), f"clip {i}: samples behind its end were written"
    assert not got[3, :5000].any(), "a silent clip is all zeros"


# ----------------------------------------------------------------------------- whole model
def _figures(got, want):
    """(relmax, 1 - cosine) of logits and max |d| of their log-probabilities, all in float64."""
    got, want = torch.as_tensor(got).to(F64), torch.as_tensor(want).to(F64)
    relmax = float((got - want).abs().max() / want.abs().max())
    cos = float((got * want).sum() / ((got * got).sum() * (want * want).sum()).sqrt())
    dlp = float((torch.log_softmax(got, -1) - torch.log_softmax(want, -1)).abs().max())
    return relmax, 1.0 - cos, dlp


def _yardstick(fx, tag):
    bits = torch.from_numpy(fx[f"logits_bf16_{tag}"].astype(np.int32) << 16).to(torch.int32).view(F32)
    return _figures(bits, fx[f"logits_f32_{tag}"])


@pytest.fixture(scope="module")
def fixtures():
    return {g: np.load(os.path.join(GOLD, f"wav2vec2_sln_{g}.npz")) for g in R.GEOMS}


def _assert_within(name, got, yard):
    for what, a, b in zip(("relmax", "1 - cosine", "max |d log-prob|"), got, yard):
        assert a <= MARGIN * b, f"{name} {what}: device {a:.3e} > {MARGIN} x yardstick {b:.3e}"


@pytest.mark.parametrize("res_f32", [False, True])
@pytest.mark.parametrize("geom", ["c", "d"])
def test_whole_model_against_transformers(fixtures, geom, res_f32):
    """Both fixture clips in one ragged call, the device normalising the raw clips itself (normalize_input="hf").  Yardstick
    (transformers' bf16 module against its fp32 one, from the fixture): relmax 1.1e-2 .. 1.8e-2, 1 - cosine 1.0e-4 .. 1.2e-4."""
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
        print(f"wav2vec2-sln {geom} res_f32={int(res_f32)} clip {i}: device relmax {got[0]:.3e} 1-cos {got[1]:.3e} dlogp {got[2]:.3e} | "
              f"bf16 module relmax {yard[0]:.3e} 1-cos {yard[1]:.3e} dlogp {yard[2]:.3e}")
        _assert_within(f"{geom} clip {i}", got, yard)
        r += T


def test_one_clip_without_normalisation(fixtures):
    """normalize_input=None: the raw waveform goes in, against the fixture's logits of the raw clip and their own yardstick."""
    for geom in ("c", "d"):
        m = model(geom, normalize_input=None)
        m([R.waves()[R.RAW_CLIP]])
        torch.cuda.synchronize()
        got, yard = _figures(m.logits_of_last_call().cpu(), fixtures[geom]["logits_f32_raw"]), _yardstick(fixtures[geom], "raw")
        print(f"wav2vec2-sln {geom} raw clip: device relmax {got[0]:.3e} 1-cos {got[1]:.3e} dlogp {got[2]:.3e} | bf16 module {yard}")
        _assert_within(f"{geom} raw clip", got, yard)


# ----------------------------------------------------------------------------- intermediate states of geometry c
# A bf16 rounding is relatively off by at most half an ulp, uniformly: rms at most 2^-7 / sqrt(12) of the value.  Every stage that
# rounds to bf16 (a weight matrix, a GEMM operand, a stored activation) adds one such independent relative error to the state; LayerNorm
# passes a relative error on and GELU stretches it by at most 1.13.  With N roundings behind a state its relative L2 error is therefore
# at most 1.13 sqrt(N) 2^-7 / sqrt(12), and no element should be off by more than 6 such standard deviations of the state's rms.
#   feat   7 conv layers x (weights, input operand, stored output)                                              N = 21
#   pos    + feature projection (operand, weights, stored stream) + positional conv (operand, weights, stored)   N = 27
#   layer0 + q|k|v (operand, weights, stored), probabilities, attention output, out_proj weights, stream,
#            ffn operand, W1, stored gelu, W2, stream                                                            N = 39
STATE_ROUNDINGS = {"feat": 21, "pos": 27, "layer0": 39}


def _state_bound(n):
    return GELU_LIP * math.sqrt(n) * 2.0 ** -7 / math.sqrt(12.0)


@pytest.mark.parametrize("res_f32", [False, True])
def test_intermediate_states_of_geometry_c(fixtures, res_f32):
    """feat from the full model; pos from the same weights with no layer, layer0 with one: the residual stream behind the last layer
    is what ``state_of_last_call`` reads, and hidden_states[0] / [1] of this family are that raw stream."""
    fx, waves = fixtures["c"], R.waves()
    frames = [R.frames_of(len(w)) for w in waves]
    got = {}
    for name, layers in (("pos", 0), ("layer0", 1)):
        m = model("c", res_f32, num_hidden_layers=layers)
        m(waves)
        torch.cuda.synchronize()
        got[name] = m.state_of_last_call("stream").to(F64).cpu()
        if layers == 1:
            got["feat"] = m.state_of_last_call("feat").to(F64).cpu()
    r = 0
    for i, T in enumerate(frames):
        for name in ("feat", "pos", "layer0"):
            want = torch.from_numpy(fx[f"{name}_{i}"]).to(F64)
            d = got[name][r:r + T] - want
            rel, worst = float(d.norm() / want.norm()), float(d.abs().max() / want.pow(2).mean().sqrt())
            bound = _state_bound(STATE_ROUNDINGS[name])
            print(f"state {name} clip {i} res_f32={int(res_f32)}: rel L2 {rel:.3e} (bound {bound:.3e}), max |d| / rms {worst:.3e} (bound {6 * bound:.3e})")
            assert rel <= bound and worst <= 6 * bound, f"{name} clip {i}: rel L2 {rel:.3e} > {bound:.3e} or max |d| / rms {worst:.3e} > {6 * bound:.3e}"
        r += T


# ----------------------------------------------------------------------------- ragged batch
RAGGED = (8000, 24000, 43200)          # 0.5 s, 1.5 s, 2.7 s: 24, 74 and 134 frames


def test_ragged_batch_is_every_clip_alone(fixtures):
    """Three clips in one call against each clip through the definition (normalised over its OWN samples), within the whole-model
    bound of this geometry (the larger of its fixture clips' yardsticks x 1.5).  What lies behind a clip's end in the padded tensor is
    never read (NaN there), rows behind sum T stay untouched, and the third clip's samples do not reach the rows of the first two."""
    geom, cfg = "c", R.GEOMS["c"]
    sd = WEIGHTS(geom)
    m = model(geom)
    clips = [clip(n, 40 + i) for i, n in enumerate(RAGGED)]
    frames = [24, 74, 134]
    yard = [max(v) for v in zip(*(_yardstick(fixtures[geom], i) for i in range(len(R.CLIP_SAMPLES))))]
    wav = torch.full((3, max(RAGGED)), float("nan"))
    for i, c in enumerate(clips):
        wav[i, :len(c)] = torch.from_numpy(c)
    rows = sum(frames)
    out = torch.full((rows + 3, 32), 55.0, device=DEV)
    em = m._forward_impl(wav.to(DEV), list(RAGGED), out=out)
    torch.cuda.synchronize()
    logits = m.logits_of_last_call().cpu()
    assert em.shape == (rows, 32) and (out[rows:] == 55.0).all(), "rows behind sum T were written"
    assert torch.isfinite(em).all()
    em_list, fr = m(clips)
    assert fr == frames and torch.equal(em_list, em), "a list of clips and the padded tensor with lengths disagree"
    r = 0
    for i, T in enumerate(frames):
        want = REF.forward(sd, clips[i], cfg["num_attention_heads"], cfg["num_hidden_layers"], normalize="hf")
        got = _figures(logits[r:r + T], want)
        print(f"ragged clip {i} ({T} frames): relmax {got[0]:.3e} 1-cos {got[1]:.3e} dlogp {got[2]:.3e} | bound {MARGIN} x {yard}")
        _assert_within(f"ragged clip {i}", got, yard)
        r += T
    before = em.clone()
    wav[2, :RAGGED[2]] = torch.from_numpy(clip(RAGGED[2], 99))
    after = m._forward_impl(wav.to(DEV), list(RAGGED))
    torch.cuda.synchronize()
    assert torch.equal(after[:98], before[:98]), "the third clip's samples reached another clip's rows"
    assert not torch.equal(after[98:], before[98:])


# ----------------------------------------------------------------------------- long form
def test_emissions_long():
    """A recording shorter than one window: the bytes of ``forward``.  One recording across three windows (140 frames in windows
    of 50): finite, the right frame count, the whole recording's statistics applied once -- so the windowed emissions equal those
    of the same windows cut from the pre-normalised recording, byte for byte."""
    m = model("c")
    w = R.waves()[1]
    whole = m([w])[0].clone()
    assert torch.equal(m.emissions_long(w, window_s=30.0), whole)
    table = W.long_windows(len(w), 16000, 3200)
    assert len(table) == 3
    em = m.emissions_long(w, window_s=1.0, context_s=0.2)
    torch.cuda.synchronize()
    assert em.shape == (140, 32) and torch.isfinite(em).all() and (em.to(F64).exp().sum(-1) - 1).abs().max() <= 1e-5
    wn = ops.w2v_input_norm(torch.from_numpy(w).to(DEV)[None], torch.tensor([len(w)], dtype=I32, device=DEV), 1e-7)[0]
    parts, _ = m([wn[s0:s1] for s0, s1, _, _ in table], normalized=True)
    row = 0
    for s0, s1, f0, f1 in table:
        lo = row + f0 - s0 // 320
        assert torch.equal(em[f0:f1], parts[lo:lo + f1 - f0])
        row += W.frames_of(s1 - s0)


# ----------------------------------------------------------------------------- chain into the trellis
VOCAB = {t: i for i, t in enumerate(["<s>", "</s>", "<unk>", "<pad>", " "] + list("abcdefghijklmnopqrstuvwxyz") + list("äöüß'") + ["é", "ñ", "ç", "-"])}
TEXTS = ("Grüße dich", "it's a Test of alignment", "one two three four")


def _vocab_model():
    sd = dict(WEIGHTS("c"))
    g = np.random.default_rng(40)
    sd["lm_head.weight"] = (g.standard_normal((40, 256)) / 16.0 * R.HEAD_GAIN).astype(np.float32)
    sd["lm_head.bias"] = (0.5 * g.standard_normal(40)).astype(np.float32)
    m = W.Wav2Vec2CtcMI355X(config("c", n_classes=40), device=DEV).load_state_dict_hf(sd)
    return m.set_vocab(VOCAB, blank_token="<pad>", word_delimiter=" ")


def _words_from_ref(text, e, tokens, dictionary, blank_id):
    want = align_ref.align(e, tokens, blank_id=blank_id, fast=True)
    spans = align_ref.spans(tokens, want["status"], want["frames"], e.shape[0])
    return alignment._group_words(text, spans, dictionary, 320 / 16000, ForcedAligner.START_OFFSET, ForcedAligner.END_OFFSET)


def test_chain_into_the_trellis_with_the_models_own_vocabulary():
    """40 classes, blank id 3, lower-case letters, ' ' as the word delimiter: align_audio_batch and align_long give exactly the words of
    the numpy trellis (tests/align_ref.py) run on the device's own emissions copied to the host."""
    m = _vocab_model()
    assert m.blank_id == 3
    clips = [clip(n, 60 + i) for i, n in enumerate(RAGGED)]
    em, frames = m(clips)
    torch.cuda.synchronize()
    assert em.shape == (sum(frames), 40)
    cu = np.concatenate([[0], np.cumsum(frames)])
    tokens = [alignment._tokenize(t, m.dictionary, True) for t in TEXTS]
    assert tokens[0] == [VOCAB[c] for c in "grüße"] + [4] + [VOCAB[c] for c in "dich"]
    want = [_words_from_ref(TEXTS[n], em[cu[n]:cu[n + 1]].cpu().numpy(), tokens[n], m.dictionary, 3) for n in range(3)]
    got = ForcedAligner.align_audio_batch(clips, list(TEXTS), m)
    assert got == want and [len(w) for w in got] == [2, 5, 4]
    assert ForcedAligner.align(clips[0], TEXTS[0], acoustic_model=m) == want[0]
    # blank 0 -- what the aligner used before -- is a different alignment here: the model's blank id is what went in
    other = _words_from_ref(TEXTS[1], em[cu[1]:cu[2]].cpu().numpy(), tokens[1], m.dictionary, 0)
    assert other != want[1]
    # the long form on the longest clip, one window and three
    for window_s in (30.0, 1.0):
        e = m.emissions_long(clips[2], window_s=window_s, context_s=0.2)
        got_long = ForcedAligner.align_long(clips[2], TEXTS[2], acoustic_model=m, window_s=window_s, context_s=0.2)
        assert got_long == _words_from_ref(TEXTS[2], e.cpu().numpy(), tokens[2], m.dictionary, 3)


def test_operator_passes_opcheck():
    from tiny_audio_amd import torch_ops
    m = model("c")
    h = torch_ops.register_module(m)
    wav = torch.zeros((2, 9000), device=DEV)
    wav[0], wav[1, :500] = torch.from_numpy(clip(9000, 1)).to(DEV), torch.from_numpy(clip(500, 2)).to(DEV)
    for normalized in (False, True):
        torch.library.opcheck(torch.ops.ta355.wav2vec2_sln_emissions, (wav, [9000, 500], normalized, h), test_utils=("test_schema", "test_faketensor"))


# ----------------------------------------------------------------------------- regression guard
def test_base_model_through_the_new_plumbing_is_bit_identical():
    """The base model built from the new config's defaults, through ``forward`` (the operator, ``_forward_impl``'s new dispatch),
    against the old entry point ``ta_wav2vec2_forward`` called directly on the same weights in this run: the same bytes, both
    stream modes."""
    waves = RB.waves()
    for res_f32 in (False, True):
        m = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**RB.GEOMS["a"], n_classes=32), device=DEV).load_state_dict_hf(RB.weights("a"))
        m.res_f32 = res_f32
        assert isinstance(m._w, _lib.Wav2Vec2Weights) and not m.config.sln
        em, frames = m(waves)
        lens = np.asarray([len(w) for w in waves], np.int32)
        Ls, B = int(lens.max()), len(waves)
        wav = torch.zeros((B, Ls), device=DEV)
        for i, w in enumerate(waves):
            wav[i, :len(w)] = torch.from_numpy(w).to(DEV)
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum(frames)
        L = _lib.lib()
        n = L.ta_wav2vec2_workspace_bytes(C.byref(m._w), B, Ls, int(cu[-1]))
        ws = torch.empty(n, device=DEV, dtype=torch.uint8)
        out = torch.empty((int(cu[-1]), 32), device=DEV)
        lens_d, cu_d = torch.from_numpy(lens).to(DEV), torch.from_numpy(cu).to(DEV)
        _lib.check(L.ta_wav2vec2_forward(C.byref(m._w), ptr(wav), lens.ctypes.data_as(C.c_void_p), ptr(lens_d), ptr(cu_d), B, Ls, ptr(out),
                                         ptr(ws), n, stream()), "ta_wav2vec2_forward")
        torch.cuda.synchronize()
        assert torch.equal(em, out), f"res_f32={res_f32}"

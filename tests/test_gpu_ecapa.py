"""-m gpu: the ECAPA-TDNN speaker-embedding model on the device (csrc/ecapa.hip, tiny_audio_amd/ecapa.py) against the float64 definition
(tests/ecapa_ref.py) and against torch's own outputs (tests/golden/ecapa_{a,full}.npz).

Bounds.  The new kernels are measured against the definition evaluated on the very operands the kernel reads, so what is left is the
output rounding (bf16 keeps 8 significant bits: half an ulp is up to 2^-8 of the value) plus f32 arithmetic; each test states its own.
The features get 4x the error of torch.stft-based f32 features against float64 on the same input (read from the fixture): a different
FFT factorisation and summation order, both f32.  The whole model is measured against the fp32 fixture with the same torch modules
cast to bfloat16 ON THE SAME FEATURES as the yardstick (read from the fixture, never from the code under test) and gets 1.5x its
relmax and 1.5x its (1 - cosine), the margin and yardstick of tests/test_gpu_wav2vec2.py.

Figures measured on MI355X: profiles/diarization.md.
"""
import os

import numpy as np
import pytest
import torch

from tests import ecapa_ref as REF
from tests.golden import ecapa_recipe as R
from tiny_audio_amd import ecapa as E
from tiny_audio_amd import ops

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
MARGIN = 1.5
FEATURE_MARGIN = 4.0
SENTINEL = -1234.0


def fixture(geom):
    return np.load(os.path.join(GOLD, f"ecapa_{geom}.npz"))


def tables():
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in E.fbank_tables())


def model(geom):
    return E.EcapaTdnnMI355X(E.EcapaConfig(**R.GEOMS[geom]), device=DEV).load_state_dict_speechbrain(R.weights(geom))


def fma32(x, s, t):
    """fmaf(x, s, t) of f32 operands as the device computes it: the product and sum are exact in float64 here (x has 8 significant bits)."""
    return (x.to(F64) * s.to(F64) + t.to(F64)).to(F32)


# ----------------------------------------------------------------------------- 1. features
def test_features_against_the_definition():
    """Windows of 12000 (T = 76), 3333 (T = 21), 640 (T = 5) samples and a 7000-sample chunk reflected to 12000, each over a 1e-3 noise
    floor, one on a DC offset; the audio buffer holds 9.0 between the chunks (never read).  Bound: 4x the torch.stft f32 yardstick of
    the fixture, per input.  The slab carries the same values rounded to bf16, its halo rows equal the reflected rows bit for bit and
    its channels 80 .. 127 are zero.  An all-zero window gives exactly 0 everywhere (-100 dB minus its own mean)."""
    yard = fixture("a")["feat_yardstick_db"]
    tabs = tables()
    inputs = R.feature_windows()
    gap = 37
    audio = np.full(sum(len(c) + gap for c, _ in inputs) + 12000, 9.0, np.float32)
    starts, pos = [], 0
    for c, _ in inputs:
        audio[pos:pos + len(c)] = c
        starts.append(pos)
        pos += len(c) + gap
    zero_start = pos
    audio[zero_start:zero_start + 12000] = 0.0
    a_dev = torch.from_numpy(audio).to(DEV)
    for L in sorted({L for _, L in inputs}):
        idx = [i for i, (_, Li) in enumerate(inputs) if Li == L]
        st = [starts[i] for i in idx] + ([zero_start] if L == 12000 else [])
        ln = [len(inputs[i][0]) for i in idx] + ([12000] if L == 12000 else [])
        feat, slab = ops.ecapa_fbank(a_dev, torch.tensor(st, dtype=I32, device=DEV), torch.tensor(ln, dtype=I32, device=DEV), L, tabs)
        torch.cuda.synchronize()
        feat, slab = feat.cpu(), slab.cpu()
        T = REF.frames_of(L)
        assert feat.shape == (len(st), T, 80) and slab.shape == (len(st), T + 4, 128)
        for j, i in enumerate(idx):
            want = REF.fbank(REF.reflect_extend(inputs[i][0], L).astype(np.float32))
            err = float(np.abs(feat[j].to(F64).numpy() - want).max())
            print(f"features input {i} (chunk {len(inputs[i][0])} -> {L}, T = {T}): max |d| {err:.3e} dB, yardstick {yard[i]:.3e}, "
                  f"ratio {err / yard[i]:.2f}")
            assert err <= FEATURE_MARGIN * yard[i], f"input {i}: {err:.3e} dB against {FEATURE_MARGIN} x {yard[i]:.3e}"
        if L == 12000:
            assert (feat[-1] == 0).all() and (slab[-1].to(F32) == 0).all(), "an all-zero window must give exactly 0"
        bits = slab.view(torch.int16)
        assert (bits[:, 2:T + 2, :80] == feat.to(BF16).view(torch.int16)).all()
        assert (bits[:, :, 80:] == 0).all()
        assert (bits[:, 0] == bits[:, 4]).all() and (bits[:, 1] == bits[:, 3]).all()
        assert (bits[:, T + 2] == bits[:, T]).all() and (bits[:, T + 3] == bits[:, T - 1]).all()


# ----------------------------------------------------------------------------- 2. Res2Net chain
def _res2net_case(w, d, T, seed, N=3, guard=3):
    g = torch.Generator().manual_seed(seed)
    Cw = 8 * w
    z1 = torch.full((N, T + guard, Cw), 5.0)
    z1[:, :T] = torch.randn(N, T, Cw, generator=g)
    bn1_s, bn1_t = 0.8 + 0.4 * torch.rand(Cw, generator=g), 0.2 * torch.randn(Cw, generator=g)
    ws = [torch.randn(w, w, 3, generator=g) * (2.0 / (3 * w)) ** 0.5 for _ in range(7)]
    rb, rs, rt = 0.1 * torch.randn(7 * w, generator=g), 0.8 + 0.4 * torch.rand(7 * w, generator=g), 0.2 * torch.randn(7 * w, generator=g)
    return z1.to(BF16), bn1_s, bn1_t, ws, rb, rs, rt


@pytest.mark.parametrize("T", [5, 21, 76])
@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("w", [16, 48, 128])
def test_res2net_against_the_definition(w, d, T):
    """Three windows per launch, three guard rows behind every window's slab in z1 (5.0: never read) and in y (a sentinel that must
    survive).  The gate is per sub-band: the float64 definition of sub-band i takes the DEVICE's own bf16 y_{i-1}, and its operand
    a = bf16(fmaf(relu(z1_i), s1, t1) + y_{i-1}) is rebuilt here in the device's f32 arithmetic, so what is left is
      2^-8 |y|                     half a bf16 ulp of the result
    + |rs| 3w 2^-24 (sum |a||b| + |bias|)   the f32 accumulation of the 3w exact products and the bias add, through the BatchNorm factor
    + 2^-23 (|y| + |rt|)           the f32 fmaf of the BatchNorm.
    y_0 equals bf16(fmaf(relu(z1_0), s1, t1)) bit for bit."""
    N, guard = 3, 3
    z1, s1, t1, ws, rb, rs, rt = _res2net_case(w, d, T, 100 * w + 10 * d + T)
    y = torch.full((N, T + guard, 8 * w), SENTINEL, dtype=BF16, device=DEV)
    ops.ecapa_res2net(z1.to(DEV), s1.to(DEV), t1.to(DEV), E.pack_res2net(ws).to(DEV), rb.to(DEV), rs.to(DEV), rt.to(DEV), T, w, d, y)
    torch.cuda.synchronize()
    y = y.cpu()
    assert (y[:, T:] == torch.tensor(SENTINEL, dtype=BF16)).all(), "rows behind a window's T frames were written"
    x = fma32(torch.relu(z1[:, :T].to(F32)), s1, t1)                                   # [N, T, 8w] f32
    assert (y[:, :T, :w].view(torch.int16) == x[:, :, :w].to(BF16).view(torch.int16)).all(), "y_0 is not the copied sub-band"
    worst = 0.0
    for i in range(1, 8):
        xi = x[:, :, i * w:(i + 1) * w]
        a = (xi + y[:, :T, (i - 1) * w:i * w].to(F32) if i >= 2 else xi).to(BF16).to(F64).numpy()
        wq = ws[i - 1].to(BF16).to(F64).numpy()
        sl = slice((i - 1) * w, i * w)
        b64, s64, t64 = rb[sl].to(F64).numpy(), rs[sl].to(F64).numpy(), rt[sl].to(F64).numpy()
        for n in range(N):
            pre = REF.conv3_reflect(a[n], wq, b64, d)
            want = np.maximum(pre, 0.0) * s64 + t64
            S = REF.conv3_reflect(np.abs(a[n]), np.abs(wq), np.abs(b64), d)
            bound = 2.0 ** -8 * np.abs(want) + np.abs(s64) * 3 * w * 2.0 ** -24 * S + 2.0 ** -23 * (np.abs(want) + np.abs(t64))
            err = np.abs(y[n, :T, i * w:(i + 1) * w].to(F64).numpy() - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (f"sub-band {i}, window {n}: max |d| {err.max():.3e}, worst err / bound {(err / bound).max():.2f} at "
                                          f"{np.unravel_index(int((err / bound).argmax()), err.shape)}")
    print(f"res2net w={w} d={d} T={T}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("w,d,T", [(16, 2, 5), (16, 4, 5), (48, 3, 21), (128, 4, 76), (128, 2, 21)])
def test_res2net_impulse_reproduces_the_taps(w, d, T):
    """A unit impulse at frame 0, 1, d or T - 1 (one window each) in the LAST channel of sub-band 1, identity BatchNorms, no bias and
    positive weights k / 64 (sums of three are exact in bf16): y_1[t, co] = sum of the taps whose (reflected) frame is the impulse's, to
    1e-6."""
    frames = (0, 1, d, T - 1)
    g = torch.Generator().manual_seed(7 * w + d + T)
    z1 = torch.zeros(len(frames), T, 8 * w)
    for n, f in enumerate(frames):
        z1[n, f, 2 * w - 1] = 1.0
    ws = [torch.randint(1, 33, (w, w, 3), generator=g).to(F32) / 64.0 for _ in range(7)]
    one, zero = torch.ones(8 * w), torch.zeros(8 * w)
    y = torch.zeros((len(frames), T, 8 * w), dtype=BF16, device=DEV)
    ops.ecapa_res2net(z1.to(BF16).to(DEV), one.to(DEV), zero.to(DEV), E.pack_res2net(ws).to(DEV), zero[:7 * w].to(DEV), one[:7 * w].to(DEV),
                      zero[:7 * w].to(DEV), T, w, d, y)
    torch.cuda.synchronize()
    y = y.cpu().to(F64).numpy()
    for n, f in enumerate(frames):
        want = REF.conv3_reflect(z1[n, :, w:2 * w].numpy(), ws[0].numpy(), np.zeros(w), d)
        assert np.abs(want).max() > 0
        assert np.abs(y[n, :, w:2 * w] - want).max() <= 1e-6, f"impulse at frame {f}: max |d| {np.abs(y[n, :, w:2 * w] - want).max():.3e}"


# ----------------------------------------------------------------------------- 3. the per-(window, channel) passes
@pytest.mark.parametrize("T", [5, 76])
def test_relu_bn_and_window_statistics(T):
    """Geometry a's 3C = 384 channels, three windows.  out = bf16(fmaf(relu(z), s, t)) bit for bit; the statistics are those of the
    rounded output, f32 sums of T terms in two passes (bounds at the assertions); one channel is constant over
    time and its std comes out at the clamp sqrt(1e-12)."""
    N, Cw = 3, 384
    g = torch.Generator().manual_seed(T)
    z = torch.randn(N * T, Cw, generator=g)
    z[:, 5] = 0.75
    z = z.to(BF16)
    s, t = 0.8 + 0.4 * torch.rand(Cw, generator=g), 0.2 * torch.randn(Cw, generator=g)
    out, sf, sb = ops.ecapa_relu_bn(z.to(DEV), s.to(DEV), t.to(DEV), N, T, want_stats=True)
    torch.cuda.synchronize()
    out, sf, sb = out.cpu(), sf.cpu(), sb.cpu()
    want = fma32(torch.relu(z.to(F32)), s, t).to(BF16)
    assert (out.view(torch.int16) == want.view(torch.int16)).all()
    o = want.to(F64).reshape(N, T, Cw)
    m = o.mean(1)
    sd = ((o - m[:, None]) ** 2).mean(1).clamp(min=1e-12).sqrt()
    tol = (T + 2) * 2.0 ** -24 * o.abs().amax(1)          # T f32 additions of terms <= max, each rounding <= 2^-24 T max; the division
    assert ((sf[:, :Cw].to(F64) - m).abs() <= tol).all()
    live = torch.ones(Cw, dtype=torch.bool)
    live[5] = False
    # the variance: the same kind of sum over squares <= max^2, plus 2 max |d mean| -- within 4 tol max (compared as variances: the
    # std of a channel that ReLU leaves nearly constant would amplify it)
    assert ((sf[:, Cw:].to(F64) ** 2 - sd ** 2).abs()[:, live] <= 4 * tol[:, live] * o.abs().amax(1)[:, live] + 1e-12).all()
    assert torch.isfinite(sf).all() and ((sf[:, Cw + 5] - 1e-6).abs() <= 1e-9).all(), "a constant channel's std must sit at the clamp"
    assert (sb.view(torch.int16) == sf.to(BF16).view(torch.int16)).all()
    plain = ops.ecapa_relu_bn(z.to(DEV), s.to(DEV), t.to(DEV), N, T)
    assert (plain.cpu().view(torch.int16) == want.view(torch.int16)).all()


@pytest.mark.parametrize("T", [5, 76])
def test_se_residual_lands_in_its_column_slice(T):
    """C = 128, SE 32, three windows; the residual comes from a 384-wide buffer (its first 128 columns) and the output goes to
    columns 128 .. 255 of a 384-wide concat buffer whose other columns hold a sentinel that must survive.  Against float64 on the same
    bf16 operands: 2^-8 |y| (output rounding) + 1e-5 (1 + |v|) for the f32 mean over T, the two small matrix products and the sigmoid."""
    N, Cw, se, ld = 3, 128, 32, 384
    g = torch.Generator().manual_seed(50 + T)
    z2 = torch.randn(N * T, Cw, generator=g).to(BF16)
    res = torch.randn(N * T, ld, generator=g).to(BF16)
    s, t = 0.8 + 0.4 * torch.rand(Cw, generator=g), 0.2 * torch.randn(Cw, generator=g)
    w1, b1 = torch.randn(se, Cw, generator=g) * (2.0 / Cw) ** 0.5, 0.1 * torch.randn(se, generator=g)
    w2, b2 = torch.randn(Cw, se, generator=g) * (2.0 / se) ** 0.5, 0.1 * torch.randn(Cw, generator=g)
    out = torch.full((N * T, ld), SENTINEL, dtype=BF16, device=DEV)
    d = lambda x: x.contiguous().to(DEV)
    _, mean, gate = ops.ecapa_se_residual(d(z2), d(s), d(t), d(w1.t()), d(b1), d(w2.t()), d(b2), d(res), out, 128, N, T)
    torch.cuda.synchronize()
    out = out.cpu()
    sent = torch.tensor(SENTINEL, dtype=BF16)
    assert (out[:, :128] == sent).all() and (out[:, 256:] == sent).all(), "the neighbouring columns of the concat buffer were written"
    v = (torch.relu(z2.to(F64)) * s.to(F64) + t.to(F64)).reshape(N, T, Cw)
    m = v.mean(1)
    gt = torch.sigmoid(torch.relu(m @ w1.to(F64).T + b1.to(F64)) @ w2.to(F64).T + b2.to(F64))
    assert ((mean.cpu().to(F64) - m).abs() <= 1e-5).all() and ((gate.cpu().to(F64) - gt).abs() <= 1e-5).all()
    want = v * gt[:, None] + res[:, :Cw].to(F64).reshape(N, T, Cw)
    err = (out[:, 128:256].to(F64).reshape(N, T, Cw) - want).abs()
    bound = 2.0 ** -8 * want.abs() + 1e-5 * (1 + v.abs())
    print(f"se/residual T={T}: max |d| {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("T", [5, 76])
def test_attention_activation_and_pooling(T):
    """A = 64 attention channels and 3C = 384 pooled channels, three windows.  Activation: tanh(fmaf(relu(g + per-window term), s, t))
    to 2^-8 |y| + 1e-6.  Pooling against float64 on the same operands: channel 3 has a logit of +30 at one frame (a peaked softmax:
    that frame's weight is 1 to 1e-5), channel 5 is constant over time (its std is the clamp 1e-6, not NaN); the weights of every
    (window, channel) sum to 1 within 1e-5 and match to 1e-6; mean and std to 2e-5 (1 + max |h|); the BatchNormed bf16 output to
    2^-8 |y| + 1e-4."""
    N, A, Cw = 3, 64, 384
    g = torch.Generator().manual_seed(90 + T)
    ga, pw = torch.randn(N * T, A, generator=g), torch.randn(N, A, generator=g)
    s, t = 0.8 + 0.4 * torch.rand(A, generator=g), 0.2 * torch.randn(A, generator=g)
    act = ops.ecapa_attn_act(ga.to(DEV), pw.to(DEV), s.to(DEV), t.to(DEV), N, T)
    torch.cuda.synchronize()
    v = ga.to(F64).reshape(N, T, A) + pw.to(F64)[:, None]
    want = torch.tanh(torch.relu(v) * s.to(F64) + t.to(F64)).reshape(N * T, A)
    assert ((act.cpu().to(F64) - want).abs() <= 2.0 ** -8 * want.abs() + 1e-6).all()

    lg = 3.0 * torch.randn(N, T, Cw, generator=g)
    lg[:, T // 2, 3] += 30.0
    h = torch.randn(N, T, Cw, generator=g)
    h[:, :, 5] = 0.625
    h = h.to(BF16)
    bs, bt = 0.8 + 0.4 * torch.rand(2 * Cw, generator=g), 0.2 * torch.randn(2 * Cw, generator=g)
    out, aw, pooled = ops.ecapa_asp_pool(lg.reshape(N * T, Cw).to(DEV), h.reshape(N * T, Cw).to(DEV), bs.to(DEV), bt.to(DEV), N, T)
    torch.cuda.synchronize()
    out, aw, pooled = out.cpu(), aw.cpu().reshape(N, T, Cw).to(F64), pooled.cpu()
    assert torch.isfinite(pooled).all() and torch.isfinite(out.to(F32)).all()
    a64 = torch.softmax(lg.to(F64), 1)
    h64 = h.to(F64)
    assert ((aw.sum(1) - 1).abs() <= 1e-5).all() and ((aw - a64).abs() <= 1e-6).all()
    assert ((aw[:, T // 2, 3] - 1).abs() <= 1e-5).all()
    m = (a64 * h64).sum(1)
    sd = (a64 * (h64 - m[:, None]) ** 2).sum(1).clamp(min=1e-12).sqrt()
    tol = 2e-5 * (1 + h64.abs().amax(1))
    assert ((pooled[:, :Cw].to(F64) - m).abs() <= tol).all()
    live = torch.ones(Cw, dtype=torch.bool)
    live[5] = False
    assert ((pooled[:, Cw:].to(F64) - sd).abs()[:, live] <= tol[:, live]).all()
    assert ((pooled[:, Cw + 5] - 1e-6).abs() <= 1e-9).all(), "a constant channel's std must sit at the clamp"
    want = torch.cat([m, sd], 1) * bs.to(F64) + bt.to(F64)
    assert ((out.to(F64) - want).abs() <= 2.0 ** -8 * want.abs() + 1e-4).all()


# ----------------------------------------------------------------------------- 4. whole model
def _figures(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (float(np.abs(got - want).max() / np.abs(want).max()),
            float(1.0 - (got @ want) / np.sqrt((got @ got) * (want @ want))))


@pytest.mark.parametrize("geom", ["a", "full"])
def test_whole_model_against_the_fixture(geom):
    """Every window of the fixture alone (76, 21 and 5 frames): relmax and 1 - cosine of the device's embedding against the fp32
    module's, gated at 1.5x the figures of the same modules in bfloat16 (read from the fixture).

    Measured on MI355X: see profiles/diarization.md."""
    fx = fixture(geom)
    m = model(geom)
    rows = []
    for i, w in enumerate(R.windows()):
        got = m.encode_batch(torch.from_numpy(w)[None])
        torch.cuda.synchronize()
        assert got.shape == (1, 1, R.GEOMS[geom]["lin_neurons"])
        ref = fx[f"emb_f32_{i}"]
        yard = torch.from_numpy(fx[f"emb_bf16_{i}"].view(np.int16).copy()).view(BF16).to(F64).numpy()
        dr, dc = _figures(got[0, 0].cpu().numpy(), ref)
        yr, yc = _figures(yard, ref)
        print(f"ecapa {geom} window {i} (T = {REF.frames_of(len(w))}): device relmax {dr:.3e} 1-cos {dc:.3e} | bf16 module relmax {yr:.3e} 1-cos {yc:.3e}")
        rows.append((i, dr, dc, yr, yc))
    for i, dr, dc, yr, yc in rows:
        assert dr <= MARGIN * yr, f"window {i}: relmax {dr:.3e} against {MARGIN} x {yr:.3e}"
        assert dc <= MARGIN * yc, f"window {i}: 1 - cosine {dc:.3e} against {MARGIN} x {yc:.3e}"


# ----------------------------------------------------------------------------- 5. windows do not mix
def test_windows_do_not_mix_and_chunking_changes_nothing():
    """Geometry a, 3333-sample windows (T = 21).  Replacing window 1's samples leaves the embeddings of windows 0 and 2 bit-identical;
    five overlapping windows of one buffer through chunks of two equal the single-chunk call bit for bit, and a window cut from the
    shared buffer equals the same samples passed alone."""
    m = model("a")
    g = np.random.default_rng(5)
    L = 3333
    wavs = (0.1 * g.standard_normal((3, L))).astype(np.float32)
    e0 = m.encode_batch(torch.from_numpy(wavs))[:, 0].cpu()
    wavs[1] = (0.3 * g.standard_normal(L)).astype(np.float32)
    e1 = m.encode_batch(torch.from_numpy(wavs))[:, 0].cpu()
    assert torch.equal(e0[0], e1[0]) and torch.equal(e0[2], e1[2]) and not torch.equal(e0[1], e1[1])
    audio = (0.1 * g.standard_normal(6000)).astype(np.float32)
    starts, lens = [0, 500, 1000, 1500, 3000], [L, L, L, L, 3000]
    whole = m.embed_windows(audio, starts, lens, L).cpu()
    m.chunk_windows = 2
    chunked = m.embed_windows(audio, starts, lens, L).cpu()
    print("chunked against whole: max |d|", float((chunked - whole).abs().max()))
    assert torch.equal(chunked, whole)
    alone = m.embed_windows(audio[500:500 + L], [0], [L], L).cpu()
    assert torch.equal(alone[0], whole[1])
    tail = m.embed_windows(REF.reflect_extend(audio[3000:], L).astype(np.float32), [0], [L], L).cpu()
    assert torch.equal(tail[0], whole[4]), "the reflected tail must equal the same window padded on the host"


def test_envelope_errors_name_the_limit():
    m = model("a")
    audio = np.zeros(100000, np.float32)
    with pytest.raises(ValueError, match="frames"):
        m.embed_windows(audio, [0], [500], 500)
    with pytest.raises(ValueError, match="reflect-padded"):
        m.embed_windows(audio, [0], [1000], 3333)
    with pytest.raises(ValueError, match="outside"):
        m.embed_windows(audio, [99000], [3333], 3333)

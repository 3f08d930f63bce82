"""The ragged encoder on the device: every clip of a batch encoded at its own mel length (``ta_attention_enc_fwd_varlen``,
``ta_encoder_forward_ragged``, ``GlmAsrEncoderMI355X.forward(mel_lengths=...)``, ``ASRModel(ragged_encoder=True)``).

Truth is the CPU oracle run on ONE clip at a time with unpadded features (``oracle.encoder.encoder_forward(x[b:b+1, :, :T_b])``,
``oracle.model.asr_forward`` on a one-clip batch), and float64 softmax for the attention kernel alone; the library's padded path is
never the truth.  Gates are the ones the existing tests apply to the same quantities -- no new number:
  attention   max|d| / max|ref| < 2e-2 per clip          tests/test_gpu_kernels.py::test_attention_enc_fwd
  encoder     rel-to-max < 2e-2 and cosine > 0.9995      tests/test_gpu_parity.py::test_encoder_true_width_vs_oracle, per clip
  logits      max|d| / max|ref| < 2e-2                   header of tests/test_gpu_packing.py
  nll         |d| < 2 * (2e-2 * max|ref logits|)         header of tests/test_gpu_packing.py
Everything else is bit-for-bit: isolation between clips, padding never read, equal lengths == the padded path, frame dropout.
All at true encoder width (H = 1280, 20 heads, 128 mel bins), 2 layers."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import encoder as OE
from oracle import model as OM
from oracle import weights as OW

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib, ops
    from tiny_audio_amd.asr_config import ASRConfig, EncoderConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    from tiny_audio_amd.encoder import GlmAsrEncoderMI355X
    from tiny_audio_amd.ops import ptr, stream
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments

DEV = "cuda"
BF16 = torch.bfloat16
TRUE_ENC = OW.enc_config(layers=2)
# odd and even T_b, S_b = 1 (twice), the 64 and 128 row boundaries and their neighbours, one full-length clip
T_LENS = [261, 1, 2, 33, 128, 129, 255, 77]
T_MAX = 261


def npy(t):
    return t.detach().float().cpu().numpy()


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


def s_of(t):
    return (t - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def enc_weights():
    return OW.init_encoder(TRUE_ENC, 0)


@functools.lru_cache(maxsize=None)
def encoder():
    return GlmAsrEncoderMI355X(EncoderConfig(TRUE_ENC), DEV).load_state_dict_hf(enc_weights())


@functools.lru_cache(maxsize=None)
def batch_x():
    return (0.6 * np.random.RandomState(3).standard_normal((len(T_LENS), 128, T_MAX))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_per_clip():
    """The encoder applied to every clip ALONE at its own length (computed once; read-only)."""
    x = batch_x()
    return tuple(OE.encoder_forward(x[b:b + 1, :, :t], enc_weights(), TRUE_ENC)[0] for b, t in enumerate(T_LENS))


def run(x, lens=None, res_f32=False, keep=None):
    """-> (bf16 output, f32 output) as numpy, through the encoder module (both outputs come out of one call of the composite)."""
    enc = encoder()
    enc.res_f32 = res_f32
    try:
        kw = {} if lens is None else dict(mel_lengths=lens)
        xt = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
        of = enc(xt, frame_keep=keep, return_f32=True, **kw).last_hidden_state
        ob = enc(xt, frame_keep=keep, return_f32=False, **kw).last_hidden_state
        return ob.cpu(), of.cpu()
    finally:
        enc.res_f32 = False


# ============================================================================ the attention kernel
def _qkv(rows, heads, seed):
    H = heads * 64
    g = torch.Generator().manual_seed(seed)
    return torch.cat([1.5 * torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g)],
                     1).to(DEV).to(BF16).contiguous()


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)


def test_attention_varlen_vs_float64_and_fixed_length_kernel():
    """Fewer rows than a fragment, the fragment / key-tile / query-tile boundaries and their neighbours, odd row offsets -- in one call."""
    heads, lens = 2, [1, 15, 16, 63, 64, 65, 127, 128, 129, 200]
    H, rows = heads * 64, sum(lens)
    qkv = _qkv(rows, heads, 1)
    cu = _cu(lens)
    GUARD, SENT = 64, 12345.0
    buf = torch.full((rows + 2 * GUARD, H), SENT, device=DEV, dtype=BF16)
    out = buf[GUARD:GUARD + rows]
    ops.attention_enc_fwd_varlen(qkv, cu, heads, max(lens), out=out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + rows:] == SENT).all())      # guard rows untouched
    assert bool(torch.isfinite(out.float()).all())
    at = 0
    for n in lens:
        sl = qkv[at:at + n]
        q, k, v = (sl[:, i * H:(i + 1) * H].double().reshape(n, heads, 64).transpose(0, 1) for i in range(3))
        ref = (torch.softmax(q @ k.transpose(-1, -2) * math.log(2.0), -1) @ v).transpose(0, 1).reshape(n, H)
        got = out[at:at + n].double()
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"clip of {n} rows at {at}: relerr {err:.3e}")
        assert err < 2e-2, (n, err)
        alone = ops.attention_enc_fwd(sl.contiguous(), 1, heads, n)
        assert torch.equal(alone, out[at:at + n]), n                                            # the same bits as the clip alone
        at += n
    assert _lib.lib().ta_attention_enc_fwd_varlen(ptr(qkv), ptr(out), None, len(lens), heads, max(lens), stream()) == 1


def test_attention_varlen_isolation():
    """A clip whose q | k | v rows are all NaN leaves its neighbours' outputs finite and bit-identical (the ragged last key tile
    of clip 0 ends one row short of clip 1's first row; its clamp must stop at clip 0's own last row)."""
    heads, lens = 2, [65, 70, 33]
    qkv = _qkv(sum(lens), heads, 2)
    cu = _cu(lens)
    a = ops.attention_enc_fwd_varlen(qkv, cu, heads, max(lens)).clone()
    bad = qkv.clone()
    bad[65:135] = float("nan")
    b = ops.attention_enc_fwd_varlen(bad, cu, heads, max(lens))
    for lo, hi in ((0, 65), (135, 168)):
        assert bool(torch.isfinite(a[lo:hi].float()).all()) and bool(torch.isfinite(b[lo:hi].float()).all())
        assert torch.equal(a[lo:hi], b[lo:hi])


# ============================================================================ the composite
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "f32-stream"])
def test_ragged_encoder_vs_oracle_clip_by_clip(res_f32):
    x, refs = batch_x(), oracle_per_clip()
    ob, of = run(x, T_LENS, res_f32)
    S = s_of(T_MAX)
    assert ob.shape == of.shape == (len(T_LENS), S, 1280) and ob.dtype == BF16 and of.dtype == torch.float32
    for b, t in enumerate(T_LENS):
        sb, ref = s_of(t), refs[b]
        assert ref.shape == (sb, 1280) and np.isfinite(ref).all()
        for name, o in (("bf16", ob), ("f32", of)):
            got = npy(o[b, :sb])
            r, c = relmax(got, ref), cosine(got, ref)
            print(f"T_b {t:3d} S_b {sb:3d} {name}: relmax {r:.3e} cosine {c:.6f}")
            assert r < 2e-2 and c > 0.9995, (t, name, r, c)
            assert float(o[b, sb:].float().abs().max()) == 0.0 if sb < S else True


@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "f32-stream"])
def test_padding_is_never_read_and_padding_rows_are_zero(res_f32):
    x = batch_x()
    xn, xz = x.copy(), x.copy()
    for b, t in enumerate(T_LENS):
        xn[b, :, t:] = np.nan
        xz[b, :, t:] = 0.0
    (nb, nf), (zb, zf) = run(xn, T_LENS, res_f32), run(xz, T_LENS, res_f32)
    for a, z in ((nb, zb), (nf, zf)):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, z)
        for b, t in enumerate(T_LENS):
            assert bool((a[b, s_of(t):] == 0).all())


def test_neighbours_do_not_leak():
    x = batch_x()
    other = (0.6 * np.random.RandomState(11).standard_normal(x.shape)).astype(np.float32)
    base_b, base_f = run(x, T_LENS)
    for keep_clip in (1, 3, 6):                       # S_b = 1, 17, 128
        y = other.copy()
        y[keep_clip] = x[keep_clip]
        ob, of = run(y, T_LENS)
        sb = s_of(T_LENS[keep_clip])
        assert torch.equal(ob[keep_clip, :sb], base_b[keep_clip, :sb]) and torch.equal(of[keep_clip, :sb], base_f[keep_clip, :sb])
        assert not torch.equal(ob[0], base_b[0])


@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "f32-stream"])
@pytest.mark.parametrize("B,T", [(2, 207), (8, 77)])
def test_equal_lengths_reduce_to_the_padded_path(B, T, res_f32):
    x = (0.6 * np.random.RandomState(3).standard_normal((B, 128, T))).astype(np.float32)
    (pb, pf), (rb, rf) = run(x, None, res_f32), run(x, [T] * B, res_f32)
    assert torch.equal(pb, rb) and torch.equal(pf, rf)


def test_frame_keep():
    x = batch_x()
    S = s_of(T_MAX)
    keep = (np.random.RandomState(4).rand(len(T_LENS), S) < 0.8).astype(np.float32)
    kt = torch.from_numpy(keep).reshape(-1)
    (fb, ff), (kb, kf) = run(x, T_LENS), run(x, T_LENS, keep=kt)
    real = np.zeros_like(keep, dtype=bool)
    for b, t in enumerate(T_LENS):
        real[b, :s_of(t)] = True
    kept, dropped = torch.from_numpy(real & (keep != 0)), torch.from_numpy(real & (keep == 0))
    assert int(dropped.sum()) > 0
    for full, masked in ((fb, kb), (ff, kf)):
        assert bool((masked[dropped] == 0).all())                     # exactly zero, no rescale
        assert torch.equal(masked[kept], full[kept])                  # kept frames: the unmasked run's bits
        assert bool((masked[torch.from_numpy(~real)] == 0).all())     # padding rows stay zero


def test_device_path_refusals():
    enc = encoder()
    L = _lib.lib()
    B, T = 3, 77
    S = s_of(T)
    x = torch.zeros((B, 128, T), device=DEV)
    out = torch.empty((B, S, 1280), device=DEV, dtype=BF16)

    def call(lens, ws_bytes=None):
        cu = [0]
        for t in lens:
            cu.append(cu[-1] + s_of(max(t, 1)))
        n = L.ta_encoder_ragged_workspace_bytes(C.byref(enc._w), B, T, cu[-1])
        ws = torch.empty(n, device=DEV, dtype=torch.uint8)
        cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
        return L.ta_encoder_forward_ragged(C.byref(enc._w), ptr(x), B, T, (C.c_int * B)(*lens), ptr(cud), None, ptr(out), None, ptr(ws),
                                           n if ws_bytes is None else ws_bytes(n), stream())

    assert call([77, 40, 1]) == 0
    assert call([77, 0, 40]) == 1                    # TA_ERR_ARG: a length of 0
    assert call([77, 78, 40]) == 1                   # ... of T + 1
    assert call([77, 40, 1], lambda n: n - 256) == 1  # ... a short workspace
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="mel_lengths"):
        enc(x, mel_lengths=[77, 0, 40])
    with pytest.raises(ValueError, match="mel_lengths"):
        enc(x, mel_lengths=[77, 40])


# ============================================================================ the whole model
TRUE_LM = OW.lm_config(vocab=5003, layers=2)
AID, PAD, EOS = 5002, 4990, 4991


@functools.lru_cache(maxsize=None)
def model_weights():
    return enc_weights(), OW.init_lm(TRUE_LM, 1), OW.init_mlp_projector(1280, 1024, 1024)


def build_model(**kw):
    wE, wL, wP = model_weights()
    cfg = ASRConfig(audio_config=TRUE_ENC, text_config=TRUE_LM, projector_hidden_dim=1024, audio_token_id=AID, pad_token_id=PAD,
                    eos_token_id=EOS)
    m = ASRModel(cfg, device=DEV, init="none", **kw)
    m.audio_tower.load_state_dict_hf(wE)
    m.language_model.load_state_dict_hf(wL)
    m.load_state_dict({"projector." + k: torch.from_numpy(v) for k, v in wP.items()})
    return m


def test_whole_model_ragged():
    lens = [261, 77, 130]
    B, T = len(lens), max(lens)
    x = (0.6 * np.random.RandomState(21).standard_normal((B, 128, T))).astype(np.float32)
    amask = (np.arange(T)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)
    counts = [(s_of(t) - 4) // 4 + 1 for t in lens]
    ids, att, lab, cnt = OW.synthetic_tokens(B, counts, TRUE_LM["vocab"], AID, PAD, EOS, n_text=10, n_suffix=4, ragged=True)
    wE, wL, wP = model_weights()
    W = dict(encoder=wE, lm=wL, projector=wP)
    ocfg = dict(enc=TRUE_ENC, lm=TRUE_LM, projector_type="mlp", k=4, audio_token_id=AID)
    refs = []
    for b, t in enumerate(lens):                      # every clip alone, unpadded features, its own token row
        n = int(att[b].sum())
        one = dict(input_ids=ids[b:b + 1, :n], attention_mask=att[b:b + 1, :n], labels=lab[b:b + 1, :n], input_features=x[b:b + 1, :, :t],
                   audio_token_counts=cnt[b:b + 1])
        r = OM.asr_forward(one, W, ocfg, keep_cache=False)
        lg = np.asarray(r["logits"][0], np.float64)
        tl = lab[b, 1:n]
        z = lg[:-1][tl != -100]
        nll = np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1)) + z.max(-1) - z[np.arange(len(z)), tl[tl != -100]]
        refs.append((n, lg, nll))
    m = build_model(ragged_encoder=True)
    assert m.ragged_encoder is True
    batch = dict(input_ids=torch.from_numpy(ids), input_features=torch.from_numpy(x), audio_attention_mask=torch.from_numpy(amask),
                 attention_mask=torch.from_numpy(att), labels=torch.from_numpy(lab), audio_token_counts=torch.from_numpy(cnt))

    def errors(out):
        nll_all, at, res = npy(out.nll).astype(np.float64), 0, []
        for b, (n, lg, nll) in enumerate(refs):
            got = npy(out.logits[b, :n]).astype(np.float64)
            k = len(nll)
            res.append((np.abs(got - lg).max() / np.abs(lg).max(), np.abs(nll_all[at:at + k] - nll).max(), 2 * 2e-2 * np.abs(lg).max()))
            at += k
        assert at == len(nll_all)
        return res

    m.eval()
    with torch.no_grad():
        on = errors(m(**batch))
        m.ragged_encoder = False
        off = errors(m(**batch))
        m.ragged_encoder = True
    for b, ((rl, dn, bound), (rl0, dn0, _)) in enumerate(zip(on, off)):
        print(f"clip {b} (T_b {lens[b]}): ragged logits relmax {rl:.3e} nll |d| {dn:.3e} (bound {bound:.3e}); padded logits relmax {rl0:.3e}")
        assert rl < 2e-2 and dn < bound, (b, rl, dn, bound)
    assert max(off[1][0], off[2][0]) > 2e-2, off      # the switch is read: padded to T = 261 the short clips miss the gate

    # one training step with the switch on: the forward's loss, finite gradients
    m.train()
    with torch.no_grad():
        fwd = float(m(**batch, num_items_in_batch=1.0, return_logits=False).loss)
    tr = ASRTrainer(m, TrainingArguments(gradient_accumulation_steps=8))      # no optimizer step inside this micro-batch
    ce = float(tr.training_step(batch))
    assert math.isfinite(ce) and abs(ce - fwd) <= 1e-5 * abs(fwd), (ce, fwd)
    grads = [p.grad for p in m.projector.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)

    # generate: clips of different lengths with equal placeholder counts (S_b = 67, 64, 65 -> 16 each), so the prompts need no padding
    glens = [133, 128, 130]
    gT = max(glens)
    gx = (0.6 * np.random.RandomState(22).standard_normal((3, 128, gT))).astype(np.float32)
    gy = (0.6 * np.random.RandomState(23).standard_normal((3, 128, gT))).astype(np.float32)
    gy[1, :, :glens[1]] = gx[1, :, :glens[1]]          # clip 1 keeps its audio; its padding and both neighbours change
    gmask = torch.from_numpy((np.arange(gT)[None, :] < np.asarray(glens)[:, None]).astype(np.int64))
    pid = torch.tensor([[5, 6] + [AID] * 16 + [7, 8]] * 3)
    kw = dict(input_ids=pid, audio_attention_mask=gmask, attention_mask=torch.ones_like(pid), max_new_tokens=6, eos_token_id=[])
    ta = m.generate(input_features=torch.from_numpy(gx), **kw).cpu()
    tb = m.generate(input_features=torch.from_numpy(gy), **kw).cpu()
    assert ta.shape == (3, 6) and torch.equal(ta[1], tb[1])
    with pytest.raises(ValueError, match="audio_attention_mask"):
        m(**{k: v for k, v in batch.items() if k != "audio_attention_mask"})

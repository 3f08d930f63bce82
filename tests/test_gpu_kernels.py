"""-m gpu: every primitive kernel of libta355.so, called through the C ABI, against a plain fp32
reference of the same op (torch on the same device, fp32 math).  Tolerances are stated per test:
bf16 operands (8 mantissa bits) with fp32 accumulation => relative error ~ 2^-8 on outputs."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import ops

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32



def _force_variant(monkeypatch, variant):
    """TA355_GEMM_VARIANT for the launches that follow (0, 3, 4, 5, 10, 12: every tile variant the library carries; any other
    number -- the plain 256-row tiles 1 / 2 and the experiment-only variants 6-9 / 11 of earlier rounds -- is the model's choice)."""
    monkeypatch.setenv("TA355_GEMM_VARIANT", variant)


def rnd(*shape, seed=0, scale=1.0, dtype=F32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def relerr(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def cos_sim(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 256, 128), (1000, 1280, 1280), (77, 384, 3840), (2048, 1024, 4096), (333, 1284, 128), (515, 5128, 64)])
@pytest.mark.parametrize("out_bf16", [True, False])
@pytest.mark.parametrize("variant", [None, "3", "4", "10", "12"])     # automatic choice; persistent ping-pong tiles (v4); one 192x128 tile per CU (v5)
def test_gemm_plain(M, N, K, out_bf16, variant, monkeypatch):
    if variant is not None:
        _force_variant(monkeypatch, variant)
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    C = ops.gemm_nt(A, W, out_dtype=BF16 if out_bf16 else F32)
    ref = A.float() @ W.float().T                      # asymmetric operands: a transposed store would not pass
    assert relerr(C, ref) < (1.5e-2 if out_bf16 else 2e-3)


def test_gemm_epilogues():
    M, N, K = 515, 640, 256
    A, W = rnd(M, K, seed=3, dtype=BF16), rnd(N, K, seed=4, scale=1 / math.sqrt(K), dtype=BF16)
    bias, res = rnd(N, seed=5), rnd(M, N, seed=6)
    ref = A.float() @ W.float().T + bias
    assert relerr(ops.gemm_nt(A, W, bias=bias, out_dtype=F32), ref) < 2e-3
    assert relerr(ops.gemm_nt(A, W, bias=bias, act=1, out_dtype=F32), torch.nn.functional.gelu(ref)) < 2e-3
    assert relerr(ops.gemm_nt(A, W, bias=bias, residual=res, out_dtype=F32), ref + res) < 2e-3
    inplace = res.clone()
    ops.gemm_nt(A, W, bias=bias, residual=inplace, out=inplace)
    assert relerr(inplace, ref + res) < 2e-3
    assert relerr(ops.gemm_nt(A, W, bias=bias, act=1, out_dtype=BF16), torch.nn.functional.gelu(ref)) < 1.5e-2


@pytest.mark.parametrize("variant", ["3", "4", "12"])
def test_gemm_gelu_chord_table(variant, monkeypatch):
    """The persistent ping-pong kernel evaluates erf-GELU through the 1024-chord table of csrc/gelu_lut.h staged in LDS
    (round 3): f32 output against torch's exact GELU, |error| <= 2.5e-5 + fp32 accumulation noise; TA355_GELU_LUT=0 (the
    arithmetic form) gives the same values to that tolerance; inputs far outside the table's range take the end chords."""
    _force_variant(monkeypatch, variant)
    M, N, K = 700, 640, 256
    A, W = rnd(M, K, seed=3, dtype=BF16), rnd(N, K, seed=4, scale=2.5 / math.sqrt(K), dtype=BF16)
    bias = rnd(N, seed=5)
    bias[:8] = torch.tensor([-30.0, 30.0, -9.0, 9.0, -8.0, 8.0, 1e4, -1e4], device=DEV)        # beyond [-8, 8): GELU -> 0 resp. x
    pre = A.float() @ W.float().T + bias
    ref = torch.nn.functional.gelu(pre)
    out = ops.gemm_nt(A, W, bias=bias, act=1, out_dtype=F32)
    assert float((out - ref).abs()[:, 8:].max()) < 1e-4, float((out - ref).abs()[:, 8:].max())
    assert relerr(out[:, :8], ref[:, :8]) < 1e-5
    monkeypatch.setenv("TA355_GELU_LUT", "0")
    out0 = ops.gemm_nt(A, W, bias=bias, act=1, out_dtype=F32)
    assert float((out0 - ref).abs()[:, 8:].max()) < 1e-4 and not torch.equal(out0, out)
    monkeypatch.delenv("TA355_GELU_LUT")
    assert relerr(ops.gemm_nt(A, W, bias=bias, act=1, out_dtype=BF16), ref) < 1.5e-2


@pytest.mark.parametrize("M,N,K", [(200, 64, 256), (1000, 1024, 1024), (6144, 4096, 1024), (4100, 1024, 3072)])
@pytest.mark.parametrize("variant", [None, "0", "3", "4", "10", "12"])
def test_gemm_k_extension(M, N, K, variant, monkeypatch):
    """C = A W^T + A2 W2^T in one launch (one extra 64-wide K tile: the fused LoRA update), every tile variant."""
    if variant is not None:
        _force_variant(monkeypatch, variant)
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    A2, W2 = rnd(M, 64, seed=3, dtype=BF16), rnd(N, 64, seed=4, scale=0.2, dtype=BF16)
    res = rnd(M, N, seed=5)
    ref = A.float() @ W.float().T + A2.float() @ W2.float().T
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32, k_ext=(A2, W2)), ref) < 2e-3
    assert relerr(ops.gemm_nt(A, W, out_dtype=BF16, k_ext=(A2, W2)), ref) < 1.5e-2
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32, residual=res, k_ext=(A2, W2)), ref + res) < 2e-3
    # one-shot: the next call is a plain GEMM again
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32), A.float() @ W.float().T) < 2e-3


def _gemm_with_logged_variant(A, W):
    """(C, tile variant the launch log records) of one plain bf16 GEMM under the current TA355_GEMM_VARIANT."""
    import ctypes as C
    from tiny_audio_amd import _lib
    L = _lib.lib()
    ops.sync_gemm_knobs()
    L.ta_profile_gemm(2)
    try:
        out = ops.gemm_nt(A, W, out_dtype=BF16)
        torch.cuda.synchronize()
        n = L.ta_profile_gemm_log(None, 0)
        buf = (C.c_long * (n * 24))()
        L.ta_profile_gemm_log(C.cast(buf, C.c_void_p), n)
    finally:
        L.ta_profile_gemm(0)
    assert n == 1, n
    return out, buf[20]                                   # field 20 of a log row: the tile variant as launched


_UNFORCED = {}


@pytest.mark.parametrize("forced", ["1", "2", "7", "11", "13"])
def test_gemm_forced_variant_the_library_does_not_carry_is_the_models_choice(forced, monkeypatch):
    """TA355_GEMM_VARIANT with a number that has no row in the variant table (the removed plain 256-row tiles 1 / 2, the
    experiment-only 7 / 11, anything above 12) launches what the model chooses: the same logged variant, the same bits."""
    M, N, K = 300, 256, 128
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    if not _UNFORCED:
        monkeypatch.delenv("TA355_GEMM_VARIANT", raising=False)
        _UNFORCED["out"], _UNFORCED["variant"] = _gemm_with_logged_variant(A, W)
    _force_variant(monkeypatch, forced)
    out, variant = _gemm_with_logged_variant(A, W)
    assert variant == _UNFORCED["variant"], (variant, _UNFORCED["variant"])
    assert torch.equal(out, _UNFORCED["out"])


@pytest.mark.parametrize("splits", [2, 5, 16])
@pytest.mark.parametrize("variant", [None, "4", "10", "12"])
def test_gemm_splitk(splits, variant, monkeypatch):
    if variant is not None:
        _force_variant(monkeypatch, variant)
    M, N, K = 200, 256, 64 * 37
    A, W = rnd(M, K, seed=7, dtype=BF16), rnd(N, K, seed=8, scale=1 / math.sqrt(K), dtype=BF16)
    ref = A.float() @ W.float().T
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32, splits=splits), ref) < 2e-3
    add = rnd(M, N, seed=9)
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32, splits=splits, residual=add), ref + add) < 2e-3


@pytest.mark.parametrize("variant", [None, "4", "10", "12"])
def test_gemm_conv_rowmap(variant, monkeypatch):
    """Conv1d(k=3, pad=1, stride s) as a row-mapped GEMM over a zero-padded time-major buffer."""
    if variant is not None:
        _force_variant(monkeypatch, variant)
    B, T, Cin, Cout = 3, 37, 128, 256
    x = rnd(B, Cin, T, seed=10)
    w = rnd(Cout, Cin, 3, seed=11, scale=1 / math.sqrt(3 * Cin))
    bias = rnd(Cout, seed=12)
    xp = torch.zeros(B, T + 2, Cin, device=DEV, dtype=BF16)
    xp[:, 1:T + 1] = x.transpose(1, 2).to(BF16)
    wp = w.permute(0, 2, 1).reshape(Cout, 3 * Cin).to(BF16).contiguous()
    for stride in (1, 2):
        S = (T + 2 - 3) // stride + 1
        out = ops.gemm_nt(xp, wp, M=B * S, N=Cout, K=3 * Cin, bias=bias, out_dtype=F32,
                          a_map=(stride * Cin, S, (T + 2) * Cin))
        ref = torch.nn.functional.conv1d(xp[:, 1:T + 1].float().transpose(1, 2), wp.float().reshape(Cout, 3, Cin).permute(0, 2, 1),
                                         bias, stride=stride, padding=1)
        assert relerr(out.reshape(B, S, Cout), ref.transpose(1, 2)) < 2e-3
    # mapped output: rows land at offset +1 row inside a padded [B, T+2, Cout] buffer, pad rows untouched
    outp = torch.full((B, T + 2, Cout), 7.0, device=DEV, dtype=BF16)
    ops.gemm_nt(xp, wp, M=B * T, N=Cout, K=3 * Cin, bias=bias, out=outp, a_map=(Cin, T, (T + 2) * Cin),
                c_map=(Cout, T, (T + 2) * Cout, Cout))
    ref = torch.nn.functional.conv1d(xp[:, 1:T + 1].float().transpose(1, 2), wp.float().reshape(Cout, 3, Cin).permute(0, 2, 1),
                                     bias, stride=1, padding=1).transpose(1, 2)
    assert relerr(outp[:, 1:T + 1], ref) < 1.5e-2
    assert float(outp[:, 0].float().min()) == 7.0 and float(outp[:, T + 1].float().max()) == 7.0


# ----------------------------------------------------------------------------- norms
@pytest.mark.parametrize("H", [256, 1280, 5120])
def test_layernorm(H):
    M = 333
    x, w, b = rnd(M, H, seed=1, scale=3.0) + 0.5, 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    rs = (torch.arange(M, device=DEV) % 3 != 0).float()
    yb, yf = ops.layernorm(x, w, b, 1e-5, rowscale=rs, out_bf16=True, out_f32=True)
    ref = torch.nn.functional.layer_norm(x, (H,), w, b, 1e-5) * rs[:, None]
    assert relerr(yf, ref) < 1e-5
    assert relerr(yb, ref) < 8e-3


@pytest.mark.parametrize("H,gelu", [(1024, False), (1024, True), (2048, False), (5120, False), (128, True)])
def test_rmsnorm_fwd_bwd(H, gelu):
    M = 301
    x = rnd(M, H, seed=1, scale=2.0).requires_grad_(True)
    w = (1 + 0.1 * rnd(H, seed=2)).requires_grad_(True)
    dy = rnd(M, H, seed=3)
    dres = rnd(M, H, seed=4)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6)
    y = w * (x * r)
    if gelu:
        y = torch.nn.functional.gelu(y)
    y.backward(dy)
    yb, yf, rstd = ops.rmsnorm_fwd(x.detach(), w.detach(), 1e-6, act_gelu=gelu, out_bf16=True, out_f32=True)
    assert relerr(yf, y) < 1e-5 and relerr(yb, y) < 8e-3 and relerr(rstd, r.flatten()) < 1e-5
    dx, dxb, dw = ops.rmsnorm_bwd(dy, x.detach(), rstd, w.detach(), dres=dres, act_gelu=gelu, want_dw=True)
    assert relerr(dx, x.grad + dres) < 2e-5
    assert relerr(dxb, x.grad + dres) < 8e-3
    assert relerr(dw, w.grad) < 1e-4


# ----------------------------------------------------------------------------- attention
def ref_attention(q, k, v, causal, scale, kmask=None):
    """q [B,Hq,L,d], k/v [B,Hkv,L,d] fp32 (autograd-capable)."""
    B, Hq, L, d = q.shape
    g = Hq // k.shape[1]
    kr, vr = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    s = (q @ kr.transpose(-1, -2)) * scale
    allow = torch.ones(B, 1, L, L, dtype=torch.bool, device=q.device)
    if causal:
        allow = allow & torch.tril(torch.ones(L, L, dtype=torch.bool, device=q.device))
    if kmask is not None:
        allow = allow & (kmask[:, None, None, :] != 0)
    s = s.masked_fill(~allow, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)
    return p @ vr, torch.logsumexp(s, -1)


def to_T(x, Lp):
    B, H, L, d = x.shape
    out = torch.zeros(B, H, d, Lp, device=x.device, dtype=x.dtype)
    out[..., :L] = x.transpose(-1, -2)
    return out.contiguous()


@pytest.mark.parametrize("hd,Hq,Hkv,L,causal,masked", [(64, 4, 4, 500, False, False), (64, 3, 3, 64, False, False),
                                                       (128, 4, 2, 192, True, True), (128, 2, 1, 70, True, False),
                                                       (128, 4, 2, 257, True, True)])
def test_attention_fwd(hd, Hq, Hkv, L, causal, masked):
    B = 2
    q, k, v = rnd(B, Hq, L, hd, seed=1), rnd(B, Hkv, L, hd, seed=2), rnd(B, Hkv, L, hd, seed=3)
    kmask = None
    if masked:
        kmask = torch.ones(B, L, dtype=torch.int32, device=DEV)
        kmask[1, L - 37:] = 0
    qb, kb, vb = q.to(BF16), k.to(BF16), v.to(BF16)
    scale = hd ** -0.5
    O, lse = ops.attention_fwd(qb.contiguous(), kb.contiguous(), to_T(vb, ops.pad64(L)), L, causal, scale, kmask)
    ref, ref_lse = ref_attention(qb.float(), kb.float(), vb.float(), causal, scale, kmask)
    ref = ref.transpose(1, 2).reshape(B * L, Hq * hd)
    assert relerr(O, ref) < 2e-2, relerr(O, ref)
    assert float((lse - ref_lse).abs().max()) < 2e-2


@pytest.mark.parametrize("L,masked", [(192, True), (64, False), (150, True)])
def test_attention_bwd(L, masked):
    B, Hq, Hkv, hd = 2, 4, 2, 128
    q, k, v = (rnd(B, h, L, hd, seed=s).to(BF16).float().requires_grad_(True) for h, s in ((Hq, 1), (Hkv, 2), (Hkv, 3)))
    dO = rnd(B * L, Hq * hd, seed=4).to(BF16)
    kmask = None
    if masked:
        kmask = torch.ones(B, L, dtype=torch.int32, device=DEV)
        kmask[0, L - 20:] = 0
    scale = hd ** -0.5
    ref, _ = ref_attention(q, k, v, True, scale, kmask)
    ref_tok = ref.transpose(1, 2).reshape(B * L, Hq * hd)
    valid_q = torch.ones(B, L, dtype=torch.bool, device=DEV) if kmask is None else (kmask != 0)
    dO_eff = dO.float() * valid_q.reshape(B * L, 1)            # padded query rows carry no gradient in the model
    ref_tok.backward(dO_eff)
    Lp = ops.pad64(L)
    qb, kb, vb = q.detach().to(BF16), k.detach().to(BF16), v.detach().to(BF16)
    O, lse = ops.attention_fwd(qb, kb, to_T(vb, Lp), L, True, scale, kmask)
    dOb = dO_eff.to(BF16).contiguous()
    delta, dOT = ops.attn_bwd_prep(dOb, O, B, Hq, L)
    ref_delta = (dOb.float() * O.float()).reshape(B, L, Hq, hd).sum(-1).transpose(1, 2)
    assert relerr(delta, ref_delta) < 1e-3
    assert relerr(dOT[..., :L], dOb.reshape(B, L, Hq, hd).permute(0, 2, 3, 1)) == 0.0
    dQ, dK, dV = ops.attention_bwd(qb, to_T(qb, Lp), kb, to_T(kb, Lp), vb, dOb, dOT, lse, delta, L, True, scale, kmask)
    assert cos_sim(dQ, q.grad) > 0.999 and relerr(dQ, q.grad) < 3e-2
    assert cos_sim(dK, k.grad) > 0.999 and relerr(dK, k.grad) < 3e-2
    assert cos_sim(dV, v.grad) > 0.999 and relerr(dV, v.grad) < 3e-2


# ----------------------------------------------------------------------------- RoPE / QK-norm
def rope_tables(n, rot, theta):
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=F32) / rot))
    f = torch.arange(n, dtype=F32)[:, None] * inv[None]
    return f.cos().to(DEV).contiguous(), f.sin().to(DEV).contiguous()


def rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def test_enc_qkv_post():
    B, H, S = 2, 5, 77
    qkv = rnd(B * S, 3 * H * 64, seed=1).to(BF16)
    cos, sin = rope_tables(128, 32, 10000.0)
    Q, K, VT = ops.enc_qkv_post(qkv, cos, sin, B, H, S)
    x = qkv.float().reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)          # [3,B,H,S,64]
    c = torch.cat([cos[:S], cos[:S]], -1)[None, None]; s = torch.cat([sin[:S], sin[:S]], -1)[None, None]

    def rope(t):
        r = t[..., :32] * c + rot_half(t[..., :32]) * s
        return torch.cat([r, t[..., 32:]], -1)
    assert relerr(Q, rope(x[0])) < 8e-3 and relerr(K, rope(x[1])) < 8e-3
    assert relerr(VT[..., :S], x[2].transpose(-1, -2)) == 0.0
    assert float(VT[..., S:].float().abs().max()) == 0.0


def test_lm_qkv_post_fwd_bwd():
    B, Hq, Hkv, L, hd = 2, 4, 2, 70, 128
    NQKV = (Hq + 2 * Hkv) * hd
    x0 = rnd(B * L, NQKV, seed=1).to(BF16)
    qn, kn = (1 + 0.1 * rnd(hd, seed=2)).requires_grad_(True), (1 + 0.1 * rnd(hd, seed=3)).requires_grad_(True)
    cos, sin = rope_tables(256, hd, 1e6)
    Q, K, V, QT, KT, VT, rq, rk = ops.lm_qkv_post_fwd(x0, qn.detach(), kn.detach(), cos, sin, B, Hq, Hkv, L)
    xf = x0.float().requires_grad_(True)
    xs = xf.reshape(B, L, Hq + 2 * Hkv, hd)
    c = torch.cat([cos[:L], cos[:L]], -1)[None, :, None]; s = torch.cat([sin[:L], sin[:L]], -1)[None, :, None]

    def nr(t, w):
        r = torch.rsqrt((t * t).mean(-1, keepdim=True) + 1e-6)
        n = w * (t * r)
        return n * c + rot_half(n) * s, r
    q_ref, rq_ref = nr(xs[:, :, :Hq], qn)
    k_ref, rk_ref = nr(xs[:, :, Hq:Hq + Hkv], kn)
    v_ref = xs[:, :, Hq + Hkv:]
    assert relerr(Q, q_ref.transpose(1, 2)) < 8e-3 and relerr(K, k_ref.transpose(1, 2)) < 8e-3
    assert relerr(V, v_ref.transpose(1, 2)) == 0.0
    assert relerr(rq, rq_ref.reshape(B * L, Hq)) < 1e-5 and relerr(rk, rk_ref.reshape(B * L, Hkv)) < 1e-5
    for T_, X_ in ((QT, Q), (KT, K), (VT, V)):
        assert relerr(T_[..., :L], X_.transpose(-1, -2)) == 0.0 and float(T_[..., L:].float().abs().max()) == 0.0
    dQ, dK, dV = rnd(B, Hq, L, hd, seed=5).to(BF16), rnd(B, Hkv, L, hd, seed=6).to(BF16), rnd(B, Hkv, L, hd, seed=7).to(BF16)
    (q_ref * dQ.float().transpose(1, 2)).sum().add((k_ref * dK.float().transpose(1, 2)).sum()).add(
        (v_ref * dV.float().transpose(1, 2)).sum()).backward()
    dqn, dkn = torch.full((hd,), 1.0, device=DEV), torch.zeros(hd, device=DEV)
    dqkv = ops.lm_qkv_post_bwd(dQ, dK, dV, x0, rq, rk, qn.detach(), kn.detach(), cos, sin, B, Hq, Hkv, L, dqn=dqn, dkn=dkn)
    assert relerr(dqkv, xf.grad) < 1e-2 and cos_sim(dqkv, xf.grad) > 0.9999
    assert relerr(dqn - 1.0, qn.grad) < 2e-3 and relerr(dkn, kn.grad) < 2e-3       # q_norm / k_norm weight gradients (+=)
    assert relerr(ops.lm_qkv_post_bwd(dQ, dK, dV, x0, rq, rk, qn.detach(), kn.detach(), cos, sin, B, Hq, Hkv, L), dqkv) == 0.0


@pytest.mark.parametrize("L,masked", [(192, True), (70, False), (150, True), (33, False)])
def test_attention_fwd_with_fused_qkv_post(L, masked):
    """ta_attention_fwd_qkv (QK-norm + RoPE + head split in the attention kernel's staging, V read transposed out of its row tile)
    against ta_lm_qkv_post_fwd followed by ta_attention_fwd."""
    B, Hq, Hkv, hd = 2, 4, 2, 128
    NQKV = (Hq + 2 * Hkv) * hd
    x0 = rnd(B * L, NQKV, seed=1).to(BF16)
    qn, kn = 1 + 0.1 * rnd(hd, seed=2), 1 + 0.1 * rnd(hd, seed=3)
    cos, sin = rope_tables(256, hd, 1e6)
    Q, K, V, QT, KT, VT, rq, rk = ops.lm_qkv_post_fwd(x0, qn, kn, cos, sin, B, Hq, Hkv, L)
    kmask = None
    if masked:
        kmask = torch.ones(B, L, dtype=torch.int32, device=DEV); kmask[1, L - 9:] = 0
    scale = hd ** -0.5
    O, lse = ops.attention_fwd(Q, K, VT, L, True, scale, kmask=kmask)
    O2, lse2, Q2, K2, V2, rq2, rk2 = ops.attention_fwd_qkv(x0, qn, kn, cos, sin, B, Hq, Hkv, L, scale, kmask=kmask)
    assert torch.equal(V2, V)
    assert relerr(rq2, rq) < 1e-6 and relerr(rk2, rk) < 1e-6
    assert relerr(Q2, Q) < 4e-3 and relerr(K2, K) < 4e-3          # the sums of squares are reduced in a different order: last-bit differences of 1/rms
    assert relerr(O2, O) < 1e-2 and cos_sim(O2, O) > 0.9999
    assert float((lse2 - lse).abs().max()) < 2e-2


@pytest.mark.parametrize("L,masked", [(192, True), (70, False), (150, True)])
def test_attention_bwd_with_fused_qkv_post(L, masked):
    """ta_attention_bwd_qkv (RoPE^T + per-head RMSNorm backward + head-major -> token-major in the epilogue, from the f32
    accumulators) against ta_attention_bwd followed by ta_lm_qkv_post_bwd (which rounds dQ / dK / dV to bf16 in between)."""
    B, Hq, Hkv, hd = 2, 4, 2, 128
    NQKV = (Hq + 2 * Hkv) * hd
    x0 = rnd(B * L, NQKV, seed=1).to(BF16)
    qn, kn = 1 + 0.1 * rnd(hd, seed=2), 1 + 0.1 * rnd(hd, seed=3)
    cos, sin = rope_tables(256, hd, 1e6)
    Q, K, V, QT, KT, VT, rq, rk = ops.lm_qkv_post_fwd(x0, qn, kn, cos, sin, B, Hq, Hkv, L)
    kmask = None
    if masked:
        kmask = torch.ones(B, L, dtype=torch.int32, device=DEV); kmask[1, L - 9:] = 0
    scale = hd ** -0.5
    O, lse = ops.attention_fwd(Q, K, VT, L, True, scale, kmask=kmask)
    dO = rnd(B * L, Hq * hd, seed=9).to(BF16)
    delta, dOT = ops.attn_bwd_prep(dO, O, B, Hq, L)
    dQ, dK, dV = ops.attention_bwd(Q, QT, K, KT, V, dO, dOT, lse, delta, L, True, scale, kmask=kmask)
    ref = ops.lm_qkv_post_bwd(dQ, dK, dV, x0, rq, rk, qn, kn, cos, sin, B, Hq, Hkv, L)
    got = ops.attention_bwd_qkv(Q, K, V, dO, lse, delta, x0, rq, rk, qn, kn, cos, sin, L, scale, kmask=kmask)
    assert torch.isfinite(got.float()).all()
    assert relerr(got, ref) < 1.5e-2 and cos_sim(got, ref) > 0.9999
    # the v section is a pure relayout of the same accumulators: identical
    assert torch.equal(got.view(B * L, Hq + 2 * Hkv, hd)[:, Hq + Hkv:], ref.view(B * L, Hq + 2 * Hkv, hd)[:, Hq + Hkv:])
    # round 6: V = NULL -- the kernel reads the V rows in place from the q|k|v GEMM output (same values: bit-identical result)
    got2 = ops.attention_bwd_qkv(Q, K, None, dO, lse, delta, x0, rq, rk, qn, kn, cos, sin, L, scale, kmask=kmask)
    assert torch.equal(got2, got)


# ----------------------------------------------------------------------------- element-wise / movement
def test_swiglu():
    M, F = 300, 768
    gu = rnd(M, 2 * F, seed=1).to(BF16)
    g, u = gu.float()[:, :F].clone().requires_grad_(True), gu.float()[:, F:].clone().requires_grad_(True)
    act = torch.nn.functional.silu(g) * u
    assert relerr(ops.swiglu_fwd(gu, F), act) < 8e-3
    d = rnd(M, F, seed=2).to(BF16)
    act.backward(d.float())
    dgu = ops.swiglu_bwd(d, gu, F)
    assert relerr(dgu[:, :F], g.grad) < 1e-2 and relerr(dgu[:, F:], u.grad) < 1e-2


def test_cast_transpose():
    x = rnd(130, 200, seed=1)
    assert relerr(ops.cast_bf16(x), x) < 4e-3
    t = ops.transpose_to_bf16(x, ld_out=192)
    assert torch.equal(t[:, :130], x.to(BF16).T.contiguous()) and float(t[:, 130:].float().abs().max()) == 0.0
    xb = rnd(4, 50, 64, seed=2).to(BF16)      # frame-stack row map: rows (b, n) = 4 frames, tail frames dropped
    N = (50 - 4) // 4 + 1
    xs = xb[:, :N * 4].reshape(4 * N, 256)
    from tiny_audio_amd import _lib
    out = torch.empty(256, 64, device=DEV, dtype=BF16)
    _lib.check(_lib.lib().ta_transpose_to_bf16(ops.ptr(xb), 0, 256, 50 * 64, N, ops.ptr(out), 64, 4 * N, 256, ops.stream()))
    assert torch.equal(out[:, :4 * N], xs.T.contiguous()) and float(out[:, 4 * N:].float().abs().max()) == 0.0


def test_audio_index_and_scatter():
    from oracle import model as OM
    B, L, N, D, V, AID = 3, 40, 9, 64, 100, 99
    rng = np.random.RandomState(0)
    ids = rng.randint(0, 90, (B, L)).astype(np.int64)
    counts = np.array([9, 4, 11])                 # last sample asks for more rows than the projector produced
    for b, c in enumerate(counts):
        ids[b, 2:2 + c] = AID
    y = rng.standard_normal((B, N, D)).astype(np.float32)
    emb = rng.standard_normal((V, D)).astype(np.float32)
    ref = OM.masked_scatter_rows(emb[ids], ids == AID, OM.gather_audio_embeds(y, counts))
    ids_d, counts_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(counts).to(DEV)     # keep every operand alive:
    emb_d, y_d = torch.from_numpy(emb).to(DEV), torch.from_numpy(y).to(DEV)               # raw pointers hold no refs
    src = ops.audio_index(ids_d, counts_d, N, AID)
    x0 = torch.empty(B * L, D, device=DEV)
    from tiny_audio_amd import _lib
    _lib.check(_lib.lib().ta_embed_scatter(ops.ptr(ids_d), ops.ptr(src), ops.ptr(emb_d), ops.ptr(y_d), ops.ptr(x0), None,
                                           B * L, D, V, ops.stream()))
    np.testing.assert_array_equal(x0.cpu().numpy().reshape(B, L, D), ref)
    dx0 = torch.randn(B * L, D, device=DEV)
    dy = torch.zeros(B * N, D, device=DEV)
    _lib.check(_lib.lib().ta_audio_grad_gather(ops.ptr(src), ops.ptr(dx0), ops.ptr(dy), B * L, D, ops.stream()))
    s = src.cpu().numpy()
    ref_dy = np.zeros((B * N, D), np.float32)
    ref_dy[s[s >= 0]] = dx0.cpu().numpy()[s >= 0]
    np.testing.assert_array_equal(dy.cpu().numpy(), ref_dy)


def test_label_rows_and_cross_entropy():
    B, L, V, Vp = 3, 50, 1000 + 3, 1024
    labels = torch.full((B, L), -100, dtype=torch.int64)
    labels[0, 10:30] = torch.randint(0, V, (20,)); labels[1, 0:5] = torch.randint(0, V, (5,)); labels[2, 49] = 7
    rows, tg, n = ops.label_rows(labels.to(DEV))
    n = int(n.item())
    shift = torch.cat([labels[:, 1:], torch.full((B, 1), -100)], 1).reshape(-1)
    exp_rows = torch.nonzero(shift != -100).flatten()
    assert n == exp_rows.numel()
    assert torch.equal(rows[:n].cpu().long(), exp_rows) and torch.equal(tg[:n].cpu(), shift[exp_rows])
    logits = rnd(n, Vp, seed=3, scale=3.0)
    logits[:, V:] = 50.0                                         # padding columns must be ignored
    scale = 1.0 / n
    loss, nll, dl = ops.cross_entropy(logits, tg[:n].contiguous(), V, scale)
    lf = logits[:, :V].clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, tg[:n], reduction="sum") * scale
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-4 * float(ref)
    assert relerr(dl[:, :V], lf.grad) < 1e-2 and float(dl[:, V:].float().abs().max()) == 0.0
    lb = logits.to(BF16)
    loss_b, _, _ = ops.cross_entropy(lb, tg[:n].contiguous(), V, scale)
    ref_b = torch.nn.functional.cross_entropy(lb[:, :V].float(), tg[:n], reduction="sum") * scale
    assert abs(float(loss_b) - float(ref_b)) < 1e-4 * float(ref_b)


def test_cross_entropy_loss_is_deterministic():
    """The loss is the per-row nll summed in row order by one workgroup: the same bits on every call (the bench's 1152 label rows)."""
    n, V, Vp = 1152, 4093, 4096
    logits = rnd(n, Vp, seed=21, scale=3.0).to(BF16)
    tg = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(22)).to(DEV)
    runs = [ops.cross_entropy(logits, tg, V, 1.0 / n) for _ in range(3)]
    for loss, nll, dl in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(nll, runs[0][1]) and torch.equal(dl, runs[0][2])
    ref = float(runs[0][1].double().sum() / n)
    assert abs(float(runs[0][0]) - ref) < 1e-5 * ref
    ref_t = torch.nn.functional.cross_entropy(logits[:, :V].float(), tg, reduction="sum") / n
    assert abs(float(runs[0][0]) - float(ref_t)) < 1e-4 * float(ref_t)


def test_adamw_and_clip():
    n = 10007
    p0, g = rnd(n, seed=1), rnd(n, seed=2, scale=3.0)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=0.01)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sq = torch.zeros(1, device=DEV)
    cnt = torch.full((1,), 4.0, device=DEV)
    for step in (1, 2, 3):
        gs = g * step
        pt.grad = (gs / 4.0).clone()
        torch.nn.utils.clip_grad_norm_([pt], 1.0)
        opt.step()
        sq.zero_()
        ops.grad_sqnorm(gs, sq)
        assert abs(float(sq) - float((gs.double() ** 2).sum())) < 1e-4 * float(sq)
        ops.adamw_step(p, gs, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, sqnorm=sq, max_norm=1.0, denom=cnt)
    d = (p - pt.detach()).abs()
    assert float(d.mean()) < 1e-7 and float(d.max()) < 3e-4


def test_grad_sqnorm_is_bit_reproducible():
    """ta_grad_sqnorm must give the SAME float for the same gradient whatever order its blocks finish in: data-parallel ranks compute
    the clip coefficient from it independently, and a last-bit difference makes their replicas drift apart (rounds 1-4 used one float
    atomicAdd per block).  6.3 M elements (the MLP projector's flat gradient), 40 launches with other kernels in between."""
    g = rnd(6293504 + 12, seed=3, scale=2.0)
    junk = torch.empty(32 * 1024 * 1024, device=DEV, dtype=torch.int16)
    seen = set()
    for it in range(40):
        if it % 3 == 0:
            junk.fill_(it)
        sq = torch.zeros(1, device=DEV)
        ops.grad_sqnorm(g, sq)
        seen.add(float(sq))
    assert len(seen) == 1, sorted(seen)
    v = seen.pop()
    assert abs(v - float((g.double() ** 2).sum())) < 1e-5 * v
    sq = torch.full((1,), 5.0, device=DEV); ops.grad_sqnorm(g, sq)                # accumulates
    assert abs(float(sq) - (v + 5.0)) < 1e-6 * v


def test_adamw_multi_matches_per_segment():
    """One launch over a flat buffer of segments with their own (lr, weight decay) == one ta_adamw_step per segment, bit for bit."""
    sizes = [1024, 12, 40000, 4, 5120 * 4, 8]
    ends = torch.tensor(sizes).cumsum(0)
    n = int(ends[-1])
    lrs, wds = [1e-3, 1e-3, 2e-4, 2e-4, 1e-3, 5e-5], [0.01, 0.0, 0.01, 0.0, 0.1, 0.0]
    p0, g = rnd(n, seed=1), rnd(n, seed=2, scale=3.0)
    pa, ma, va = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb, mb, vb = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sq, cnt = torch.zeros(1, device=DEV), torch.full((1,), 7.0, device=DEV)
    seg_end, seg_lr, seg_wd = ends.to(DEV), torch.tensor(lrs, device=DEV), torch.tensor(wds, device=DEV)
    for step in (1, 2, 3):
        gs = g * step
        sq.zero_(); ops.grad_sqnorm(gs, sq)
        o = 0
        for e, lr, wd in zip(ends.tolist(), lrs, wds):
            ops.adamw_step(pa[o:e], gs[o:e], ma[o:e], va[o:e], lr * 0.5, 0.9, 0.999, 1e-8, wd, step, sqnorm=sq, max_norm=1.0, denom=cnt)
            o = e
        ops.adamw_step_multi(pb, gs, mb, vb, seg_end, seg_lr, seg_wd, 0.5, 0.9, 0.999, 1e-8, step, sqnorm=sq, max_norm=1.0, denom=cnt)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)


def test_bernoulli_keep():
    k = ops.bernoulli_keep(200000, 0.9, 123, DEV)
    assert set(k.unique().tolist()) <= {0.0, 1.0} and abs(float(k.mean()) - 0.9) < 5e-3
    assert torch.equal(k, ops.bernoulli_keep(200000, 0.9, 123, DEV)) and not torch.equal(k, ops.bernoulli_keep(200000, 0.9, 124, DEV))


# ----------------------------------------------------------------------------- log-mel vs the oracle
def test_logmel_vs_oracle(golden):
    from oracle import features as OF
    from tests.golden import recipe as R
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    fe = LogMelFeatureExtractor(128, DEV)
    out = fe(R.logmel_waves(), sampling_rate=16000)
    g = golden("logmel.npz")
    wav, lens = OF.pad_batch(R.logmel_waves())
    of, om = OF.log_mel(wav, lens)
    f = out["input_features"].cpu().numpy()
    np.testing.assert_array_equal(out["attention_mask"].cpu().numpy(), om)
    # exact-f32 DFT (400-term FMA chain) vs float64 FFT: same tolerance class as the reference's own f32 chain
    assert np.abs(f - of).max() < 5e-4 and np.abs(f - of).mean() < 1e-5
    assert np.abs(f - g["feats"]).max() < 5e-4                       # and vs the reference's own output
    out = fe([R.OW.synthetic_wave(3, 16000 + 77)], sampling_rate=16000)
    np.testing.assert_array_equal(out["attention_mask"].cpu().numpy(), g["mask_odd"])
    assert np.abs(out["input_features"].cpu().numpy() - g["feats_odd"]).max() < 5e-4


# ----------------------------------------------------------------------------- trainable-projector primitives (nn_prims.hip)
def test_gelu_colsum():
    h = rnd(300, 512, seed=1, dtype=BF16)
    a = ops.gelu_fwd(h)
    assert relerr(a, torch.nn.functional.gelu(h.float())) < 1e-2
    da = rnd(300, 512, seed=2, dtype=BF16)
    hf = h.float().requires_grad_(True)
    torch.nn.functional.gelu(hf).backward(da.float())
    assert relerr(ops.gelu_bwd(da, h), hf.grad) < 1.5e-2
    x = rnd(5000, 300, seed=3)
    assert relerr(ops.colsum(x), x.sum(0)) < 1e-5
    assert relerr(ops.colsum(x.to(BF16)), x.to(BF16).float().sum(0)) < 1e-5


@pytest.mark.parametrize("H", [256, 1280])
def test_layernorm_res_fwd_bwd(H):
    M = 333
    z, res = rnd(M, H, seed=1), rnd(M, H, seed=2)
    keep = (torch.rand(M, H, generator=torch.Generator().manual_seed(3)) < 0.9).float().to(DEV) / 0.9
    gamma, beta = 1 + 0.1 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    for kp, rs in ((None, None), (keep, res)):
        zt = z.clone().requires_grad_(True); gt = gamma.clone().requires_grad_(True); bt = beta.clone().requires_grad_(True)
        u = zt * (kp if kp is not None else 1.0) + (rs if rs is not None else 0.0)
        ref = torch.nn.functional.layer_norm(u, (H,), gt, bt, 1e-12)
        yf, yb, xhat, rstd = ops.layernorm_res_fwd(z, gamma, beta, 1e-12, res=rs, keep=kp)
        assert relerr(yf, ref) < 1e-5 and relerr(yb, ref) < 1e-2
        dy = rnd(M, H, seed=6)
        ref.backward(dy)
        dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        du, dz = ops.layernorm_bwd(dy, xhat, rstd, gamma, dg, db, keep=kp)
        assert relerr(dz, zt.grad) < 1e-2                                   # bf16 output
        assert relerr(dg, gt.grad) < 1e-4 and relerr(db, bt.grad) < 1e-4
        if rs is not None:
            assert relerr(du * kp, zt.grad) < 1e-4


@pytest.mark.parametrize("heads,hd,Lq,Lk", [(16, 80, 3, 15), (16, 80, 3, 3), (4, 64, 3, 15)])
def test_attn_small_fwd_bwd(heads, hd, Lq, Lk):
    EB, H = 37, heads * hd
    q, k, v = rnd(EB * Lq, H, seed=1, dtype=BF16), rnd(EB * Lk, H, seed=2, dtype=BF16), rnd(EB * Lk, H, seed=3, dtype=BF16)
    keep = (torch.rand(EB, heads, Lq, Lk, generator=torch.Generator().manual_seed(4)) < 0.9).float().to(DEV) / 0.9
    scale = hd ** -0.5
    for kp in (None, keep):
        qt, kt, vt = (t.float().requires_grad_(True) for t in (q, k, v))
        sh = lambda t, L: t.reshape(EB, L, heads, hd).transpose(1, 2)
        pr = torch.softmax(sh(qt, Lq) @ sh(kt, Lk).transpose(-1, -2) * scale, -1)
        o_ref = ((pr * kp if kp is not None else pr) @ sh(vt, Lk)).transpose(1, 2).reshape(EB * Lq, H)
        O, P = ops.attn_small_fwd(q, k, v, EB, heads, Lq, Lk, scale, kp)
        assert relerr(P, pr) < 1e-4 and relerr(O, o_ref) < 1e-2
        do = rnd(EB * Lq, H, seed=5, dtype=BF16)
        o_ref.backward(do.float())
        dQ, dK, dV = ops.attn_small_bwd(do, q, k, v, P, EB, heads, Lq, Lk, scale, kp)
        assert relerr(dQ, qt.grad) < 1.5e-2 and relerr(dK, kt.grad) < 1.5e-2 and relerr(dV, vt.grad) < 1.5e-2


def test_relu_and_mix():
    h = rnd(200, 512, seed=1, dtype=BF16)
    assert torch.equal(ops.relu_fwd(h), torch.relu(h))
    da = rnd(200, 512, seed=2, dtype=BF16)
    assert torch.equal(ops.relu_bwd(da, h), torch.where(h.float() > 0, da, torch.zeros_like(da)))
    M, D, E = 333, 1024, 4
    lg, o, dout = rnd(M, E, seed=3), rnd(E, M, D, seed=4), rnd(M, D, seed=5)
    lt, ot = lg.clone().requires_grad_(True), o.clone().requires_grad_(True)
    p = torch.softmax(lt, -1)
    ref = (ot * p.t()[:, :, None]).sum(0)
    rw, out = ops.mix_fwd(lg, o)
    assert relerr(rw, p.detach()) < 1e-5 and relerr(out, ref.detach()) < 1e-5
    ref.backward(dout)
    dob, dlg = ops.mix_bwd(dout, o, rw)
    assert relerr(dob, ot.grad) < 1e-2 and relerr(dlg, lt.grad) < 1e-4


@pytest.mark.parametrize("variant", [None, "0", "3", "4", "5", "10", "12"])
def test_gemm_bf16_residual_in_place(variant, monkeypatch):
    """x += A W^T + b with a bf16 residual stream aliased to the output (the encoder's residual GEMMs)."""
    if variant is not None:
        _force_variant(monkeypatch, variant)
    M, N, K = 900, 1280, 256
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    bias, xr = rnd(N, seed=3), rnd(M, N, seed=4, dtype=BF16)
    ref = A.float() @ W.float().T + bias + xr.float()
    x = xr.clone()
    ops.gemm_nt(A, W, bias=bias, out=x, residual_bf16=x)
    assert relerr(x, ref) < 1.5e-2
    out = ops.gemm_nt(A, W, bias=bias, out_dtype=F32, residual_bf16=xr)         # f32 output, bf16 residual, not aliased
    assert relerr(out, ref) < 2e-3
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32), A.float() @ W.float().T) < 2e-3     # one-shot


def test_layernorm_bf16_input():
    M, H = 517, 1280
    x = rnd(M, H, seed=1, scale=2.0, dtype=BF16)
    w, b = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    keep = (torch.rand(M, generator=torch.Generator().manual_seed(4)) < 0.8).float().to(DEV)
    ref = torch.nn.functional.layer_norm(x.float(), (H,), w, b, 1e-5)
    yb, yf = ops.layernorm(x, w, b, out_f32=True)
    assert relerr(yf, ref) < 1e-5 and relerr(yb, ref) < 1e-2
    yb2, _ = ops.layernorm(x, w, b, rowscale=keep)
    assert relerr(yb2, ref * keep[:, None]) < 1e-2


def test_rmsnorm_bf16_stream():
    """RMSNorm forward / backward with the input stream in bf16 == the f32 kernels on the same (bf16-rounded) values."""
    M, H = 333, 1024
    xb = rnd(M, H, seed=1, scale=1.5, dtype=BF16)
    w = 1 + 0.1 * rnd(H, seed=2)
    yb0, yf0, r0 = ops.rmsnorm_fwd(xb.float(), w, out_f32=True)
    yb1, yf1, r1 = ops.rmsnorm_fwd(xb, w, out_f32=True)
    assert torch.equal(yf0, yf1) and torch.equal(r0, r1) and torch.equal(yb0, yb1)
    dy, dres = rnd(M, H, seed=3), rnd(M, H, seed=4)
    dx0, dxb0, _ = ops.rmsnorm_bwd(dy, xb.float(), r0, w, dres=dres)
    dx1, dxb1, _ = ops.rmsnorm_bwd(dy, xb, r1, w, dres=dres)
    assert relerr(dx1, dx0) < 1e-6 and relerr(dxb1, dxb0) < 1e-2          # (FMA contraction may differ between the two instantiations)


# ----------------------------------------------------------------------------- fused encoder q|k|v path
def il_perm():
    """column p of a head <- head dim (the interleaved rotary layout of ta_gemm_opts.rope_tab)."""
    p = torch.arange(64)
    return torch.where(p < 32, (p >> 1) + 16 * (p & 1), p)


@pytest.mark.parametrize("variant", [None, "0", "3", "4", "5", "10", "12"])
def test_gemm_rope_epilogue(variant, monkeypatch):
    """act = 2: q|k = rope(A W^T + b) with W's rows in the interleaved pair order == HF rotate-half rope on the plain
    projection, column-permuted (TF:models/glmasr/modeling_glmasr.py:153-168)."""
    if variant is not None:
        _force_variant(monkeypatch, variant)
    B, S, nh, K = 3, 100, 5, 256
    M, N = B * S, 2 * nh * 64
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    bias = 0.1 * rnd(N, seed=3)
    cos, sin = rope_tables(128, 32, 10000.0)                                  # [128, 16]
    tab = torch.stack([cos, sin], -1).contiguous()
    rows = (torch.arange(2 * nh)[:, None] * 64 + il_perm()[None, :]).reshape(-1).to(DEV)
    out = ops.gemm_nt(A, W[rows].contiguous(), bias=bias[rows].contiguous(), act=2, rope=(tab, S))
    y = (A.float() @ W.float().T + bias).reshape(B, S, 2 * nh, 64)
    c = torch.cat([cos[:S], cos[:S]], -1)[None, :, None]; s = torch.cat([sin[:S], sin[:S]], -1)[None, :, None]
    ref = torch.cat([y[..., :32] * c + rot_half(y[..., :32]) * s, y[..., 32:]], -1)
    ref = ref[..., il_perm().to(DEV)].reshape(M, N)
    assert relerr(out, ref) < 8e-3
    assert relerr(ops.gemm_nt(A, W, out_dtype=F32), A.float() @ W.float().T) < 2e-3       # next call: plain again


@pytest.mark.parametrize("S", [104, 100, 99])        # V^T clip offsets 16-B, 8-B and 2-B aligned
def test_attention_fwd_strided_layout(S):
    """ta_attention_fwd_ex over the encoder's fused layout (token-major q|k, V^T as [H*64, B*S]) == the head-major call."""
    B, nh, hd = 3, 5, 64
    M, H = B * S, nh * hd
    qk = rnd(M, 2 * H, seed=1).to(BF16)
    v = rnd(M, H, seed=2).to(BF16)
    vt = torch.zeros(H * M + 64, device=DEV, dtype=BF16)
    vt[:H * M] = v.T.contiguous().reshape(-1)
    lay = (S * 2 * H, 64, 2 * H, S * 2 * H, 64, 2 * H, S, 64 * M, M)
    O = ops.attention_fwd_strided(qk, qk[:, H:], vt, B, nh, nh, S, hd, False, 0.125, lay)
    q = qk[:, :H].reshape(B, S, nh, hd).transpose(1, 2).contiguous()
    k = qk[:, H:].reshape(B, S, nh, hd).transpose(1, 2).contiguous()
    vh = v.reshape(B, S, nh, hd).transpose(1, 2).contiguous()
    ref, _ = ops.attention_fwd(q, k, to_T(vh, ops.pad64(S)), S, False, 0.125, None, want_lse=False)
    assert relerr(O, ref) < 1e-6, relerr(O, ref)
    ref32, _ = ref_attention(q.float(), k.float(), vh.float(), False, 0.125, None)
    assert relerr(O, ref32.transpose(1, 2).reshape(M, H)) < 2e-2


@pytest.mark.parametrize("B,nh,S", [(3, 5, 500), (2, 3, 77), (1, 2, 64), (2, 2, 129), (1, 20, 1500), (4, 1, 7)])
def test_attention_enc_fwd(B, nh, S):
    """ta_attention_enc_fwd (round 3: DMA-staged K / V row tiles, V read transposed, base-2 softmax on pre-scaled scores, running
    maximum as the MFMA C operand) == softmax(ln 2 * q k^T) v in fp32; ragged last key tile, ragged last query tile, one tile,
    30 s clips, a sequence shorter than one fragment."""
    H = nh * 64
    qkv = torch.cat([rnd(B * S, H, seed=1, scale=1.5), rnd(B * S, H, seed=2), rnd(B * S, H, seed=3)], 1).to(BF16).contiguous()
    out = ops.attention_enc_fwd(qkv, B, nh, S)
    q, k, v = (qkv[:, i * H:(i + 1) * H].float().reshape(B, S, nh, 64).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * math.log(2.0), -1)
    ref = (p @ v).transpose(1, 2).reshape(B * S, H)
    assert relerr(out, ref) < 2e-2, relerr(out, ref)
    assert cos_sim(out, ref) > 0.9999


def test_attention_enc_fwd_moving_maximum_and_determinism():
    """The rescale branch (a later key tile raises a row's maximum: scores grow with the key index, and one spiked key in the
    LAST tile) and bitwise run-to-run reproducibility."""
    B, nh, S = 2, 2, 500
    H = nh * 64
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * S, H, generator=g)
    k = torch.randn(B * S, H, generator=g) * (0.2 + torch.arange(B * S)[:, None] % S / S * 1.5)      # later keys score higher
    k[S - 3] *= 6.0                                                                                  # a spike in the ragged last tile
    v = torch.randn(B * S, H, generator=g)
    qkv = torch.cat([q, k, v], 1).to(DEV).to(BF16).contiguous()
    out = ops.attention_enc_fwd(qkv, B, nh, S).clone()
    qf, kf, vf = (qkv[:, i * H:(i + 1) * H].float().reshape(B, S, nh, 64).transpose(1, 2) for i in range(3))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * math.log(2.0), -1) @ vf).transpose(1, 2).reshape(B * S, H)
    assert relerr(out, ref) < 2e-2, relerr(out, ref)
    for _ in range(5):
        assert torch.equal(ops.attention_enc_fwd(qkv, B, nh, S), out)


def test_gemm_rope_epilogue_column_limit():
    """ta_gemm_opts.rope_cols: the q | k | v GEMM of the encoder rotates the first 2H columns only."""
    B, S, nh, K = 2, 100, 5, 256
    M, H = B * S, nh * 64
    N = 3 * H
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    bias = 0.1 * rnd(N, seed=3)
    cos, sin = rope_tables(128, 32, 10000.0)
    tab = torch.stack([cos, sin], -1).contiguous()
    rows = (torch.arange(2 * nh)[:, None] * 64 + il_perm()[None, :]).reshape(-1).to(DEV)
    rows = torch.cat([rows, 2 * H + torch.arange(H, device=DEV)])
    out = ops.gemm_nt(A, W[rows].contiguous(), bias=bias[rows].contiguous(), act=2, rope=(tab, S, 2 * H))
    y = (A.float() @ W.float().T + bias)
    yqk = y[:, :2 * H].reshape(B, S, 2 * nh, 64)
    c = torch.cat([cos[:S], cos[:S]], -1)[None, :, None]; s = torch.cat([sin[:S], sin[:S]], -1)[None, :, None]
    rq = torch.cat([yqk[..., :32] * c + rot_half(yqk[..., :32]) * s, yqk[..., 32:]], -1)[..., il_perm().to(DEV)].reshape(M, 2 * H)
    assert relerr(out[:, :2 * H], rq) < 8e-3
    assert relerr(out[:, 2 * H:], y[:, 2 * H:]) < 8e-3              # the v columns: bias only, no rotation


# ----------------------------------------------------------------------------- trainable-LM helpers
@pytest.mark.parametrize("dyb,xb", [(False, False), (True, True), (False, True)])
def test_rmsnorm_dw(dyb, xb):
    M, H = 333, 1024
    dy, x = rnd(M, H, seed=1), rnd(M, H, seed=2, scale=2.0)
    dy, x = (dy.to(BF16) if dyb else dy), (x.to(BF16) if xb else x)
    r = torch.rsqrt((x.float() ** 2).mean(-1) + 1e-6)
    dw = torch.full((H,), 0.5, device=DEV)
    ops.rmsnorm_dw(dy, x, r, dw)
    ref = 0.5 + (dy.float() * x.float() * r[:, None]).sum(0)
    assert relerr(dw, ref) < 1e-4


def test_embed_grad_scatter():
    V, D, n = 50, 64, 40
    ids = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(0)).to(DEV)
    src = torch.full((n,), -1, dtype=torch.int32, device=DEV); src[5:12] = torch.arange(7, dtype=torch.int32, device=DEV)
    dx = rnd(n, D, seed=3)
    de = torch.zeros(V, D, device=DEV)
    ops.embed_grad_scatter(ids, src, dx, de)
    ref = torch.zeros(V, D, device=DEV)
    keep = src < 0
    ref.index_add_(0, ids[keep], dx[keep])
    assert relerr(de, ref) < 1e-5


def test_attention_fwd_is_deterministic():
    """Bitwise run-to-run reproducibility of the encoder attention at its real length (8 key tiles, 7 of them through the
    unmasked tile body).  Guards the MFMA -> VALU hazard an inline-asm row maximum once slipped past the compiler."""
    B, nh, hd, S = 4, 5, 64, 500
    q, k, v = (rnd(B, nh, S, hd, seed=s).to(BF16) for s in (1, 2, 3))
    vT = to_T(v, ops.pad64(S))
    ref, _ = ops.attention_fwd(q, k, vT, S, False, 0.125, None, want_lse=False)
    ref = ref.clone()
    for _ in range(10):
        out, _ = ops.attention_fwd(q, k, vT, S, False, 0.125, None, want_lse=False)
        assert torch.equal(out, ref)
    ql, kl, vl = (rnd(2, h, 192, 128, seed=s).to(BF16) for h, s in ((4, 4), (2, 5), (2, 6)))       # LM shapes: GQA kernel
    vlT = to_T(vl, 192)
    r2, _ = ops.attention_fwd(ql, kl, vlT, 192, True, 128 ** -0.5, None)
    r2 = r2.clone()
    for _ in range(10):
        o2, _ = ops.attention_fwd(ql, kl, vlT, 192, True, 128 ** -0.5, None)
        assert torch.equal(o2, r2)


@pytest.mark.parametrize("variant", [None, "0", "3", "4", "5", "10", "12"])
def test_gemm_w_blocked(variant, monkeypatch):
    """W handed over as [N/64][K/64][64][64] blocks (8 KB contiguous per K tile of 64 rows) == the row-major call."""
    if variant is not None:
        _force_variant(monkeypatch, variant)
    M, N, K = 700, 1280, 384
    A, W = rnd(M, K, seed=1, dtype=BF16), rnd(N, K, seed=2, scale=1 / math.sqrt(K), dtype=BF16)
    bias = rnd(N, seed=3)
    Wb = W.view(N // 64, 64, K // 64, 64).permute(0, 2, 1, 3).contiguous()
    ref = ops.gemm_nt(A, W, bias=bias, act=1)
    out = ops.gemm_nt(A, Wb, M, N, K, bias=bias, act=1, w_blocked=True)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("M,Ny,Nx", [(6144, 1024, 2048), (700, 136, 264), (95, 128, 256), (6144, 4096, 1024)])
def test_gemm_tn(M, Ny, Nx):
    """out (+)= Y^T X over row-major bf16 operands (the weight-gradient product): full tiles, ragged rows / columns,
    accumulation into an existing gradient."""
    Y, X = rnd(M, Ny, seed=1, dtype=BF16), rnd(M, Nx, seed=2, dtype=BF16)
    ref = Y.float().T @ X.float()
    out = ops.gemm_tn(Y, X)
    assert relerr(out, ref) < 2e-3, relerr(out, ref)
    base = rnd(Ny, Nx, seed=3)
    acc = base.clone()
    ops.gemm_tn(Y, X, out=acc, accumulate=True)
    assert relerr(acc, base + ref) < 2e-3

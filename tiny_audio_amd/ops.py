"""Thin torch-tensor wrappers over the primitive kernels of libta355.so.

PyTorch is plumbing here (device memory, streams); all arithmetic happens in the HIP library.
Every wrapper launches on ``torch.cuda.current_stream()`` and raises ``Ta355Error`` on failure.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, lib

BF16 = torch.bfloat16
F32 = torch.float32


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    if _lib.DRY_RUN:          # test instrumentation only (see _lib.DRY_RUN)
        return None
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, dtype=None):
    assert (t.is_cuda or _lib.DRY_RUN) and t.is_contiguous(), "ta355 ops need contiguous CUDA(HIP) tensors"
    if dtype is not None:
        assert t.dtype == dtype, (t.dtype, dtype)
    return t


# The library reads its environment knobs once (csrc/gemm.hip GemmKnobs::load, the decode switch of generate.hip); tests and A/B
# scripts switch them between launches, so the wrapper calls ta_gemm_reload_knobs() whenever one has changed since the previous call.
# These four are all the library has (plus TA355_ENC_QKV_FUSED, read per call).
_KNOB_KEYS = ("TA355_GEMM_VARIANT", "TA355_GELU_LUT", "TA355_DECODE_FUSED", "TA355_SCORES_SPLIT")
_knob_state = None


def sync_gemm_knobs():
    global _knob_state
    import os
    cur = tuple(os.environ.get(k) for k in _KNOB_KEYS)
    if cur != _knob_state:
        if _knob_state is not None or any(v is not None for v in cur):
            lib().ta_gemm_reload_knobs()
        _knob_state = cur


def gemm_nt(A, W, M=None, N=None, K=None, *, out=None, out_dtype=BF16, bias=None, residual=None, act=0,
            a_map=None, c_map=None, splits=1, k_ext=None, residual_bf16=None, rope=None, w_blocked=False):
    """C[M,N] = epilogue(A[M,K] @ W[N,K]^T).  a_map=(ld, rpb, batch_stride); c_map=(ld, rpb, batch_stride, offset);
    k_ext=(A2 [M,K2], W2 [N,K2]) adds A2 @ W2^T inside the same launch (the LoRA rank-space tile);
    rope=(table f32 [rows,16,2], rows) with act=2: interleaved partial rotary embedding in the epilogue (ta355.h)."""
    _req(A, BF16); _req(W, BF16)
    sync_gemm_knobs()
    opts = None
    if residual_bf16 is not None or k_ext is not None or rope is not None or w_blocked:
        from ._lib import GemmOpts
        opts = GemmOpts()
        opts.w_blocked = int(bool(w_blocked))      # W given as [N/64][K/64][64][64] blocks (pass N and K explicitly)
        if rope is not None:
            _req(rope[0], F32)
            opts.rope_tab, opts.rope_rows = ptr(rope[0]), int(rope[1])
            opts.rope_cols = int(rope[2]) if len(rope) > 2 else 0       # rope on columns [0, rope_cols) only (0 = all)
        if residual_bf16 is not None:       # bf16 residual with C's row map (may alias `out`)
            _req(residual_bf16, BF16)
            opts.residual_bf16 = ptr(residual_bf16)
        if k_ext is not None:
            A2, W2 = k_ext
            _req(A2, BF16); _req(W2, BF16)
            opts.a2, opts.w2, opts.k2, opts.lda2 = ptr(A2), ptr(W2), W2.shape[1], A2.shape[1]
    N = N or W.shape[0]
    K = K or W.shape[1]
    M = M or A.numel() // K
    lda, a_rpb, a_bs = a_map or (K, 0, 0)
    ldc, c_rpb, c_bs, c_off = c_map or (N, 0, 0, 0)
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=out_dtype)
    ws = None
    if splits > 1:
        ws = torch.empty(lib().ta_gemm_splitk_ws_bytes(M, N, splits) // 4, device=A.device, dtype=F32)
    import ctypes as _C
    check(lib().ta_gemm_bf16_nt_opt(ptr(A), ptr(W), ptr(out), M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off,
                                    ptr(bias), ptr(residual), act, 1 if out.dtype == BF16 else 0, splits, ptr(ws),
                                    None, None, None, None if opts is None else _C.addressof(opts), stream()), "ta_gemm_bf16_nt_opt")
    return out


def gemm_tn(Y, X, out=None, accumulate=False):
    """out f32 [Ny, Nx] (+)= Y[M, Ny]^T @ X[M, Nx]  (bf16 operands; the weight-gradient product dW = dY^T X)."""
    _req(Y, BF16); _req(X, BF16)
    M, Ny = Y.shape
    Nx = X.shape[1]
    if out is None:
        out = torch.zeros((Ny, Nx), device=Y.device, dtype=F32)
        accumulate = False
    ws = torch.empty(max(lib().ta_gemm_bf16_tn_ws_bytes(M, Ny, Nx), 16), device=Y.device, dtype=torch.uint8)
    check(lib().ta_gemm_bf16_tn(ptr(Y), ptr(X), ptr(out), M, Ny, Nx, int(bool(accumulate)), ptr(ws), ws.numel(), stream()),
          "ta_gemm_bf16_tn")
    return out


def gemm_nt_grouped(A, W, out, M, N, K, *, seg=None, krange=None, n_groups=1, bias=None, act=0, a_idx=None, w_stride=0, c_stride=0):
    """ta_gemm_bf16_nt_grouped: every group (MoE expert) in ONE launch.  rows form: ``seg`` int32 [2 * n] {row base, count},
    W [n, N, K] (w_stride = N * K), bias [n, N]; K-slice form: ``krange`` int32 [2 * n] 64-wide K-tile ranges, out f32
    [n, M, N] (c_stride = M * N)."""
    _req(A, BF16); _req(W, BF16)
    sync_gemm_knobs()
    check(lib().ta_gemm_bf16_nt_grouped(ptr(A), ptr(W), ptr(out), M, N, K, ptr(bias), act, int(out.dtype == BF16), ptr(a_idx),
                                        ptr(seg), ptr(krange), n_groups, w_stride, c_stride, stream()), "ta_gemm_bf16_nt_grouped")
    return out


def layernorm(x, w, b, eps=1e-5, rowscale=None, out_bf16=True, out_f32=False):
    if x.dtype == BF16:
        M, H = x.shape
        yb = torch.empty((M, H), device=x.device, dtype=BF16) if out_bf16 else None
        yf = torch.empty((M, H), device=x.device, dtype=F32) if out_f32 else None
        check(lib().ta_layernorm_bf16(ptr(x), ptr(w), ptr(b), ptr(yb), ptr(yf), ptr(rowscale), M, H, eps, stream()),
              "ta_layernorm_bf16")
        return yb, yf
    _req(x, F32)
    M, H = x.shape
    yb = torch.empty((M, H), device=x.device, dtype=BF16) if out_bf16 else None
    yf = torch.empty((M, H), device=x.device, dtype=F32) if out_f32 else None
    check(lib().ta_layernorm_f32(ptr(x), ptr(w), ptr(b), ptr(yb), ptr(yf), ptr(rowscale), M, H, eps, stream()),
          "ta_layernorm_f32")
    return yb, yf


def rmsnorm_fwd(x, w, eps=1e-6, act_gelu=False, out_bf16=True, out_f32=False):
    M, H = x.shape
    yb = torch.empty((M, H), device=x.device, dtype=BF16) if out_bf16 else None
    yf = torch.empty((M, H), device=x.device, dtype=F32) if out_f32 else None
    r = torch.empty(M, device=x.device, dtype=F32)
    if x.dtype == BF16:                  # residual stream kept in the model dtype
        assert not act_gelu
        check(lib().ta_rmsnorm_fwd_bf16(ptr(x), ptr(w), ptr(yb), ptr(yf), ptr(r), M, H, eps, stream()), "ta_rmsnorm_fwd_bf16")
        return yb, yf, r
    _req(x, F32)
    check(lib().ta_rmsnorm_fwd(ptr(x), ptr(w), ptr(yb), ptr(yf), ptr(r), M, H, eps, int(act_gelu), stream()),
          "ta_rmsnorm_fwd")
    return yb, yf, r


def rmsnorm_bwd(dy, x, rstd, w, dres=None, act_gelu=False, want_dw=False, out_bf16=True):
    if x.dtype != BF16:
        _req(dy, F32)
    M, H = x.shape
    dx = torch.empty((M, H), device=x.device, dtype=F32)
    dxb = torch.empty((M, H), device=x.device, dtype=BF16) if out_bf16 else None
    if x.dtype == BF16:
        assert not act_gelu and not want_dw
        check(lib().ta_rmsnorm_bwd_bf16(ptr(dy), int(dy.dtype == BF16), ptr(x), ptr(rstd), ptr(w), ptr(dres), ptr(dx), ptr(dxb), M, H, stream()),
              "ta_rmsnorm_bwd_bf16")
        return dx, dxb, None
    _req(x, F32)
    dw = torch.zeros(H, device=x.device, dtype=F32) if want_dw else None
    check(lib().ta_rmsnorm_bwd(ptr(dy), ptr(x), ptr(rstd), ptr(w), ptr(dres), ptr(dx), ptr(dxb), ptr(dw), M, H,
                               int(act_gelu), stream()), "ta_rmsnorm_bwd")
    return dx, dxb, dw


def pad64(n):
    return (n + 63) // 64 * 64


def _out(out, shape, device, dtype=BF16):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype
    return _req(out)


def attention_fwd(Q, K, VT, L, causal, scale, kmask=None, want_lse=True, out=None):
    """Q [B,Hq,L,hd], K [B,Hkv,L,hd], VT [B,Hkv,hd,Lp] bf16 -> O [B*L, Hq*hd] bf16, LSE [B,Hq,L].  ``out``: the tensor to write O
    into (here and in the wrappers below: a caller that wants to see which rows a kernel wrote passes its own, pre-filled)."""
    B, Hq, _, hd = Q.shape
    Hkv, Lp = K.shape[1], VT.shape[3]
    O = _out(out, (B * L, Hq * hd), Q.device)
    lse = torch.empty((B, Hq, L), device=Q.device, dtype=F32) if want_lse else None
    check(lib().ta_attention_fwd(ptr(Q), ptr(K), ptr(VT), ptr(O), ptr(lse), ptr(kmask), B, Hq, Hkv, L, Lp, hd,
                                 int(causal), scale, stream()), "ta_attention_fwd")
    return O, lse


def attention_fwd_strided(Q, K, VT, B, Hq, Hkv, L, hd, causal, scale, layout, kmask=None):
    """ta_attention_fwd_ex: operands described by element strides (q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs)."""
    import ctypes as _C
    from ._lib import AttnLayout
    lay = AttnLayout(*[int(v) for v in layout])
    O = torch.empty((B * L, Hq * hd), device=Q.device, dtype=BF16)
    check(lib().ta_attention_fwd_ex(ptr(Q), ptr(K), ptr(VT), ptr(O), None, ptr(kmask), B, Hq, Hkv, L, pad64(L), hd,
                                    int(causal), scale, _C.addressof(lay), stream()), "ta_attention_fwd_ex")
    return O


def _out3(out, Q, K, V):
    if out is None:
        return torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    return tuple(_out(o, t.shape, t.device) for o, t in zip(out, (Q, K, V)))


def attention_bwd(Q, QT, K, KT, V, dO, dOT, lse, delta, L, causal, scale, kmask=None, out=None):
    """QT / KT / dOT: the transposed images the library no longer reads (None is fine).  ``out``: (dQ, dK, dV) to write into."""
    B, Hq, _, hd = Q.shape
    Hkv, Lp = K.shape[1], (pad64(L) if KT is None else KT.shape[3])
    dQ, dK, dV = _out3(out, Q, K, V)
    check(lib().ta_attention_bwd(ptr(Q), ptr(QT), ptr(K), ptr(KT), ptr(V), ptr(dO), dO.shape[-1], ptr(dOT), ptr(lse),
                                 ptr(delta), ptr(kmask), ptr(dQ), ptr(dK), ptr(dV), B, Hq, Hkv, L, Lp, hd, int(causal),
                                 scale, stream()), "ta_attention_bwd")
    return dQ, dK, dV


def attention_enc_fwd(qkv, B, heads, S):
    """GLM-ASR encoder attention straight from the q|k|v GEMM output: qkv bf16 [B*S, 3*heads*64] (q pre-scaled by
    head_dim^-0.5 * log2 e) -> bf16 [B*S, heads*64] = softmax_base2(q k^T) v, non-causal, no mask."""
    _req(qkv, BF16)
    assert qkv.shape == (B * S, 3 * heads * 64)
    out = torch.empty((B * S, heads * 64), device=qkv.device, dtype=BF16)
    check(lib().ta_attention_enc_fwd(ptr(qkv), ptr(out), B, heads, S, stream()), "ta_attention_enc_fwd")
    return out


def attention_enc_fwd_varlen(qkv, cu_rows, heads, max_rows, out=None):
    """The same over clips of different lengths (ta_attention_enc_fwd_varlen): clip b owns rows ``cu_rows[b] .. cu_rows[b + 1]``
    of qkv bf16 [rows, 3*heads*64]; ``cu_rows`` int32 [B + 1] on the device, ``max_rows`` the longest clip.  ``out``: a bf16
    [rows, heads*64] tensor to write into."""
    _req(qkv, BF16)
    assert qkv.dim() == 2 and qkv.shape[1] == 3 * heads * 64
    assert cu_rows.dtype == torch.int32 and cu_rows.is_contiguous() and cu_rows.device == qkv.device
    if out is None:
        out = torch.empty((qkv.shape[0], heads * 64), device=qkv.device, dtype=BF16)
    check(lib().ta_attention_enc_fwd_varlen(ptr(qkv), ptr(out), ptr(cu_rows), cu_rows.numel() - 1, heads, int(max_rows), stream()),
          "ta_attention_enc_fwd_varlen")
    return out


def attention_fwd_seg(Q, K, VT, L, scale, kmask=None, seg=None, want_lse=True, out=None):
    """ta_attention_fwd_seg: the causal head_dim-128 forward over packed rows (``seg``: the table of ``segment_table``; None = the
    plain causal ``attention_fwd``).  Shapes as ``attention_fwd``."""
    B, Hq, _, hd = Q.shape
    Hkv, Lp = K.shape[1], VT.shape[3]
    assert hd == 128
    O = _out(out, (B * L, Hq * hd), Q.device)
    lse = torch.empty((B, Hq, L), device=Q.device, dtype=F32) if want_lse else None
    check(lib().ta_attention_fwd_seg(ptr(Q), ptr(K), ptr(VT), ptr(O), ptr(lse), ptr(kmask), ptr(seg), B, Hq, Hkv, L, Lp, scale,
                                     stream()), "ta_attention_fwd_seg")
    return O, lse


def attention_extend(Q, Kn, Vn, Kc, Vc, pmask, clip_of, lens, scale, want_lse=True, out=None):
    """ta_attention_extend: R rows of T given positions behind the prompt cache of their clips.  Q [R,Hq,T,128], Kn / Vn [R,Hkv,T,128]
    bf16 (the row's own keys, ``lens`` int32 [R] of them valid), Kc / Vc [B,Hkv,Lmax,128] bf16 = one layer of the prompt cache, read in
    place through ``clip_of`` int32 [R]; pmask int32 [B, Lp], Lp <= Lmax -> O [R*T, Hq*128] bf16 (exact 0 at t >= lens[r]), LSE
    [R,Hq,T] or None.  ``out``: the tensor to write O into."""
    R, Hq, T, hd = Q.shape
    B, Hkv, Lmax, _ = Kc.shape
    assert hd == 128 and Kn.shape == (R, Hkv, T, hd) and Vn.shape == Kn.shape and Vc.shape == Kc.shape
    assert pmask.dtype == torch.int32 and pmask.dim() == 2 and pmask.shape[0] == B
    assert clip_of.dtype == torch.int32 and clip_of.numel() == R and lens.dtype == torch.int32 and lens.numel() == R
    for t in (Q, Kn, Vn, Kc, Vc, pmask, clip_of, lens):
        _req(t)
    O = _out(out, (R * T, Hq * hd), Q.device)
    lse = torch.empty((R, Hq, T), device=Q.device, dtype=F32) if want_lse else None
    check(lib().ta_attention_extend(ptr(Q), ptr(Kn), ptr(Vn), ptr(Kc), ptr(Vc), ptr(pmask), ptr(clip_of), ptr(lens), ptr(O), ptr(lse),
                                    B, R, Hq, Hkv, T, pmask.shape[1], Lmax, scale, stream()), "ta_attention_extend")
    return O, lse


def attention_bwd_seg(Q, K, V, dO, lse, delta, L, scale, kmask=None, seg=None, out=None):
    """ta_attention_bwd_seg: the causal head_dim-128 backward over packed rows (``seg`` None = the plain causal call).
    ``out``: (dQ, dK, dV) to write into."""
    B, Hq, _, hd = Q.shape
    Hkv, Lp = K.shape[1], pad64(L)
    dQ, dK, dV = _out3(out, Q, K, V)
    check(lib().ta_attention_bwd_seg(ptr(Q), ptr(K), ptr(V), ptr(dO), dO.shape[-1], ptr(lse), ptr(delta), ptr(kmask), ptr(seg), ptr(dQ),
                                     ptr(dK), ptr(dV), B, Hq, Hkv, L, Lp, scale, stream()), "ta_attention_bwd_seg")
    return dQ, dK, dV


def attention_fwd_qkv(qkv0, qn_w, kn_w, cosT, sinT, B, Hq, Hkv, L, scale, eps=1e-6, kmask=None, pos=None, seg=None, out=None):
    """ta_lm_qkv_post_fwd + ta_attention_fwd in one launch (short causal sequences): returns O, LSE, Q, K, V, rq, rk.
    qn_w / kn_w None: no q/k-norm (rq / rk are not written); cosT / sinT None: a NoPE layer; ``seg``: packed rows (the table of
    ``segment_table``), dispatching to ta_attention_fwd_qkv_seg."""
    hd, dev = 128, qkv0.device
    mk = lambda h: torch.empty((B, h, L, hd), device=dev, dtype=BF16)
    Q, K, V = mk(Hq), mk(Hkv), mk(Hkv)
    rq = torch.empty((B * L, Hq), device=dev, dtype=F32); rk = torch.empty((B * L, Hkv), device=dev, dtype=F32)
    O = _out(out, (B * L, Hq * hd), dev)
    lse = torch.empty((B, Hq, L), device=dev, dtype=F32)
    if seg is None:
        check(lib().ta_attention_fwd_qkv(ptr(qkv0), ptr(qn_w), ptr(kn_w), ptr(cosT), ptr(sinT), ptr(pos), ptr(Q), ptr(K), ptr(V), ptr(rq),
                                         ptr(rk), ptr(O), ptr(lse), ptr(kmask), B, Hq, Hkv, L, scale, eps, stream()), "ta_attention_fwd_qkv")
    else:
        check(lib().ta_attention_fwd_qkv_seg(ptr(qkv0), ptr(qn_w), ptr(kn_w), ptr(cosT), ptr(sinT), ptr(pos), ptr(Q), ptr(K), ptr(V), ptr(rq),
                                             ptr(rk), ptr(O), ptr(lse), ptr(kmask), ptr(seg), B, Hq, Hkv, L, scale, eps, stream()),
              "ta_attention_fwd_qkv_seg")
    return O, lse, Q, K, V, rq, rk


def attention_bwd_qkv(Q, K, V, dO, lse, delta, qkv0, rq, rk, qn_w, kn_w, cosT, sinT, L, scale, kmask=None, pos=None, seg=None, out=None):
    """Causal GQA attention backward with the q|k|v post-processing backward in its epilogue: returns d(qkv0) token-major.
    V None: the V rows are read in place from qkv0.  qn_w / kn_w / cosT / sinT None as in ``attention_fwd_qkv``; ``seg``: packed rows,
    dispatching to ta_attention_bwd_qkv_seg."""
    B, Hq, _, hd = Q.shape
    Hkv, Lp = K.shape[1], pad64(L)
    dqkv = _out(out, qkv0.shape, qkv0.device)
    if seg is None:
        check(lib().ta_attention_bwd_qkv(ptr(Q), ptr(K), ptr(V), ptr(dO), dO.shape[-1], ptr(lse), ptr(delta), ptr(kmask), ptr(qkv0),
                                         ptr(rq), ptr(rk), ptr(qn_w), ptr(kn_w), ptr(cosT), ptr(sinT), ptr(pos), ptr(dqkv), B, Hq, Hkv,
                                         L, Lp, hd, 1, scale, stream()), "ta_attention_bwd_qkv")
    else:
        check(lib().ta_attention_bwd_qkv_seg(ptr(Q), ptr(K), ptr(V), ptr(dO), dO.shape[-1], ptr(lse), ptr(delta), ptr(kmask), ptr(seg),
                                             ptr(qkv0), ptr(rq), ptr(rk), ptr(qn_w), ptr(kn_w), ptr(cosT), ptr(sinT), ptr(pos), ptr(dqkv),
                                             B, Hq, Hkv, L, Lp, scale, stream()), "ta_attention_bwd_qkv_seg")
    return dqkv


def lm_qkv_post_fwd(qkv0, qn_w, kn_w, cosT, sinT, B, Hq, Hkv, L, eps=1e-6, pos=None):
    hd, Lp, dev = 128, pad64(L), qkv0.device
    mk = lambda h: torch.empty((B, h, L, hd), device=dev, dtype=BF16)
    mkT = lambda h: torch.empty((B, h, hd, Lp), device=dev, dtype=BF16)
    Q, K, V, QT, KT, VT = mk(Hq), mk(Hkv), mk(Hkv), mkT(Hq), mkT(Hkv), mkT(Hkv)
    rq = torch.empty((B * L, Hq), device=dev, dtype=F32); rk = torch.empty((B * L, Hkv), device=dev, dtype=F32)
    check(lib().ta_lm_qkv_post_fwd(ptr(qkv0), ptr(qn_w), ptr(kn_w), ptr(cosT), ptr(sinT), ptr(pos), ptr(Q), ptr(K),
                                   ptr(V), ptr(QT), ptr(KT), ptr(VT), ptr(rq), ptr(rk), B, Hq, Hkv, L, Lp, eps,
                                   stream()), "ta_lm_qkv_post_fwd")
    return Q, K, V, QT, KT, VT, rq, rk


def lm_qkv_post_bwd(dQ, dK, dV, qkv0, rq, rk, qn_w, kn_w, cosT, sinT, B, Hq, Hkv, L, pos=None, dqn=None, dkn=None, out=None):
    """dqn / dkn f32 [128]: += the q_norm / k_norm weight gradients (trainable LM)."""
    dqkv = _out(out, qkv0.shape, qkv0.device)
    check(lib().ta_lm_qkv_post_bwd(ptr(dQ), ptr(dK), ptr(dV), ptr(qkv0), ptr(rq), ptr(rk), ptr(qn_w), ptr(kn_w),
                                   ptr(cosT), ptr(sinT), ptr(pos), ptr(dqkv), ptr(dqn), ptr(dkn), B, Hq, Hkv, L, stream()),
          "ta_lm_qkv_post_bwd")
    return dqkv


def rmsnorm_dw(dy, x, rstd, dw):
    """dw[h] += sum_m dy[m,h] * x[m,h] * rstd[m]   (dy, x: f32 or bf16 [M, H])"""
    M, H = x.shape
    check(lib().ta_rmsnorm_dw(ptr(dy), int(dy.dtype == BF16), ptr(x), int(x.dtype == BF16), ptr(rstd), ptr(dw), M, H, stream()),
          "ta_rmsnorm_dw")
    return dw


def embed_grad_scatter(ids, src_row, dx0, dembed):
    n, D = dx0.shape
    check(lib().ta_embed_grad_scatter(ptr(ids), ptr(src_row), ptr(dx0), ptr(dembed), n, D, dembed.shape[0], stream()),
          "ta_embed_grad_scatter")
    return dembed


def enc_qkv_post(qkv, cosT, sinT, B, H, S):
    Sp, dev = pad64(S), qkv.device
    Q = torch.empty((B, H, S, 64), device=dev, dtype=BF16); K = torch.empty_like(Q)
    VT = torch.empty((B, H, 64, Sp), device=dev, dtype=BF16)
    check(lib().ta_enc_qkv_post(ptr(qkv), ptr(cosT), ptr(sinT), ptr(Q), ptr(K), ptr(VT), B, H, S, Sp, stream()),
          "ta_enc_qkv_post")
    return Q, K, VT


def attn_bwd_prep(dO, O, B, Hq, L):
    Lp, dev = pad64(L), dO.device
    delta = torch.empty((B, Hq, L), device=dev, dtype=F32)
    dOT = torch.empty((B, Hq, 128, Lp), device=dev, dtype=BF16)
    check(lib().ta_attn_bwd_prep(ptr(dO), ptr(O), ptr(delta), ptr(dOT), B, Hq, L, Lp, stream()), "ta_attn_bwd_prep")
    return delta, dOT


def swiglu_fwd(gu, F):
    M = gu.shape[0]
    act = torch.empty((M, F), device=gu.device, dtype=BF16)
    check(lib().ta_swiglu_fwd(ptr(gu), ptr(act), M, F, stream()), "ta_swiglu_fwd")
    return act


def swiglu_bwd(dact, gu, F):
    dgu = torch.empty_like(gu)
    check(lib().ta_swiglu_bwd(ptr(dact), ptr(gu), ptr(dgu), gu.shape[0], F, stream()), "ta_swiglu_bwd")
    return dgu


def cast_bf16(x, out=None):
    _req(x, F32)
    y = torch.empty(x.shape, device=x.device, dtype=BF16) if out is None else out
    check(lib().ta_cast_f32_bf16(ptr(x), ptr(y), x.numel(), stream()), "ta_cast_f32_bf16")
    return y


def transpose_to_bf16(x, ld_out=None, in_map=None, rows=None, cols=None, out=None):
    """x [R, C] (f32 or bf16) -> bf16 [C, ld_out] (zero padded columns).  With ``in_map`` = (ld_in, batch_stride,
    rows_per_batch) the logical [rows, cols] matrix is an affine view of ``x`` (e.g. the im2col view of a padded
    time-major buffer: overlapping rows)."""
    R, Cc = (rows, cols) if rows is not None else x.shape
    ld_out = ld_out or R
    ld_in, in_bs, in_rpb = in_map or (Cc, 0, 0)
    if out is None:
        out = torch.empty((Cc, ld_out), device=x.device, dtype=BF16)
    check(lib().ta_transpose_to_bf16(ptr(x), int(x.dtype == F32), ld_in, in_bs, in_rpb, ptr(out), ld_out, R, Cc,
                                     stream()), "ta_transpose_to_bf16")
    return out


def audio_index(ids, counts, N, audio_id):
    B, L = ids.shape
    src = torch.empty(B * L, device=ids.device, dtype=torch.int32)
    check(lib().ta_audio_index(ptr(ids), ptr(counts), ptr(src), B, L, N, audio_id, stream()), "ta_audio_index")
    return src


def segment_table(segment_ids):
    """segment_ids int32 [R, L] (0 = padding, 1..S the clips of a packed row) -> (seg int32 [2, R*L]: first key index / one past the
    last row of every token's segment, pos int32 [R*L]: positions restarting at 0 in every segment).  See include/ta355.h."""
    R, L = segment_ids.shape
    seg = torch.empty((2, R * L), device=segment_ids.device, dtype=torch.int32)
    pos = torch.empty(R * L, device=segment_ids.device, dtype=torch.int32)
    check(lib().ta_segment_table(ptr(segment_ids), ptr(seg), ptr(pos), R, L, stream()), "ta_segment_table")
    return seg, pos


def audio_index_seg(ids, segment_ids, counts, N, audio_id):
    """``audio_index`` for packed rows: clip c (row of ``counts``) is the c-th segment, row-major over (row, segment)."""
    R, L = ids.shape
    src = torch.empty(R * L, device=ids.device, dtype=torch.int32)
    check(lib().ta_audio_index_seg(ptr(ids), ptr(segment_ids), ptr(counts), ptr(src), R, L, int(counts.numel()), N, audio_id, stream()),
          "ta_audio_index_seg")
    return src


def label_rows(labels):
    B, L = labels.shape
    rows = torch.empty(B * L, device=labels.device, dtype=torch.int32)
    tg = torch.empty(B * L, device=labels.device, dtype=torch.int64)
    n = torch.zeros(1, device=labels.device, dtype=torch.int32)
    check(lib().ta_label_rows(ptr(labels), B, L, ptr(rows), ptr(tg), ptr(n), stream()), "ta_label_rows")
    return rows, tg, n


def cross_entropy(logits, targets, V, scale, rows=None, want_dlogits=True, ldd=None):
    n = targets.shape[0]
    ldl = logits.shape[1]
    ldd = ldd or ldl
    nll = torch.empty(n, device=logits.device, dtype=F32)
    loss = torch.zeros(1, device=logits.device, dtype=F32)
    dl = torch.empty((n, ldd), device=logits.device, dtype=BF16) if want_dlogits else None
    check(lib().ta_cross_entropy(ptr(logits), int(logits.dtype == BF16), ldl, ptr(rows), ptr(targets), n, V, scale,
                                 ptr(nll), ptr(loss), ptr(dl), ldd, stream()), "ta_cross_entropy")
    return loss, nll, dl


def cross_entropy_opt(logits, targets, V, scale, label_smoothing=0.0, z_loss=0.0, rows=None, want_dlogits=True, ldd=None):
    """``cross_entropy`` with the loss options of include/ta355.h ta_ce_options -> (loss, nll, dlogits, obj): loss and dlogits are the
    objective's, obj its per-row terms, nll stays the plain NLL (both options 0: obj == nll)."""
    eps, zc = float(label_smoothing), float(z_loss)
    if not 0.0 <= eps < 1.0 or not zc >= 0.0:
        raise ValueError(f"label_smoothing must lie in [0, 1) and z_loss must be >= 0; got {label_smoothing}, {z_loss}")
    n = targets.shape[0]
    ldl = logits.shape[1]
    ldd = ldd or ldl
    nll = torch.empty(n, device=logits.device, dtype=F32)
    obj = torch.empty(n, device=logits.device, dtype=F32)
    loss = torch.zeros(1, device=logits.device, dtype=F32)
    dl = torch.empty((n, ldd), device=logits.device, dtype=BF16) if want_dlogits else None
    ce = _lib.CeOptions(eps=eps, zc=zc, obj=obj.data_ptr())
    check(lib().ta_cross_entropy_opt(ptr(logits), int(logits.dtype == BF16), ldl, ptr(rows), ptr(targets), n, V, scale,
                                     ptr(nll), ptr(loss), ptr(dl), ldd, C.byref(ce), stream()), "ta_cross_entropy_opt")
    return loss, nll, dl, obj


def bernoulli_keep(n, keep_prob, seed, device):
    keep = torch.empty(n, device=device, dtype=F32)
    check(lib().ta_bernoulli_keep(ptr(keep), n, keep_prob, seed, stream()), "ta_bernoulli_keep")
    return keep


def grad_sqnorm(g, accum, scratch=None):
    """accum[0] += sum(g ** 2), bit-reproducibly (``scratch``: f32 [1024], allocated here when not given)."""
    if scratch is None:
        scratch = torch.empty(1024, device=g.device, dtype=F32)
    check(lib().ta_grad_sqnorm(ptr(g), g.numel(), ptr(accum), ptr(scratch), stream()), "ta_grad_sqnorm")


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, sqnorm=None, max_norm=0.0, grad_scale=1.0, denom=None):
    check(lib().ta_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, wd, step, ptr(sqnorm),
                              max_norm, grad_scale, ptr(denom), stream()), "ta_adamw_step")


def adamw_step_multi(p, g, m, v, seg_end, seg_lr, seg_wd, lr_mult, beta1, beta2, eps, step, sqnorm=None, max_norm=0.0, grad_scale=1.0,
                     denom=None):
    """One launch over a flat buffer of parameter segments (seg_end int64, seg_lr / seg_wd f32, all on the device)."""
    check(lib().ta_adamw_step_multi(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(seg_end), ptr(seg_lr), ptr(seg_wd), seg_end.numel(),
                                    lr_mult, beta1, beta2, eps, step, ptr(sqnorm), max_norm, grad_scale, ptr(denom), stream()),
          "ta_adamw_step_multi")


# ----------------------------------------------------------------------------- trainable-projector primitives (nn_prims.hip)
def gelu_fwd(h):
    _req(h, BF16)
    a = torch.empty_like(h)
    check(lib().ta_gelu_fwd(ptr(h), ptr(a), h.numel(), stream()), "ta_gelu_fwd")
    return a


def gelu_bwd(da, h):
    _req(da, BF16); _req(h, BF16)
    dh = torch.empty_like(h)
    check(lib().ta_gelu_bwd(ptr(da), ptr(h), ptr(dh), h.numel(), stream()), "ta_gelu_bwd")
    return dh


def colsum(x):
    """[R, C] (f32 or bf16) -> f32 [C]"""
    R, Cc = x.shape
    out = torch.empty(Cc, device=x.device, dtype=F32)
    check(lib().ta_colsum(ptr(x), int(x.dtype == F32), R, Cc, ptr(out), stream()), "ta_colsum")
    return out


def layernorm_res_fwd(z, gamma, beta, eps, res=None, keep=None, res_rows=0):
    """-> (y f32, y bf16, xhat, rstd)"""
    _req(z, F32)
    M, H = z.shape
    yf = torch.empty_like(z)
    yb = torch.empty((M, H), device=z.device, dtype=BF16)
    xhat, rstd = torch.empty_like(z), torch.empty(M, device=z.device, dtype=F32)
    check(lib().ta_layernorm_res_fwd(ptr(z), ptr(keep), ptr(res), res_rows, ptr(gamma), ptr(beta), eps, ptr(xhat), ptr(rstd),
                                     ptr(yf), ptr(yb), M, H, stream()), "ta_layernorm_res_fwd")
    return yf, yb, xhat, rstd


def layernorm_bwd(dy, xhat, rstd, gamma, dgamma, dbeta, keep=None, want_du=True, want_dz=True):
    """-> (du f32 or None, dz bf16 or None); dgamma / dbeta accumulate."""
    _req(dy, F32)
    M, H = dy.shape
    du = torch.empty_like(dy) if want_du else None
    dz = torch.empty((M, H), device=dy.device, dtype=BF16) if want_dz else None
    check(lib().ta_layernorm_bwd(ptr(dy), ptr(xhat), ptr(rstd), ptr(gamma), ptr(keep), ptr(du), ptr(dz), ptr(dgamma),
                                 ptr(dbeta), M, H, stream()), "ta_layernorm_bwd")
    return du, dz


def attn_small_fwd(Q, K, V, EB, heads, Lq, Lk, scale, keep=None):
    _req(Q, BF16); _req(K, BF16); _req(V, BF16)
    H = Q.shape[-1]
    P = torch.empty((EB, heads, Lq, Lk), device=Q.device, dtype=F32)
    O = torch.empty((EB * Lq, H), device=Q.device, dtype=BF16)
    check(lib().ta_attn_small_fwd(ptr(Q), ptr(K), ptr(V), EB, heads, H // heads, Lq, Lk, scale, ptr(keep), ptr(P), ptr(O),
                                  stream()), "ta_attn_small_fwd")
    return O, P


def attn_small_bwd(dO, Q, K, V, P, EB, heads, Lq, Lk, scale, keep=None):
    _req(dO, BF16)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    H = Q.shape[-1]
    check(lib().ta_attn_small_bwd(ptr(dO), ptr(Q), ptr(K), ptr(V), ptr(P), ptr(keep), scale, ptr(dQ), ptr(dK), ptr(dV), EB,
                                  heads, H // heads, Lq, Lk, stream()), "ta_attn_small_bwd")
    return dQ, dK, dV


def relu_fwd(h):
    _req(h, BF16)
    a = torch.empty_like(h)
    check(lib().ta_relu_fwd(ptr(h), ptr(a), h.numel(), stream()), "ta_relu_fwd")
    return a


def relu_bwd(da, h):
    _req(da, BF16); _req(h, BF16)
    dh = torch.empty_like(h)
    check(lib().ta_relu_bwd(ptr(da), ptr(h), ptr(dh), h.numel(), stream()), "ta_relu_bwd")
    return dh


def mix_fwd(logits, o):
    """logits f32 [M, E], o f32 [E, M, D] -> (rw [M, E], out [M, D])"""
    _req(logits, F32); _req(o, F32)
    E, M, D = o.shape
    rw = torch.empty((M, E), device=o.device, dtype=F32)
    out = torch.empty((M, D), device=o.device, dtype=F32)
    check(lib().ta_mix_fwd(ptr(logits), ptr(o), ptr(rw), ptr(out), M, D, E, stream()), "ta_mix_fwd")
    return rw, out


def mix_bwd(dout, o, rw):
    """-> (do bf16 [E, M, D], dlogits f32 [M, E])"""
    _req(dout, F32)
    E, M, D = o.shape
    dob = torch.empty((E, M, D), device=o.device, dtype=BF16)
    dlg = torch.empty((M, E), device=o.device, dtype=F32)
    check(lib().ta_mix_bwd(ptr(dout), ptr(o), ptr(rw), ptr(dob), ptr(dlg), M, D, E, stream()), "ta_mix_bwd")
    return dob, dlg


# ----------------------------------------------------------------------------- forced alignment (csrc/align.hip)
ALIGN_LIMITS = {"clips": 4096, "frames": 32768, "tokens": 2048, "classes": 65536}      # TA_ALIGN_MAX_* of include/ta355.h


def ctc_align(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens, *, frames=None, trellis_off=None,
              trellis_numel=0, trellis=None):
    """ta_ctc_align_f32: N ragged clips in one launch.  ``emission`` f32 [sum T_n, C] log-probabilities (rows may be strided),
    ``cu_frames`` / ``cu_tokens`` int32 [N + 1], ``tokens`` int32 [sum J_n], all on the device; ``max_frames`` / ``max_tokens`` bound
    every clip (the caller built the lengths on the host).  -> (frames int32 [sum J_n], score f32 [N], status int32 [N], trellis):
    ``frames`` (given, or a new tensor of -1) is written for aligned clips only; ``trellis`` is None unless ``trellis_off``
    (int64 [N], element offsets) and ``trellis_numel`` ask for every clip's [T_n + 1, J_n + 1] trellis in one flat f32 tensor
    (``trellis``: a tensor of that size to write into).
    The cumulative lengths and the offsets live on the device and are NOT checked here (that would cost a synchronisation, as with
    ``cu_rows`` of the ragged encoder): ``cu_frames[N] <= emission.shape[0]``, ``cu_tokens[N] == tokens.numel()`` and
    ``trellis_off[n] + (T_n + 1) (J_n + 1) <= trellis_numel`` are the caller's responsibility.  The kernel itself refuses (status 2,
    score -inf, nothing else written) a clip longer than ``max_frames`` / ``max_tokens`` and a token id outside [0, C)."""
    if not (emission.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("ctc_align needs the emissions on a HIP device: there is no CPU path for the trellis")
    assert emission.dim() == 2 and emission.dtype == F32 and (emission.stride(1) == 1 or emission.numel() == 0), \
        "emission: f32 [frames, C], unit column stride"
    C_ = emission.shape[1]
    ld = emission.stride(0) if emission.shape[0] > 1 else C_
    N = cu_frames.numel() - 1
    for name, v, lim in (("clips", N, "clips"), ("frames per clip", max_frames, "frames"), ("tokens per clip", max_tokens, "tokens"),
                         ("classes", C_, "classes")):
        if v > ALIGN_LIMITS[lim]:
            raise ValueError(f"ctc_align: {v} {name} is beyond the kernel's limit of {ALIGN_LIMITS[lim]}")
    if not 0 <= blank_id < C_:
        raise ValueError(f"ctc_align: blank_id {blank_id} is outside [0, {C_})")
    if ld < C_:
        raise ValueError("ctc_align: emission rows overlap")
    dev = emission.device
    for t in (cu_frames, tokens, cu_tokens):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == dev
    assert cu_tokens.numel() == N + 1 and N >= 0
    if frames is None:
        frames = torch.full((tokens.numel(),), -1, device=dev, dtype=torch.int32)
    assert frames.dtype == torch.int32 and frames.is_contiguous() and frames.numel() == tokens.numel() and frames.device == dev
    score = torch.empty(N, device=dev, dtype=F32)
    status = torch.empty(N, device=dev, dtype=torch.int32)
    if trellis_off is None:
        trellis = None
    else:
        assert trellis_off.dtype == torch.int64 and trellis_off.numel() == N and trellis_off.device == dev
        if trellis is None:
            trellis = torch.empty(int(trellis_numel), device=dev, dtype=F32)
        assert trellis.dtype == F32 and trellis.is_contiguous() and trellis.numel() == int(trellis_numel) and trellis.device == dev
    L = lib()
    ws_bytes = L.ta_ctc_align_workspace_bytes(N, int(max_frames), int(max_tokens))
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    check(L.ta_ctc_align_f32(ptr(emission), ld, C_, ptr(cu_frames), ptr(tokens), ptr(cu_tokens), N, int(max_frames), int(max_tokens),
                             int(blank_id), ptr(frames), ptr(score), ptr(status), ptr(ws), ws_bytes, ptr(trellis), ptr(trellis_off),
                             stream()), "ta_ctc_align_f32")
    return frames, score, status, trellis


# ----------------------------------------------------------------------------- forced alignment, long form (csrc/align_long.hip)
ALIGN_LONG_LIMITS = {"clips": 64, "frames": 1048576, "tokens": 262144, "classes": 65536,      # TA_ALIGN_LONG_MAX_* of include/ta355.h
                     "col_block": 2048}


def ctc_align_long(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens, *, col_block=0, frame_block=0, frames=None,
                   trellis_off=None, trellis_numel=0, trellis=None, workspace=None):
    """ta_ctc_align_long_f32: ``ctc_align`` (same arguments, same returns, same bytes) beyond its envelope, as a tiled wavefront of
    launches.  ``col_block`` (a multiple of 64 up to 2048) and ``frame_block`` (>= 1) set the tile, 0 = the library's default; the
    results do not depend on them.  ``workspace``: a uint8 device tensor of at least ``ta_ctc_align_long_workspace_bytes`` bytes to
    use instead of a new one (its contents do not matter).  The unchecked device-side tables are the caller's responsibility as in
    ``ctc_align``."""
    if not (emission.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("ctc_align_long needs the emissions on a HIP device: there is no CPU path for the trellis")
    assert emission.dim() == 2 and emission.dtype == F32 and (emission.stride(1) == 1 or emission.numel() == 0), \
        "emission: f32 [frames, C], unit column stride"
    C_ = emission.shape[1]
    ld = emission.stride(0) if emission.shape[0] > 1 else C_
    N = cu_frames.numel() - 1
    for name, v, lim in (("clips", N, "clips"), ("frames per clip", max_frames, "frames"), ("tokens per clip", max_tokens, "tokens"),
                         ("classes", C_, "classes")):
        if v > ALIGN_LONG_LIMITS[lim]:
            raise ValueError(f"ctc_align_long: {v} {name} is beyond the kernel's limit of {ALIGN_LONG_LIMITS[lim]}")
    col_block, frame_block = int(col_block), int(frame_block)
    if col_block < 0 or col_block % 64 or col_block > ALIGN_LONG_LIMITS["col_block"]:
        raise ValueError(f"ctc_align_long: col_block {col_block} must be a multiple of 64 up to {ALIGN_LONG_LIMITS['col_block']} "
                         "(0 = the default)")
    if frame_block < 0:
        raise ValueError(f"ctc_align_long: frame_block {frame_block} must be at least 1 (0 = the default)")
    if not 0 <= blank_id < C_:
        raise ValueError(f"ctc_align_long: blank_id {blank_id} is outside [0, {C_})")
    if ld < C_:
        raise ValueError("ctc_align_long: emission rows overlap")
    dev = emission.device
    for t in (cu_frames, tokens, cu_tokens):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == dev
    if cu_tokens.numel() != N + 1 or N < 0:
        raise ValueError(f"ctc_align_long: cu_frames holds {N + 1} entries but cu_tokens {cu_tokens.numel()}")
    if frames is None:
        frames = torch.full((tokens.numel(),), -1, device=dev, dtype=torch.int32)
    assert frames.dtype == torch.int32 and frames.is_contiguous() and frames.numel() == tokens.numel() and frames.device == dev
    score = torch.empty(N, device=dev, dtype=F32)
    status = torch.empty(N, device=dev, dtype=torch.int32)
    if trellis_off is None:
        trellis = None
    else:
        assert trellis_off.dtype == torch.int64 and trellis_off.numel() == N and trellis_off.device == dev
        if trellis is None:
            trellis = torch.empty(int(trellis_numel), device=dev, dtype=F32)
        assert trellis.dtype == F32 and trellis.is_contiguous() and trellis.numel() == int(trellis_numel) and trellis.device == dev
    L = lib()
    ws_bytes = L.ta_ctc_align_long_workspace_bytes(N, int(max_frames), int(max_tokens), col_block, frame_block)
    if workspace is None:
        workspace = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= ws_bytes and workspace.device == dev
    check(L.ta_ctc_align_long_f32(ptr(emission), ld, C_, ptr(cu_frames), ptr(tokens), ptr(cu_tokens), N, int(max_frames),
                                  int(max_tokens), int(blank_id), col_block, frame_block, ptr(frames), ptr(score), ptr(status),
                                  ptr(workspace), ws_bytes, ptr(trellis), ptr(trellis_off), stream()), "ta_ctc_align_long_f32")
    return frames, score, status, trellis


# ----------------------------------------------------------------------------- text alignment (csrc/text_align.hip)
TEXT_ALIGN_LIMITS = {"pairs": 65536, "length": 262144, "col_block": 512, "short_m": 512}      # TA_TEXT_ALIGN_* of include/ta355.h
TEXT_ALIGN_EDIT, TEXT_ALIGN_LCS = 0, 1
TEXT_ALIGN_MAX_WORKSPACE = 8 << 30


def text_align_workspace_bytes(cu_ref_host, cu_hyp_host, max_n, max_m, want_path, col_block=0, row_block=0, pairs=None):
    """ta_text_align_workspace_bytes from HOST copies of the cumulative lengths (int32 CPU tensors), or, with None for both and the
    number of ``pairs``, its fixed part alone: all that a call without ``want_path`` needs."""
    for t in (cu_ref_host, cu_hyp_host):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and not t.is_cuda)
    N = int(pairs) if cu_ref_host is None else cu_ref_host.numel() - 1
    return lib().ta_text_align_workspace_bytes(ptr(cu_ref_host), ptr(cu_hyp_host), N, int(max_n), int(max_m), int(bool(want_path)),
                                               int(col_block), int(row_block))


def text_align(ref, cu_ref, hyp, cu_hyp, max_n, max_m, mode, want_path, *, col_block=0, row_block=0, map=None, workspace=None,
               max_workspace_bytes=TEXT_ALIGN_MAX_WORKSPACE):
    """ta_text_align_i32: N ragged pairs of int32 symbol ids in one call.  ``ref`` int32 [sum n_p], ``hyp`` int32 [sum m_p],
    ``cu_ref`` / ``cu_hyp`` int32 [N + 1], all on the device; ``max_n`` / ``max_m`` bound every pair.  ``mode``: 0 edit distance, 1 LCS.
    -> (dist int32 [N], counts int32 [N, 4] = hits, substitutions, deletions, insertions, map int32 [sum n_p], status int32 [N]).
    Without ``want_path`` only dist and status are written (counts stays zero, map is None).  ``map`` (given, or a new tensor of -1)
    is written for accepted pairs only.  ``col_block`` / ``row_block``: the long kernel's tile, 0 = the default; both 0 lets pairs
    whose hypotheses fit one tile run in the short kernel; no output byte depends on them.  ``workspace``: a uint8 device tensor to
    use instead of a new one; without it a path request reads the cumulative lengths back to size the decision bits from the actual
    pairs (one synchronisation) and is refused beyond ``max_workspace_bytes``.  A pair beyond the maxima gets status 2."""
    if not (ref.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("text_align needs the symbols on a HIP device: there is no CPU path for the tables")
    dev = ref.device
    for t in (ref, cu_ref, hyp, cu_hyp):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == dev, "int32, flat, contiguous, one device"
    N = cu_ref.numel() - 1
    if N < 0 or cu_hyp.numel() != N + 1:
        raise ValueError(f"text_align: cu_ref holds {N + 1} entries but cu_hyp {cu_hyp.numel()}")
    max_n, max_m, col_block, row_block, want_path = int(max_n), int(max_m), int(col_block), int(row_block), bool(want_path)
    if N > TEXT_ALIGN_LIMITS["pairs"]:
        raise ValueError(f"text_align: {N} pairs is beyond the kernel's limit of {TEXT_ALIGN_LIMITS['pairs']}")
    for name, v in (("reference", max_n), ("hypothesis", max_m)):
        if not 0 <= v <= TEXT_ALIGN_LIMITS["length"]:
            raise ValueError(f"text_align: a {name} length of {v} is outside the kernel's limit of {TEXT_ALIGN_LIMITS['length']}")
    if ref.numel() == 0:                 # nothing to point at: a pair that claims symbols all the same is refused, not read
        max_n = 0
    if hyp.numel() == 0:
        max_m = 0
    if mode not in (TEXT_ALIGN_EDIT, TEXT_ALIGN_LCS):
        raise ValueError(f"text_align: mode {mode} is neither 0 (edit) nor 1 (lcs)")
    if col_block not in (0, 64, 128, 256, 512):
        raise ValueError(f"text_align: col_block {col_block} must be 64, 128, 256 or 512 (0 = the default)")
    if row_block < 0 or row_block % 64 or row_block > TEXT_ALIGN_LIMITS["length"]:
        raise ValueError(f"text_align: row_block {row_block} must be a multiple of 64 (0 = the default)")
    if want_path:
        if map is None:
            map = torch.full((ref.numel(),), -1, device=dev, dtype=torch.int32)
        assert map.dtype == torch.int32 and map.is_contiguous() and map.numel() == ref.numel() and map.device == dev
    else:
        map = None
    if workspace is None:
        host = (cu_ref.cpu(), cu_hyp.cpu()) if want_path and N > 0 else (None, None)
        ws_bytes = text_align_workspace_bytes(*host, max_n, max_m, want_path, col_block, row_block, pairs=N)
        if want_path and ws_bytes > int(max_workspace_bytes):
            raise ValueError(f"text_align: the paths of this batch need a workspace of {ws_bytes} bytes, beyond max_workspace_bytes = "
                             f"{int(max_workspace_bytes)}; ask for distances only, or split the batch")
        workspace = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
    dist = torch.zeros(N, device=dev, dtype=torch.int32)
    counts = torch.zeros((N, 4), device=dev, dtype=torch.int32)
    status = torch.zeros(N, device=dev, dtype=torch.int32)
    check(lib().ta_text_align_i32(ptr(ref), ptr(cu_ref), ptr(hyp), ptr(cu_hyp), N, max_n, max_m, int(mode), int(want_path), col_block,
                                  row_block, ptr(dist), ptr(counts), ptr(map), ptr(status), ptr(workspace), workspace.numel(),
                                  stream()), "ta_text_align_i32")
    return dist, counts, map, status


# ----------------------------------------------------------------------------- long-form segmentation (csrc/segment.hip)
SEGMENT_LIMITS = {"recordings": 64, "positions": 1048576, "max_len": 3000, "smooth": 64, "windows": 65535, "blocks": 131072}     # TA_CUT_* of include/ta355.h
CUT_HOP = 160


def cut_cost_K(smooth_positions: int) -> int:
    """TA_CUT_COST_K(h): the kernel's longest chain of additions + 3 (its error bound is gamma_K * cost)."""
    return max(2 * int(smooth_positions) + 25, 65)


def _segment_batch(wav, offsets, max_samples, what):
    if not (wav.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error(f"{what} needs the recordings on a HIP device: there is no CPU path")
    assert wav.dim() == 1 and wav.dtype == F32 and wav.is_contiguous(), "wav: one flat contiguous f32 buffer"
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.device == wav.device
    R, max_samples = offsets.numel() - 1, int(max_samples)
    if R < 0 or R > SEGMENT_LIMITS["recordings"]:
        raise ValueError(f"{what}: {R} recordings, the kernels take at most {SEGMENT_LIMITS['recordings']} per call")
    if max_samples < 1:
        raise ValueError(f"{what}: max_samples must be at least 1")
    max_T = -(-max_samples // CUT_HOP)
    if max_T > SEGMENT_LIMITS["positions"]:
        raise ValueError(f"{what}: {max_samples} samples are {max_T} positions, beyond the kernel's limit of "
                         f"{SEGMENT_LIMITS['positions']} ({SEGMENT_LIMITS['positions'] * CUT_HOP / 16000 / 3600:.1f} h at 16 kHz)")
    return R, max_samples, max_T


def wave_cut_cost(wav, offsets, max_samples, smooth_positions=10, cut_penalty=0.05):
    """ta_wave_cut_cost_f32: ``wav`` flat f32 (device), ``offsets`` int64 [R + 1] (device; recording r is wav[offsets[r]:offsets[r + 1]]),
    ``max_samples`` >= every recording's length (known on the host: it sizes the rows) -> cost f32 [R, max_T + 1], row r filled for the
    positions 0 .. T_r = ceil(n_r / 160); the rest of a row, and the row of a recording longer than ``max_samples``, keeps its NaN."""
    R, max_samples, max_T = _segment_batch(wav, offsets, max_samples, "wave_cut_cost")
    h = int(smooth_positions)
    if not 0 <= h <= SEGMENT_LIMITS["smooth"]:
        raise ValueError(f"wave_cut_cost: smooth_positions must be within [0, {SEGMENT_LIMITS['smooth']}]; got {smooth_positions}")
    cut_penalty = float(cut_penalty)
    if not (0.0 <= cut_penalty < float("inf")):
        raise ValueError(f"wave_cut_cost: cut_penalty must be finite and >= 0; got {cut_penalty}")
    cost = torch.full((R, max_T + 1), float("nan"), device=wav.device, dtype=F32)
    if R == 0:
        return cost
    L = lib()
    ws_bytes = L.ta_wave_cut_cost_workspace_bytes(R, max_samples)
    ws = torch.empty(max(ws_bytes, 8), device=wav.device, dtype=torch.uint8)
    check(L.ta_wave_cut_cost_f32(ptr(wav), ptr(offsets), R, max_samples, h, cut_penalty, ptr(cost), max_T + 1, ptr(ws), ws_bytes, stream()),
          "ta_wave_cut_cost_f32")
    return cost


def cut_plan(cost, offsets, max_samples, min_len, max_len):
    """ta_cut_plan_f32 on ``wave_cut_cost``'s rows: windows of ``min_len`` .. ``max_len`` positions at the least total cost ->
    (cuts int32 [R, max_T // min_len + 2], n_seg int32 [R], dp_T f32 [R], back int32 [R, max_T + 1]); recording r is cut at the
    positions cuts[r, 0] = 0 < ... < cuts[r, n_seg[r]] = T_r.  Entries the kernel does not write hold -1."""
    assert cost.dim() == 2 and cost.dtype == F32 and cost.is_contiguous()
    flat = torch.empty(0, device=cost.device, dtype=F32)
    R, max_samples, max_T = _segment_batch(flat, offsets, max_samples, "cut_plan")
    min_len, max_len = int(min_len), int(max_len)
    if min_len < 1 or 2 * min_len > max_len or max_len > SEGMENT_LIMITS["max_len"]:
        raise ValueError(f"cut_plan: 1 <= min_len, 2 * min_len <= max_len <= {SEGMENT_LIMITS['max_len']} must hold; "
                         f"got min_len={min_len}, max_len={max_len}")
    if cost.shape[0] != R or cost.shape[1] < max_T + 1:
        raise ValueError(f"cut_plan: cost is {tuple(cost.shape)}, {R} recordings of up to {max_T + 1} positions need [{R}, >= {max_T + 1}]")
    if max_T // min_len > SEGMENT_LIMITS["blocks"]:
        raise ValueError(f"cut_plan: {max_T} positions in blocks of min_len={min_len} are more than {SEGMENT_LIMITS['blocks']} sequential "
                         "steps of one workgroup: raise min_len")
    dev, i32 = cost.device, torch.int32
    ldc = max_T // min_len + 2
    back = torch.full((R, cost.shape[1]), -1, device=dev, dtype=i32)
    cuts = torch.full((R, ldc), -1, device=dev, dtype=i32)
    n_seg = torch.full((R,), -1, device=dev, dtype=i32)
    dp_T = torch.full((R,), float("inf"), device=dev, dtype=F32)
    if R:
        check(lib().ta_cut_plan_f32(ptr(cost), cost.shape[1], ptr(offsets), R, max_samples, min_len, max_len, ptr(back), ptr(cuts), ldc,
                                    ptr(n_seg), ptr(dp_T), stream()), "ta_cut_plan_f32")
    return cuts, n_seg, dp_T, back


def wave_windows(wav, start, length, Ls, out=None):
    """ta_wave_windows_f32: ``wav`` flat f32, ``start`` int64 [W] (indices into ``wav``), ``length`` int32 [W], all on the device ->
    (out f32 [W, Ls]: window w's samples then zeros, lens int64 [W] = the lengths clamped to [0, Ls]): what ``ta_logmel_f32`` takes."""
    if not (wav.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("wave_windows needs the recordings on a HIP device: there is no CPU path")
    assert wav.dim() == 1 and wav.dtype == F32 and wav.is_contiguous(), "wav: one flat contiguous f32 buffer"
    dev = wav.device
    assert start.dtype == torch.int64 and start.dim() == 1 and start.is_contiguous() and start.device == dev
    assert length.dtype == torch.int32 and length.shape == start.shape and length.is_contiguous() and length.device == dev
    W, Ls = start.numel(), int(Ls)
    if W > SEGMENT_LIMITS["windows"]:
        raise ValueError(f"wave_windows: {W} windows, the kernel takes at most {SEGMENT_LIMITS['windows']} per call")
    if Ls < 1:
        raise ValueError(f"wave_windows: Ls must be at least 1; got {Ls}")
    if out is None:
        out = torch.empty((W, Ls), device=dev, dtype=F32)
    assert out.dtype == F32 and out.shape == (W, Ls) and out.is_contiguous() and out.device == dev
    lens = torch.empty(W, device=dev, dtype=torch.int64)
    if W:
        check(lib().ta_wave_windows_f32(ptr(wav), wav.numel(), ptr(start), ptr(length), W, Ls, ptr(out), ptr(lens), stream()),
              "ta_wave_windows_f32")
    return out, lens


# ----------------------------------------------------------------------------- voice activity detection (csrc/vad.hip)
VAD_LIMITS = {"recordings": 64, "samples": 160 * 1048576, "smooth": 8, "noise_window": 1024}      # TA_CUT_* / TA_VAD_* of include/ta355.h
VAD_HOP = 256
VAD_TILE = 256                 # frames per workgroup of the statistic kernel (TA_VAD_TILE)
VAD_ENERGY_FRAMES = 32         # frames per workgroup of the band-energy kernel (TA_VAD_ENERGY_FRAMES)


def vad_frames(n: int) -> int:
    """ta_vad_frames: the frames i >= 0 with 256 i < n - 256 -- ``len(range(0, n - 256, 256))``, the diarizer's loop count."""
    n = int(n)
    return 0 if n <= VAD_HOP else (n - 1) // VAD_HOP


def check_vad_options(smooth, noise_window, noise_bias, threshold, floor):
    """The ranges of ``ta_vad_options`` -> (h, W, beta, theta, e0) or ``ValueError``."""
    import math
    h, W, beta, theta, e0 = int(smooth), int(noise_window), float(noise_bias), float(threshold), float(floor)
    if not 0 <= h <= VAD_LIMITS["smooth"]:
        raise ValueError(f"vad: smooth must be within [0, {VAD_LIMITS['smooth']}] frames; got {smooth}")
    if not 1 <= W <= VAD_LIMITS["noise_window"]:
        raise ValueError(f"vad: noise_window must be within [1, {VAD_LIMITS['noise_window']}] frames; got {noise_window}")
    if not (math.isfinite(beta) and beta >= 1.0):
        raise ValueError(f"vad: noise_bias must be finite and >= 1; got {noise_bias}")
    if not (math.isfinite(theta) and theta > 0.0):
        raise ValueError(f"vad: threshold must be finite and > 0; got {threshold}")
    if not (math.isfinite(e0) and e0 > 0.0 and float(torch.tensor(e0, dtype=F32)) > 0.0):
        raise ValueError(f"vad: floor must be finite and > 0 in f32; got {floor}")
    return h, W, beta, theta, e0


def vad(wav, offsets, max_samples, smooth=2, noise_window=94, noise_bias=2.0, threshold=0.15, floor=1e-12, stat=None, flags=None):
    """ta_vad_f32: ``wav`` flat f32 (device), ``offsets`` int64 [R + 1] (device; recording r is wav[offsets[r]:offsets[r + 1]], at any
    sample offset), ``max_samples`` >= every recording's length -> (stat f32 [R, ld] = the likelihood-ratio statistic L, flags uint8
    [R, ld] = L > threshold, n_frames int32 [R]) with ld = vad_frames(max_samples); row r is written for its own
    ``vad_frames(n_r)`` frames, the rest keeps its zeros.  ``stat`` / ``flags`` may be passed in ([R, ld >= vad_frames(max_samples)],
    contiguous): positions the kernel does not write keep what they held."""
    if not (wav.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("vad needs the recordings on a HIP device: there is no CPU path")
    if wav.dim() != 1 or offsets.dim() != 1:
        raise ValueError(f"vad: wav must be one flat 1-D buffer and offsets 1-D; got {tuple(wav.shape)} and {tuple(offsets.shape)}")
    assert wav.dtype == F32 and wav.is_contiguous(), "wav: one flat contiguous f32 buffer"
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.device == wav.device
    R, max_samples = offsets.numel() - 1, int(max_samples)
    if R < 0 or R > VAD_LIMITS["recordings"]:
        raise ValueError(f"vad: {R} recordings, the kernels take at most {VAD_LIMITS['recordings']} per call")
    if max_samples < 1:
        raise ValueError("vad: max_samples must be at least 1")
    if max_samples > VAD_LIMITS["samples"]:
        raise ValueError(f"vad: {max_samples} samples are beyond the kernel's limit of {VAD_LIMITS['samples']} "
                         f"({VAD_LIMITS['samples'] / 16000 / 3600:.1f} h at 16 kHz)")
    h, W, beta, theta, e0 = check_vad_options(smooth, noise_window, noise_bias, threshold, floor)
    dev, maxF = wav.device, vad_frames(max_samples)
    if stat is None:
        stat = torch.zeros((R, maxF), device=dev, dtype=F32)
    if flags is None:
        flags = torch.zeros((R, stat.shape[1] if stat.dim() == 2 else maxF), device=dev, dtype=torch.uint8)
    if stat.dim() != 2 or stat.shape[0] != R or stat.shape[1] < maxF or flags.shape != stat.shape:
        raise ValueError(f"vad: stat is {tuple(stat.shape)} and flags {tuple(flags.shape)}: {R} recordings of up to {maxF} frames need "
                         f"two [{R}, ld >= {maxF}] buffers of one shape")
    assert stat.dtype == F32 and flags.dtype == torch.uint8 and stat.is_contiguous() and flags.is_contiguous()
    assert stat.device == dev and flags.device == dev
    n_frames = torch.zeros(R, device=dev, dtype=torch.int32)
    if R == 0:
        return stat, flags, n_frames
    L = lib()
    ws_bytes = L.ta_vad_workspace_bytes(R, max_samples)
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    opt = _lib.VadOptions(h, W, beta, theta, e0)
    check(L.ta_vad_f32(ptr(wav), ptr(offsets), R, max_samples, C.byref(opt), ptr(stat), ptr(flags), stat.shape[1], ptr(n_frames),
                       ptr(ws), ws_bytes, stream()), "ta_vad_f32")
    return stat, flags, n_frames


# ----------------------------------------------------------------------------- speaker turns (csrc/speaker_post.hip)
SPK_LIMITS = {"recordings": 64, "speakers": 16, "frames": 1048577, "items": 1048576}      # TA_SPK_MAX_* of include/ta355.h
SPK_FRAME_TILE = 1024          # frames per workgroup of the owner and compaction kernels (TA_SPK_FRAME_TILE)
SPK_SEG_TILE = 1024            # segments staged through LDS at a time by the words kernel (TA_SPK_SEG_TILE)
SPK_OPTION_NAMES = ("voting_rate", "vad_frame_s", "min_segment_s", "short_gap_s", "same_gap_s")
I32 = torch.int32
F64 = torch.float64


def check_spk_options(options):
    """The five ``ta_spk_post_options`` in seconds -> a tuple of floats, or ``ValueError`` naming the one that is not finite and > 0."""
    import math
    options = tuple(float(v) for v in options)
    if len(options) != len(SPK_OPTION_NAMES):
        raise ValueError(f"speaker turns: {len(SPK_OPTION_NAMES)} options are expected ({', '.join(SPK_OPTION_NAMES)}); got {len(options)}")
    for name, v in zip(SPK_OPTION_NAMES, options):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"speaker turns: {name} must be finite and > 0; got {v}")
    return options


def _spk_ragged(name, cu, *arrays, what):
    """cu int32 [R + 1] and the flat arrays it indexes -> R, after the shape, dtype and count checks that need no read-back."""
    dev = cu.device
    if cu.dim() != 1 or cu.numel() < 1 or cu.dtype != I32:
        raise ValueError(f"{name}: the offsets must be int32 [R + 1]; got {tuple(cu.shape)} {cu.dtype}")
    R = cu.numel() - 1
    if R > SPK_LIMITS["recordings"]:
        raise ValueError(f"{name}: {R} recordings, the kernels take at most {SPK_LIMITS['recordings']} per call")
    n = arrays[0].numel()
    if n > SPK_LIMITS["items"]:
        raise ValueError(f"{name}: {n} {what}, the kernels take at most {SPK_LIMITS['items']} per call")
    for a in arrays:
        if a.dim() != 1 or a.numel() != n or a.dtype != arrays[0].dtype or a.device != dev or not a.is_contiguous():
            raise ValueError(f"{name}: the {what} must be flat contiguous arrays of one length, dtype and device")
    assert cu.is_contiguous()
    return R


def _spk_check_cu(name, cu, n, what):
    """One read-back of the offsets: ascending from 0 to n (n None: to anything)."""
    c = cu.cpu().tolist()
    n = c[-1] if n is None else n
    if c[0] != 0 or c[-1] != n or any(b < a for a, b in zip(c, c[1:])):
        raise ValueError(f"{name}: the offsets of the {what} must ascend from 0 to their count {n}; got {c[:4]} .. {c[-1]}")
    return c


def spk_vote(first, last, label, cu_win, S, n_frames, max_frames, vad, n_vad, cu_cap, options, out=None, capacity=None):
    """ta_spk_vote_i32: windows ``first`` / ``last`` / ``label`` int32 [sum Nw] of R recordings (``cu_win`` int32 [R + 1]; labels in
    [0, S)) vote on the frames they cover of grids of ``n_frames`` int32 [R] frames (each <= ``max_frames``); ``vad`` uint8 [R, ld] with
    ``n_vad`` int32 [R] decisions per row, as ``ops.vad`` returns them -> (run_spk, run_f0, run_f1 int32 [cu_cap[R]], n_runs int32 [R],
    status int32 [R]): recording r's runs of one speaker in ascending time at ``cu_cap[r]`` ..; status 1 where they did not fit.
    ``out``: the three run buffers (positions beyond a recording's count keep what they held)."""
    if not (first.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("spk_vote needs its inputs on a HIP device: there is no CPU path")
    opts = check_spk_options(options)
    R = _spk_ragged("spk_vote", cu_win, first, last, label, what="windows")
    S, max_frames, dev = int(S), int(max_frames), first.device
    if first.dtype != I32:
        raise ValueError(f"spk_vote: first, last and label must be int32; got {first.dtype}")
    if not 1 <= S <= SPK_LIMITS["speakers"]:
        raise ValueError(f"spk_vote: {S} speakers, the kernels take 1 to {SPK_LIMITS['speakers']}")
    if not 0 <= max_frames <= SPK_LIMITS["frames"]:
        raise ValueError(f"spk_vote: {max_frames} voting frames are beyond the limit of {SPK_LIMITS['frames']} per recording (2.9 h of 10 ms)")
    for name, t in (("n_frames", n_frames), ("n_vad", n_vad)):
        if t.dtype != I32 or t.shape != (R,) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"spk_vote: {name} must be int32 [{R}] on the windows' device; got {tuple(t.shape)} {t.dtype}")
    if cu_cap.dtype != I32 or cu_cap.shape != (R + 1,) or cu_cap.device != dev:
        raise ValueError(f"spk_vote: cu_cap must be int32 [{R + 1}] on the windows' device")
    if vad.dtype != torch.uint8 or vad.dim() != 2 or vad.shape[0] != R or vad.device != dev or not vad.is_contiguous():
        raise ValueError(f"spk_vote: vad must be contiguous uint8 [{R}, ld] on the windows' device; got {tuple(vad.shape)} {vad.dtype}")
    n_win = first.numel()
    _spk_check_cu("spk_vote", cu_win, n_win, "windows")
    cap = _spk_check_cu("spk_vote", cu_cap, None if capacity is None else int(capacity), "run capacities")[-1]
    # the values the kernels index with: one read-back of four flags
    bad = torch.stack([(first < 0).any(), ((label < 0) | (label >= S)).any(), ((n_frames < 0) | (n_frames > max_frames)).any(),
                       (n_vad > vad.shape[1]).any()]).cpu().tolist()
    if bad[0]:
        raise ValueError("spk_vote: a window starts before 0 (first >= 0 is required: the reference's slice would wrap a negative start "
                         "around the grid, which is not rebuilt)")
    if bad[1]:
        raise ValueError(f"spk_vote: a label lies outside [0, {S}): map the labels to their ranks first")
    if bad[2]:
        raise ValueError(f"spk_vote: n_frames must lie within [0, max_frames = {max_frames}]")
    if bad[3]:
        raise ValueError(f"spk_vote: n_vad exceeds the {vad.shape[1]} decisions a row of vad holds")
    if out is None:
        out = tuple(torch.zeros(cap, device=dev, dtype=I32) for _ in range(3))
    for t in out:
        if t.dtype != I32 or t.dim() != 1 or t.numel() < cap or t.device != dev or not t.is_contiguous():
            raise ValueError(f"spk_vote: the run buffers must be contiguous int32 [>= {cap}] on the windows' device")
    n_runs, status = torch.zeros(R, device=dev, dtype=I32), torch.zeros(R, device=dev, dtype=I32)
    if R == 0:
        return (*out, n_runs, status)
    L = lib()
    ws_bytes = L.ta_spk_post_workspace_bytes(R, S, max_frames, n_win)
    if ws_bytes < 0:
        raise _lib.Ta355Error("ta_spk_post_workspace_bytes refused sizes the Python layer admitted")
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    opt = _lib.SpkPostOptions(*opts)
    check(L.ta_spk_vote_i32(ptr(first), ptr(last), ptr(label), ptr(cu_win), n_win, R, S, ptr(n_frames), max_frames, ptr(vad), vad.shape[1],
                            ptr(n_vad), C.byref(opt), ptr(cu_cap), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(n_runs), ptr(status),
                            ptr(ws), ws_bytes, stream()), "ta_spk_vote_i32")
    return (*out, n_runs, status)


def spk_merge(run_spk, run_f0, run_f1, cu_run, options, out=None, n_run=None):
    """ta_spk_merge_i32: runs (speaker, f0, f1) int32 [sum runs] of R recordings (``cu_run`` int32 [R + 1]), in time order per recording
    -> (seg_spk, seg_f0, seg_f1 int32 [sum runs], n_seg int32 [R]): ``_merge_short_segments`` of every recording, its turns at
    ``cu_run[r]`` ..; positions beyond ``n_seg[r]`` keep what they held (zeros, or the contents of ``out``).  ``n_run`` int32 [R]: only
    the first ``n_run[r]`` positions of recording r's range hold runs (``spk_vote``'s ``n_runs`` beside its ``cu_cap``)."""
    if not (run_spk.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("spk_merge needs its inputs on a HIP device: there is no CPU path")
    opts = check_spk_options(options)
    R = _spk_ragged("spk_merge", cu_run, run_spk, run_f0, run_f1, what="runs")
    if run_spk.dtype != I32:
        raise ValueError(f"spk_merge: the runs must be int32; got {run_spk.dtype}")
    n, dev = run_spk.numel(), run_spk.device
    _spk_check_cu("spk_merge", cu_run, n, "runs")
    if n_run is not None and (n_run.dtype != I32 or n_run.shape != (R,) or n_run.device != dev or not n_run.is_contiguous()):
        raise ValueError(f"spk_merge: n_run must be int32 [{R}] on the runs' device")
    if out is None:
        out = tuple(torch.zeros(n, device=dev, dtype=I32) for _ in range(3))
    for t in out:
        if t.dtype != I32 or t.dim() != 1 or t.numel() < n or t.device != dev or not t.is_contiguous():
            raise ValueError(f"spk_merge: the turn buffers must be contiguous int32 [>= {n}] on the runs' device")
    n_seg = torch.zeros(R, device=dev, dtype=I32)
    if R == 0:
        return (*out, n_seg)
    opt = _lib.SpkPostOptions(*opts)
    check(lib().ta_spk_merge_i32(ptr(run_spk), ptr(run_f0), ptr(run_f1), ptr(cu_run), ptr(n_run), R, C.byref(opt), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                 ptr(n_seg), stream()), "ta_spk_merge_i32")
    return (*out, n_seg)


def spk_words(word_start, word_end, cu_word, seg_start, seg_end, cu_seg, out=None):
    """ta_spk_words_f64: words and segments as float64 seconds, ragged over R recordings (``cu_word``, ``cu_seg`` int32 [R + 1]) ->
    int32 [sum W]: for every word the index (within its recording) of the first segment that contains its midpoint, else of the first
    among the segments whose midpoint is nearest, else -1.  Segments in any order, overlapping allowed."""
    if not (word_start.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("spk_words needs its inputs on a HIP device: there is no CPU path")
    R = _spk_ragged("spk_words", cu_word, word_start, word_end, what="words")
    if _spk_ragged("spk_words", cu_seg, seg_start, seg_end, what="segments") != R:
        raise ValueError(f"spk_words: cu_word stands for {R} recordings and cu_seg for {cu_seg.numel() - 1}")
    if word_start.dtype != F64 or seg_start.dtype != F64 or seg_start.device != word_start.device:
        raise ValueError(f"spk_words: the times must be float64 on one device; got {word_start.dtype} and {seg_start.dtype}")
    n, dev = word_start.numel(), word_start.device
    cw = _spk_check_cu("spk_words", cu_word, n, "words")
    _spk_check_cu("spk_words", cu_seg, seg_start.numel(), "segments")
    finite = torch.stack([torch.isfinite(word_start + word_end).all(), torch.isfinite(seg_start + seg_end).all()]).cpu().tolist()
    if not finite[0]:
        raise ValueError("spk_words: a word's start or end is not finite")
    if not finite[1]:
        raise ValueError("spk_words: a segment's start or end is not finite")
    if out is None:
        out = torch.zeros(n, device=dev, dtype=I32)
    if out.dtype != I32 or out.dim() != 1 or out.numel() < n or out.device != dev or not out.is_contiguous():
        raise ValueError(f"spk_words: out must be contiguous int32 [>= {n}] on the words' device")
    max_words = max((b - a for a, b in zip(cw, cw[1:])), default=0)
    if R == 0 or max_words == 0:
        return out
    check(lib().ta_spk_words_f64(ptr(word_start), ptr(word_end), ptr(cu_word), ptr(seg_start), ptr(seg_end), ptr(cu_seg), R, max_words,
                                 ptr(out), stream()), "ta_spk_words_f64")
    return out


# ----------------------------------------------------------------------------- decoding scores (csrc/generate.hip)
MAX_TOP_LOGPROBS = 8     # the per-lane candidate list of token_scores_kernel


def token_scores(logits, chosen, V, top_k=0):
    """ta_token_scores_f32 on one step of logits a caller holds: ``logits`` f32 [B, ld] (unit column stride, the first ``V`` columns are
    valid and may hold -inf; the rest is never read), ``chosen`` int64 [B] within [0, V) -> (logprob f32 [B] = log softmax(logits[:, :V])
    at ``chosen``, entropy f32 [B], top_ids int64 [B, top_k], top_logprobs f32 [B, top_k]): the ``top_k`` <= 8 most probable tokens in
    descending order, lowest index first on ties, slots beyond the finite entries (-1, -inf).  ``chosen`` is compared with V on the
    host (one synchronisation: this is the convenience form; the decode loop calls the C entry point with device-resident state)."""
    if not (logits.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error("token_scores needs the logits on a HIP device: there is no CPU path")
    if logits.dim() != 2 or logits.dtype != F32 or not (logits.stride(1) == 1 or logits.numel() == 0):
        raise ValueError("token_scores: logits must be f32 [B, ld] with unit column stride")
    B, V, top_k = logits.shape[0], int(V), int(top_k)
    ld = logits.stride(0) if B > 1 else logits.shape[1]
    if not 0 < V <= logits.shape[1]:
        raise ValueError(f"token_scores: V = {V} is outside (0, {logits.shape[1]}]")
    if ld < V:
        raise ValueError("token_scores: logits rows overlap")
    if not 0 <= top_k <= MAX_TOP_LOGPROBS:
        raise ValueError(f"token_scores: top_k = {top_k} is outside [0, {MAX_TOP_LOGPROBS}]")
    if chosen.dtype != torch.int64 or chosen.shape != (B,) or not chosen.is_contiguous() or chosen.device != logits.device:
        raise ValueError(f"token_scores: chosen must be a contiguous int64 [{B}] on the logits' device")
    if B and not bool(((chosen >= 0) & (chosen < V)).all()):
        raise ValueError(f"token_scores: chosen holds an id outside [0, {V})")
    dev = logits.device
    logprob, entropy = torch.empty(B, device=dev, dtype=F32), torch.empty(B, device=dev, dtype=F32)
    top_ids = torch.empty((B, top_k), device=dev, dtype=torch.int64)
    top_lp = torch.empty((B, top_k), device=dev, dtype=F32)
    check(lib().ta_token_scores_f32(ptr(logits), ld, V, B, ptr(chosen), None, None, 1, top_k, ptr(logprob), ptr(entropy),
                                    ptr(top_ids) if top_k else None, ptr(top_lp) if top_k else None, stream()), "ta_token_scores_f32")
    return logprob, entropy, top_ids, top_lp


# ----------------------------------------------------------------------------- decoding options (csrc/generate.hip)
SEQ_BIAS_MAX_SEQS = 4096      # TA_SEQ_BIAS_MAX_SEQS / TA_SEQ_BIAS_MAX_LEN of include/ta355.h
SEQ_BIAS_MAX_LEN = 32


def normalize_sequence_bias(sequence_bias):
    """HF's two forms of ``sequence_bias`` -- {tuple of ids: float} or [[ids, float], ...] -> [(tuple of ids, float)] in HF's order
    (a dict's; the list form becomes a dict first, so a repeated sequence keeps its first place and its last bias).  Raises HF's
    ValueErrors (TF:generation/logits_process.py SequenceBiasLogitsProcessor._validate_arguments)."""
    import numpy as np
    sb = sequence_bias
    if not isinstance(sb, (dict, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    if isinstance(sb, dict):
        if any(not isinstance(k, tuple) for k in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(len(k) == 0 or any(not isinstance(t, (int, np.integer)) or t < 0 for t in k) for k in sb):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
        if any(not isinstance(b, float) for b in sb.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
    else:
        def ok(e):
            return (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], list) and len(e[0]) > 0
                    and all(isinstance(t, (int, np.integer)) and t > 0 for t in e[0]) and isinstance(e[1], float))
        if any(not ok(e) for e in sb):
            raise ValueError("Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, "
                             f"but is {sb}.")
        sb = {tuple(e[0]): e[1] for e in sb}
    return [(tuple(int(t) for t in k), float(b)) for k, b in sb.items()]


def normalize_bad_words(bad_words_ids, eos_ids=()):
    """``bad_words_ids`` -> [(tuple of ids, -inf)] as NoBadWordsLogitsProcessor builds it: HF's ValueErrors, entries that are exactly
    ``[eos]`` dropped, repeated sequences once."""
    import numpy as np
    bw = bad_words_ids
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
    if any(not isinstance(w, list) for w in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
    if any(any(not isinstance(t, (int, np.integer)) or t < 0 for t in w) for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
    eos = [int(e) for e in eos_ids]
    kept = [w for w in bw if all(list(w) != [e] for e in eos)]
    return [(k, float("-inf")) for k in dict.fromkeys(tuple(int(t) for t in w) for w in kept)]


def build_sequence_table(entries, vocab_size, device="cpu", what="sequence_bias"):
    """[(tuple of ids, bias)] in HF's order -> the device table of ``ta_logits_sequence_bias``: dict(tokens i64 [n_tokens], offsets i32
    [n_seq + 1], bias f32 [n_seq], groups i32 [n_groups + 1], n_seq, n_groups, n_tokens), sorted by last token.  Inside a group the
    length-1 entry stands first and the longer ones keep the given order: the order in which HF's f32 bias row receives them.  None for
    an empty list.  ValueError for an id >= vocab_size (HF's wording), an empty sequence, or a table beyond the library's limits."""
    entries = [(tuple(k), float(b)) for k, b in entries]
    if not entries:
        return None
    if any(len(k) == 0 for k, _ in entries):
        raise ValueError(f"{what}: an empty token sequence")
    bad = [t for k, _ in entries for t in k if t >= vocab_size or t < 0]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {bad}")
    if len(entries) > SEQ_BIAS_MAX_SEQS:
        raise ValueError(f"{what}: {len(entries)} sequences exceed the limit of {SEQ_BIAS_MAX_SEQS} (TA_SEQ_BIAS_MAX_SEQS)")
    longest = max(len(k) for k, _ in entries)
    if longest > SEQ_BIAS_MAX_LEN:
        raise ValueError(f"{what}: a sequence of {longest} tokens exceeds the limit of {SEQ_BIAS_MAX_LEN} (TA_SEQ_BIAS_MAX_LEN)")
    order = sorted(range(len(entries)), key=lambda i: (entries[i][0][-1], len(entries[i][0]) != 1, i))
    toks, offs, bias, groups = [], [0], [], []
    for n, i in enumerate(order):
        k, b = entries[i]
        if n == 0 or entries[order[n - 1]][0][-1] != k[-1]:
            groups.append(n)
        toks.extend(k)
        offs.append(len(toks))
        bias.append(b)
    groups.append(len(order))
    return dict(tokens=torch.tensor(toks, dtype=torch.int64, device=device), offsets=torch.tensor(offs, dtype=torch.int32, device=device),
                bias=torch.tensor(bias, dtype=torch.float64).to(F32).to(device), groups=torch.tensor(groups, dtype=torch.int32, device=device),
                n_seq=len(order), n_groups=len(groups) - 1, n_tokens=len(toks))


def decay_multipliers(exponential_decay_length_penalty, max_new):
    """(start, factor) -> (start, f32 [max_new] with m[t] = float32(factor ** (t - start) - 1) for t > start, else 0): the scalar HF's
    ExponentialDecayLengthPenalty multiplies |score[eos]| with, computed by the same Python ``pow`` in float64 and rounded once."""
    start, factor = exponential_decay_length_penalty
    start, factor = int(start), float(factor)
    if start < 0:
        raise ValueError(f"exponential_decay_length_penalty: start_index must be >= 0; got {start}")
    m = torch.zeros(max(int(max_new), 1), dtype=torch.float64)
    for t in range(start + 1, int(max_new)):
        try:
            m[t] = pow(factor, t - start) - 1
        except OverflowError:
            m[t] = float("inf")
    return start, m.to(F32)


def id_list(ids, vocab_size, what):
    """An id or a list of ids -> [int]; ValueError for an id outside [0, vocab_size)."""
    if torch.is_tensor(ids):
        ids = ids.tolist()
    ids = [int(i) for i in (ids if isinstance(ids, (list, tuple)) else [ids])]
    bad = [i for i in ids if not 0 <= i < vocab_size]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but `{what}` holds the token ids {bad}")
    return ids


def check_warp_ext(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """HF's argument checks (MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper) -> the four floats of
    ``ta_logits_warp_ext`` with its "off" values (0, 1, 0, 0) for None."""
    if min_p is not None and not 0 <= float(min_p) <= 1.0:
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    if typical_p is not None and not 0 < float(typical_p) <= 1:      # (1.0 is HF's "off": _get_logits_processor builds no warper for it)
        raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {float(typical_p)}")
    if epsilon_cutoff is not None and not 0 <= float(epsilon_cutoff) < 1:      # (0.0 is HF's "off")
        raise ValueError(f"`epsilon_cutoff` has to be a float > 0 and < 1, but is {float(epsilon_cutoff)}")
    if eta_cutoff is not None and not 0 <= float(eta_cutoff) < 1:
        raise ValueError(f"`eta_cutoff` has to be a float > 0 and < 1, but is {float(eta_cutoff)}")
    return (0.0 if min_p is None else float(min_p), 1.0 if typical_p is None else float(typical_p),
            0.0 if epsilon_cutoff is None else float(epsilon_cutoff), 0.0 if eta_cutoff is None else float(eta_cutoff))


def _logits_rows(logits, V, what):
    if not (logits.is_cuda or _lib.DRY_RUN):
        raise _lib.Ta355Error(f"{what} needs the logits on a HIP device: there is no CPU path")
    if logits.dim() != 2 or logits.dtype != F32 or not (logits.stride(1) == 1 or logits.numel() == 0):
        raise ValueError(f"{what}: logits must be f32 [B, ld] with unit column stride")
    B, V = logits.shape[0], int(V)
    ld = logits.stride(0) if B > 1 else logits.shape[1]
    if not 0 < V <= logits.shape[1]:
        raise ValueError(f"{what}: V = {V} is outside (0, {logits.shape[1]}]")
    if ld < V:
        raise ValueError(f"{what}: logits rows overlap")
    return B, V, ld


def _ids_tensor(ids, V, dev, what):
    return None if not ids else torch.tensor(id_list(ids, V, what), dtype=torch.int64, device=dev)


def logits_sequence_bias(logits, V, context, entries):
    """ta_logits_sequence_bias on logits a caller holds, IN PLACE: ``logits`` f32 [B, ld] (V valid columns), ``context`` int64 [B, n]
    (the ids so far; n may be 0), ``entries`` [(tuple of ids, bias)] in HF's order (``normalize_sequence_bias`` /
    ``normalize_bad_words``), or a table ``build_sequence_table`` made on the logits' device.  -> logits."""
    B, V, ld = _logits_rows(logits, V, "logits_sequence_bias")
    dev = logits.device
    if context.dtype != torch.int64 or context.dim() != 2 or context.shape[0] != B or context.device != dev:
        raise ValueError(f"logits_sequence_bias: context must be int64 [{B}, n] on the logits' device")
    tab = entries if isinstance(entries, dict) else build_sequence_table(entries, V, dev)
    if tab is None:
        return logits
    ctx = context.contiguous()
    n = ctx.shape[1]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().ta_logits_sequence_bias(ptr(logits), ld, V, ptr(ctx) if n else None, n, None, 0, ptr(step), B, ptr(tab["tokens"]),
                                        ptr(tab["offsets"]), ptr(tab["bias"]), ptr(tab["groups"]), tab["n_seq"], tab["n_groups"],
                                        tab["n_tokens"], stream()), "ta_logits_sequence_bias")
    return logits


def logits_step_rules(logits, V, step, max_new, forced_eos_ids=None, eos_ids=None, exponential_decay_length_penalty=None,
                      suppress_tokens=None, begin_suppress_tokens=None):
    """ta_logits_step_rules on logits a caller holds, IN PLACE, for step ``step`` (tokens generated so far) of ``max_new``: HF's
    forced-eos, exponential-decay length penalty (needs ``eos_ids``), suppress and begin-suppress processors, in that order.  -> logits."""
    B, V, ld = _logits_rows(logits, V, "logits_step_rules")
    dev, max_new = logits.device, int(max_new)
    if not 0 <= int(step) < max_new:
        raise ValueError(f"logits_step_rules: step = {step} is outside [0, {max_new})")
    forced, eos = _ids_tensor(forced_eos_ids, V, dev, "forced_eos_token_id"), _ids_tensor(eos_ids, V, dev, "eos_token_id")
    sup, bsup = _ids_tensor(suppress_tokens, V, dev, "suppress_tokens"), _ids_tensor(begin_suppress_tokens, V, dev, "begin_suppress_tokens")
    start, mult = 0, None
    if exponential_decay_length_penalty is not None and eos is not None:
        start, mult = decay_multipliers(exponential_decay_length_penalty, max_new)
        mult = mult.to(dev)
    n = lambda t: 0 if t is None else t.numel()  # noqa: E731
    step_dev = torch.tensor([int(step)], dtype=torch.int32, device=dev)
    check(lib().ta_logits_step_rules(ptr(logits), ld, V, B, ptr(step_dev), max_new, ptr(forced), n(forced), ptr(eos), n(eos), start,
                                     ptr(mult), ptr(sup), n(sup), ptr(bsup), n(bsup), stream()), "ta_logits_step_rules")
    return logits


def logits_warp_ext(logits, V, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """ta_logits_warp_ext on logits a caller holds, IN PLACE: HF's min-p, typical, epsilon and eta warpers in HF's order with
    min_tokens_to_keep = 1 (None = off).  Removed entries become -inf, survivors keep their value.  -> logits."""
    B, V, ld = _logits_rows(logits, V, "logits_warp_ext")
    a = check_warp_ext(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    check(lib().ta_logits_warp_ext(ptr(logits), ld, V, B, *a, stream()), "ta_logits_warp_ext")
    return logits


# ----------------------------------------------------------------------------- beam search (csrc/beam.hip)
MAX_BEAMS = 8             # BM_MAXK / BM_MAXM / BM_MAXEOS of csrc/beam.hip
MAX_BEAM_CANDIDATES = 32
MAX_BEAM_EOS = 3
BEAM_STATE = ("run_seq", "run_score", "parent", "next_ids", "pool_seq", "pool_score", "pool_len", "pool_fin", "heur", "clip_done",
              "step_dev", "slot_dev", "pos", "kmask", "n_unfinished")      # ta_beam_advance's in/out tensors, in argument order


def beam_length_divisors(length_penalty, max_new):
    """f32 [max_new] with d[n - 1] = float32(float(n) ** length_penalty): the divisors HF's _update_finished_beams and
    _check_early_stop_heuristic form as Python floats (``(cur_len + 1 - decoder_prompt_len) ** length_penalty``), by the same ``pow``."""
    d = torch.ones(max(int(max_new), 1), dtype=torch.float64)
    for n in range(1, int(max_new) + 1):
        try:
            d[n - 1] = float(n) ** float(length_penalty)
        except OverflowError:
            d[n - 1] = float("inf")
    return d.to(F32)


def beam_candidates(num_beams, n_eos):
    """M = max(2, 1 + n_eos) * num_beams (``beams_to_keep`` of HF's _beam_search); ValueError outside the library's envelope."""
    K, n_eos = int(num_beams), int(n_eos)
    if not 1 <= K <= MAX_BEAMS:
        raise ValueError(f"num_beams = {K} is outside [1, {MAX_BEAMS}]")
    if not 0 <= n_eos <= MAX_BEAM_EOS:
        raise ValueError(f"{n_eos} eos ids: beam search takes at most {MAX_BEAM_EOS}")
    return max(2, 1 + n_eos) * K


def beam_logprobs(logits, V):
    """ta_beam_logprobs_f32: log_softmax over the first ``V`` columns of f32 ``logits`` [R, ld], IN PLACE (-inf stays -inf, columns
    >= V untouched).  -> logits."""
    R, V, ld = _logits_rows(logits, V, "beam_logprobs")
    check(lib().ta_beam_logprobs_f32(ptr(logits), ld, V, R, stream()), "ta_beam_logprobs_f32")
    return logits


def beam_topk(rows, V, score, M):
    """ta_beam_topk_f32: ``rows`` f32 [B * K, ld] (V valid columns), ``score`` f32 [B, K] -> (cand_score f32 [B, M], cand_flat i32
    [B, M]): per clip the M largest of float32(rows[b * K + k, v] + score[b, k]), descending, lowest flat index k * V + v on ties."""
    R, V, ld = _logits_rows(rows, V, "beam_topk")
    if score.dim() != 2 or score.dtype != F32 or not score.is_contiguous() or score.device != rows.device or score.numel() != R:
        raise ValueError(f"beam_topk: score must be a contiguous f32 [B, K] with B * K = {R} on the rows' device")
    B, K, M = score.shape[0], score.shape[1], int(M)
    if not 1 <= K <= MAX_BEAMS or not 1 <= M <= min(MAX_BEAM_CANDIDATES, K * V):
        raise ValueError(f"beam_topk: K = {K} must be within [1, {MAX_BEAMS}] and M = {M} within [1, {min(MAX_BEAM_CANDIDATES, K * V)}]")
    dev = rows.device
    cs, cf = torch.empty((B, M), device=dev, dtype=F32), torch.empty((B, M), device=dev, dtype=torch.int32)
    nb = lib().ta_beam_topk_workspace_bytes(B, K, V, M)
    ws = torch.empty(max(nb, 8), device=dev, dtype=torch.uint8)
    check(lib().ta_beam_topk_f32(ptr(rows), ld, V, ptr(score), B, K, M, ptr(cs), ptr(cf), ptr(ws), ws.numel(), stream()), "ta_beam_topk_f32")
    return cs, cf


def beam_advance(cand_score, cand_flat, V, eos_ids, pad_id, len_div, early_stopping, length_penalty, state, trace=None):
    """ta_beam_advance: one step of HF's beam bookkeeping on device state.  ``cand_score`` f32 / ``cand_flat`` i32 [B, M] from
    ``beam_topk``; ``len_div`` = ``beam_length_divisors(length_penalty, max_new)`` on the device; ``early_stopping`` False / True /
    "never"; ``state``: dict of the ``BEAM_STATE`` tensors (updated IN PLACE; shapes in include/ta355.h); ``trace``: None or a dict with
    cand_score, cand_flat, run_seq, run_score, parent buffers [max_new, ...].  -> state."""
    if cand_score.dim() != 2 or cand_score.dtype != F32 or cand_flat.dtype != torch.int32 or cand_flat.shape != cand_score.shape:
        raise ValueError("beam_advance: cand_score f32 [B, M] and cand_flat i32 [B, M] are required")
    missing = [k for k in BEAM_STATE if k not in state]
    if missing:
        raise ValueError(f"beam_advance: state lacks {missing}")
    B, M = cand_score.shape
    R, max_new = state["run_seq"].shape
    K = R // max(B, 1)
    eos_ids = [int(e) for e in eos_ids]
    if K * B != R or beam_candidates(K, len(eos_ids)) != M:
        raise ValueError(f"beam_advance: {R} rows, {B} clips and {len(eos_ids)} eos ids do not give M = {M} candidates")
    if early_stopping not in (False, True, "never"):
        raise ValueError(f"early_stopping must be False, True or 'never'; got {early_stopping!r}")
    if K * max_new > 12288:
        raise ValueError(f"beam_advance: num_beams * max_new = {K * max_new} exceeds 12288")
    if len_div.dtype != F32 or len_div.numel() != max_new:
        raise ValueError(f"beam_advance: len_div must be f32 [{max_new}]")
    for k, dt in (("run_seq", torch.int64), ("next_ids", torch.int64), ("pool_seq", torch.int64), ("run_score", F32), ("pool_score", F32)):
        if state[k].dtype != dt or not state[k].is_contiguous():
            raise ValueError(f"beam_advance: state[{k!r}] must be a contiguous {dt} tensor")
    for k in BEAM_STATE:
        if k not in ("run_seq", "next_ids", "pool_seq", "run_score", "pool_score") and (state[k].dtype != torch.int32 or not state[k].is_contiguous()):
            raise ValueError(f"beam_advance: state[{k!r}] must be a contiguous int32 tensor")
    if state["kmask"].dim() != 2 or state["kmask"].shape[0] != R or state["pos"].numel() != R or state["pool_seq"].numel() != R * max_new:
        raise ValueError("beam_advance: pos [R], kmask [R, Lmax] and pool_seq [B, K, max_new] are required")
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    dev = cand_score.device
    eos = torch.tensor(eos_ids or [-1], dtype=torch.int64, device=dev)
    tr = [None] * 5 if trace is None else [ptr(trace[k]) for k in ("cand_score", "cand_flat", "run_seq", "run_score", "parent")]
    s = state
    check(lib().ta_beam_advance(ptr(cand_score.contiguous()), ptr(cand_flat.contiguous()), B, K, M, int(V), ptr(eos), len(eos_ids), int(pad_id),
                                max_new, ptr(len_div), es, int(es == 2 and float(length_penalty) > 0.0), ptr(s["run_seq"]), ptr(s["run_score"]),
                                ptr(s["parent"]), ptr(s["next_ids"]), ptr(s["pool_seq"]), ptr(s["pool_score"]), ptr(s["pool_len"]),
                                ptr(s["pool_fin"]), ptr(s["heur"]), ptr(s["clip_done"]), ptr(s["step_dev"]), ptr(s["slot_dev"]), ptr(s["pos"]),
                                ptr(s["kmask"]), s["kmask"].shape[1], ptr(s["n_unfinished"]), *tr, stream()), "ta_beam_advance")
    return state


def _beam_cache(t, what):
    if t.dim() != 5 or t.dtype != BF16 or not t.is_contiguous() or t.shape[4] % 8:
        raise ValueError(f"{what}: caches must be contiguous bf16 [layers, rows, kv_heads, slots, head_dim] with head_dim a multiple of 8")
    return t.shape


def kv_beam_expand(ksrc, vsrc, num_beams, Lmax, L=None):
    """ta_kv_beam_expand: the B-row prompt caches [layers, B, kv_heads, Lsrc, head_dim] -> new caches [layers, B * K, kv_heads, Lmax,
    head_dim] whose rows b * K .. b * K + K - 1 hold slots [0, L) of clip b (L defaults to Lsrc; the other slots are uninitialised)."""
    nl, B, hkv, Ls, hd = _beam_cache(ksrc, "kv_beam_expand")
    K, L = int(num_beams), int(Ls if L is None else L)
    if vsrc.shape != ksrc.shape or vsrc.dtype != BF16 or not vsrc.is_contiguous() or not 1 <= K <= MAX_BEAMS or not 0 <= L <= min(Ls, int(Lmax)):
        raise ValueError("kv_beam_expand: the two caches must agree, 1 <= num_beams <= 8 and L <= min(Lsrc, Lmax)")
    kd, vd = (torch.empty((nl, B * K, hkv, int(Lmax), hd), dtype=BF16, device=ksrc.device) for _ in range(2))
    check(lib().ta_kv_beam_expand(ptr(ksrc), ptr(vsrc), ptr(kd), ptr(vd), nl, B, K, hkv, L, Ls, int(Lmax), hd, stream()), "ta_kv_beam_expand")
    return kd, vd


def kv_beam_reorder(kcache, vcache, num_beams, L, max_new, parent, slot_dev):
    """ta_kv_beam_reorder, IN PLACE: slots [L, *slot_dev) of row b * K + j of both caches take those of row b * K + parent[b * K + j]
    (``parent`` i32 [R], ``slot_dev`` i32 [1], both on the device).  -> (kcache, vcache)."""
    nl, R, hkv, Lmax, hd = _beam_cache(kcache, "kv_beam_reorder")
    K, L, max_new = int(num_beams), int(L), int(max_new)
    if vcache.shape != kcache.shape or vcache.dtype != BF16 or not vcache.is_contiguous() or not 1 <= K <= MAX_BEAMS or R % K:
        raise ValueError("kv_beam_reorder: the two caches must agree and hold a multiple of num_beams (1..8) rows")
    if L < 0 or max_new < 0 or L + max_new > Lmax:
        raise ValueError(f"kv_beam_reorder: L + max_new = {L + max_new} exceeds the cache's {Lmax} slots")
    if parent.dtype != torch.int32 or parent.numel() != R or not parent.is_contiguous() or slot_dev.dtype != torch.int32 or slot_dev.numel() != 1:
        raise ValueError(f"kv_beam_reorder: parent must be a contiguous int32 [{R}] and slot_dev an int32 [1]")
    check(lib().ta_kv_beam_reorder(ptr(kcache), ptr(vcache), nl, R // K, K, hkv, L, Lmax, hd, max_new, ptr(parent), ptr(slot_dev), stream()),
          "ta_kv_beam_reorder")
    return kcache, vcache


# ----------------------------------------------------------------------------- wav2vec2 acoustic model (csrc/wav2vec2.hip)
def w2v_conv0_gn_gelu(wav, lens, w, gn_w, gn_b, eps=1e-5, out=None, out_rpb=None):
    """ta_w2v_conv0_gn_gelu: conv layer 0 (k 10, stride 5) + per-channel GroupNorm over each clip's own frames + exact GELU.
    ``wav`` f32 [B, Ls], ``lens`` int32 [B] on the device, ``w`` f32 [C, 10] -> bf16 [B, out_rpb, C] time-major; clip b's rows
    t >= (lens[b] - 10) // 5 + 1 are not written (``out``: a tensor to write into)."""
    _req(wav, F32), _req(w, F32), _req(gn_w, F32), _req(gn_b, F32)
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.device == wav.device
    B, Ls = wav.shape
    Cd = w.shape[0]
    assert w.shape == (Cd, 10) and gn_w.shape == (Cd,) and gn_b.shape == (Cd,) and lens.shape == (B,)
    T0 = (Ls - 10) // 5 + 1
    rpb = T0 if out_rpb is None else int(out_rpb)
    if out is None:
        out = torch.empty((B, rpb, Cd), device=wav.device, dtype=BF16)
    assert out.dtype == BF16 and out.is_contiguous() and out.numel() >= B * rpb * Cd
    n = lib().ta_w2v_conv0_ws_bytes(B, Ls, Cd)
    ws = torch.empty(max(n, 8), device=wav.device, dtype=torch.uint8)
    check(lib().ta_w2v_conv0_gn_gelu(ptr(wav), ptr(lens), B, Ls, ptr(w), ptr(gn_w), ptr(gn_b), Cd, float(eps), ptr(out), rpb, ptr(ws),
                                     ws.numel(), stream()), "ta_w2v_conv0_gn_gelu")
    return out


def w2v_pos_conv(x, wp, bias, cu_rows, max_rows, out=None):
    """ta_w2v_pos_conv: y = x + gelu(grouped positional conv(x) + bias) per clip.  ``x`` bf16 or f32 [rows, H] (the stream's dtype),
    ``wp`` the packed bf16 image (``wav2vec2.pack_pos_conv``), ``cu_rows`` int32 [B + 1] on the device -> y like x."""
    assert x.dtype in (BF16, F32)
    _req(x), _req(wp, BF16), _req(bias, F32)
    assert cu_rows.dtype == torch.int32 and cu_rows.is_contiguous() and cu_rows.device == x.device
    H = x.shape[1]
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == x.dtype and out.shape == x.shape and out.is_contiguous() and out.data_ptr() != x.data_ptr()
    check(lib().ta_w2v_pos_conv(ptr(x), int(x.dtype == F32), ptr(wp), ptr(bias), ptr(out), ptr(cu_rows), cu_rows.numel() - 1,
                                int(max_rows), H, stream()), "ta_w2v_pos_conv")
    return out


def w2v_head_logsoftmax(logits, bias, n_classes, out=None):
    """ta_w2v_head_logsoftmax: log_softmax(logits[:, :n_classes] + bias) -> f32 [rows, n_classes]; logits f32 [rows, ld]."""
    _req(logits, F32), _req(bias, F32)
    rows, ld = logits.shape
    if out is None:
        out = torch.empty((rows, int(n_classes)), device=logits.device, dtype=F32)
    assert out.dtype == F32 and out.is_contiguous() and out.numel() >= rows * int(n_classes)
    check(lib().ta_w2v_head_logsoftmax(ptr(logits), ld, ptr(bias), int(n_classes), ptr(out), rows, stream()), "ta_w2v_head_logsoftmax")
    return out


def w2v_input_norm(wav, lens, eps, out=None):
    """ta_w2v_input_norm: out[b, i] = (wav[b, i] - mean_b) / sqrt(var_b + eps) over each clip's own first ``lens[b]`` samples (biased
    variance; 1e-7: transformers' ``zero_mean_unit_var_norm``, 1e-5: torchaudio's ``layer_norm(waveform, waveform.shape)``).
    ``wav`` f32 [B, Ls], ``lens`` int32 [B] on the device -> f32 [B, Ls]; samples behind a clip's end are not written."""
    _req(wav, F32)
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.device == wav.device
    B, Ls = wav.shape
    assert lens.shape == (B,)
    if out is None:
        out = torch.empty_like(wav)
    assert out.dtype == F32 and out.is_contiguous() and out.shape == wav.shape
    ws = torch.empty(max(lib().ta_w2v_input_norm_ws_bytes(B, Ls), 8), device=wav.device, dtype=torch.uint8)
    check(lib().ta_w2v_input_norm(ptr(wav), ptr(lens), B, Ls, float(eps), ptr(out), ptr(ws), ws.numel(), stream()), "ta_w2v_input_norm")
    return out


def w2v_conv0_ln_gelu(wav, lens, w, bias, ln_w, ln_b, eps=1e-5, out=None, out_rpb=None):
    """ta_w2v_conv0_ln_gelu: conv layer 0 (k 10, stride 5) + bias + LayerNorm over each frame's channels + exact GELU in one kernel.
    ``wav`` f32 [B, Ls], ``lens`` int32 [B] on the device, ``w`` f32 [C, 10], C in {64, 128, 256, 512} -> bf16 [B, out_rpb, C]
    time-major; clip b's rows t >= (lens[b] - 10) // 5 + 1 are not written (``out``: a tensor to write into)."""
    _req(wav, F32), _req(w, F32), _req(bias, F32), _req(ln_w, F32), _req(ln_b, F32)
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.device == wav.device
    B, Ls = wav.shape
    Cd = w.shape[0]
    assert w.shape == (Cd, 10) and bias.shape == (Cd,) and ln_w.shape == (Cd,) and ln_b.shape == (Cd,) and lens.shape == (B,)
    T0 = (Ls - 10) // 5 + 1
    rpb = T0 if out_rpb is None else int(out_rpb)
    if out is None:
        out = torch.empty((B, rpb, Cd), device=wav.device, dtype=BF16)
    assert out.dtype == BF16 and out.is_contiguous() and out.numel() >= B * rpb * Cd
    check(lib().ta_w2v_conv0_ln_gelu(ptr(wav), ptr(lens), B, Ls, ptr(w), ptr(bias), ptr(ln_w), ptr(ln_b), Cd, float(eps), ptr(out), rpb,
                                     stream()), "ta_w2v_conv0_ln_gelu")
    return out


def layernorm_gelu(x, w, b, eps=1e-5, out=None):
    """ta_layernorm_gelu_bf16: gelu(LayerNorm(x)) row by row, bf16 [M, H] -> bf16 [M, H] (the LayerNorm kernels with GELU as their
    output activation: wav2vec2's LayerNorm conv layers 1 .. 6)."""
    _req(x, BF16), _req(w, F32), _req(b, F32)
    M, H = x.shape
    assert w.shape == (H,) and b.shape == (H,)
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == BF16 and out.is_contiguous() and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    check(lib().ta_layernorm_gelu_bf16(ptr(x), ptr(w), ptr(b), ptr(out), M, H, float(eps), stream()), "ta_layernorm_gelu_bf16")
    return out


# ----------------------------------------------------------------------------- ECAPA-TDNN kernels (csrc/ecapa.hip)
def ecapa_fbank(audio, starts, lens, window_samples, tables):
    """ta_ecapa_fbank: ``audio`` f32 [n], ``starts`` / ``lens`` int32 [N] on the device, ``tables`` = (window, twiddle, mel, ranges)
    device tensors (``ecapa.fbank_tables``) -> (feat f32 [N, T, 80], slab bf16 [N, T + 4, 128]), T = window_samples // 160 + 1."""
    _req(audio, F32)
    win, tw, mel, rng = tables
    _req(win, F32), _req(tw, F32), _req(mel, F32), _req(rng, torch.int32), _req(starts, torch.int32), _req(lens, torch.int32)
    N, T = starts.numel(), int(window_samples) // 160 + 1
    feat = torch.empty((N, T, 80), device=audio.device, dtype=F32)
    slab = torch.empty((N, T + 4, 128), device=audio.device, dtype=BF16)
    check(lib().ta_ecapa_fbank(ptr(audio), audio.numel(), ptr(starts), ptr(lens), N, int(window_samples), ptr(win), ptr(tw), ptr(mel),
                               ptr(rng), ptr(feat), ptr(slab), stream()), "ta_ecapa_fbank")
    return feat, slab


def ecapa_res2net(z1, bn1_s, bn1_t, res_w, res_b, res_s, res_t, T, w, dilation, out):
    """ta_ecapa_res2net: ``z1`` bf16 [N, z_rpw, ldz] (tdnn1's pre-activation rows, window n's frames at rows 0 .. T - 1 of slab n),
    ``res_w`` the packed image (``ecapa.pack_res2net``) -> ``out`` bf16 [N, y_rpw, ldy], columns 0 .. 8 w of rows 0 .. T - 1 written."""
    _req(z1, BF16), _req(out, BF16), _req(res_w, BF16)
    for t in (bn1_s, bn1_t, res_b, res_s, res_t):
        _req(t, F32)
    N, z_rpw, ldz = z1.shape
    assert out.shape[0] == N
    check(lib().ta_ecapa_res2net(ptr(z1), ldz, z_rpw, ptr(bn1_s), ptr(bn1_t), ptr(res_w), ptr(res_b), ptr(res_s), ptr(res_t), ptr(out),
                                 out.shape[2], out.shape[1], N, int(T), int(w), int(dilation), stream()), "ta_ecapa_res2net")
    return out


def ecapa_relu_bn(z, scale, shift, N, T, want_stats=False):
    """ta_ecapa_relu_bn: ``z`` bf16 [N T, Cw] -> bf16 [N T, Cw] (and with ``want_stats`` the f32 and bf16 [N, 2 Cw] mean | std)."""
    _req(z, BF16), _req(scale, F32), _req(shift, F32)
    Cw = z.shape[1]
    out = torch.empty_like(z)
    sf = torch.empty((N, 2 * Cw), device=z.device, dtype=F32) if want_stats else None
    sb = torch.empty((N, 2 * Cw), device=z.device, dtype=BF16) if want_stats else None
    check(lib().ta_ecapa_relu_bn(ptr(z), ptr(scale), ptr(shift), ptr(out), ptr(sf), ptr(sb), int(N), int(T), Cw, stream()), "ta_ecapa_relu_bn")
    return (out, sf, sb) if want_stats else out


def ecapa_se_residual(z2, bn2_s, bn2_t, se_w1t, se_b1, se_w2t, se_b2, residual, out, col0, N, T):
    """ta_ecapa_se_residual: ``z2`` bf16 [N T, Cw], ``residual`` bf16 [N T, ldres] (its first Cw columns) -> columns
    col0 .. col0 + Cw of ``out`` bf16 [N T, ldout]; -> (out, window means f32 [N, Cw], gates f32 [N, Cw])."""
    _req(z2, BF16), _req(residual, BF16), _req(out, BF16)
    for t in (bn2_s, bn2_t, se_w1t, se_b1, se_w2t, se_b2):
        _req(t, F32)
    Cw, se = z2.shape[1], se_b1.numel()
    assert col0 % 2 == 0 and col0 + Cw <= out.shape[1] and se_w1t.shape == (Cw, se) and se_w2t.shape == (se, Cw)
    ws = torch.empty(max(lib().ta_ecapa_se_ws_floats(int(N), Cw), 1), device=z2.device, dtype=F32)
    check(lib().ta_ecapa_se_residual(ptr(z2), ptr(bn2_s), ptr(bn2_t), ptr(se_w1t), ptr(se_b1), ptr(se_w2t), ptr(se_b2), ptr(residual),
                                     residual.shape[1], C.c_void_p(out.data_ptr() + 2 * col0), out.shape[1], int(N), int(T), Cw, se, ptr(ws),
                                     stream()), "ta_ecapa_se_residual")
    return out, ws[:N * Cw].reshape(N, Cw), ws[N * Cw:2 * N * Cw].reshape(N, Cw)


def ecapa_attn_act(g, per_window, scale, shift, N, T):
    """ta_ecapa_attn_act: ``g`` f32 [N T, A], ``per_window`` f32 [N, A] -> bf16 [N T, A]."""
    for t in (g, per_window, scale, shift):
        _req(t, F32)
    out = torch.empty(g.shape, device=g.device, dtype=BF16)
    check(lib().ta_ecapa_attn_act(ptr(g), ptr(per_window), ptr(scale), ptr(shift), ptr(out), int(N), int(T), g.shape[1], stream()),
          "ta_ecapa_attn_act")
    return out


def ecapa_asp_pool(logits, h, aspbn_s, aspbn_t, N, T):
    """ta_ecapa_asp_pool: ``logits`` f32 [N T, Cw], ``h`` bf16 [N T, Cw] -> (out bf16 [N, 2 Cw], attention weights f32 [N T, Cw],
    pooled f32 [N, 2 Cw] before asp_bn)."""
    _req(logits, F32), _req(h, BF16), _req(aspbn_s, F32), _req(aspbn_t, F32)
    Cw = logits.shape[1]
    out = torch.empty((N, 2 * Cw), device=h.device, dtype=BF16)
    aw = torch.empty_like(logits)
    pooled = torch.empty((N, 2 * Cw), device=h.device, dtype=F32)
    check(lib().ta_ecapa_asp_pool(ptr(logits), ptr(h), ptr(aspbn_s), ptr(aspbn_t), ptr(out), ptr(aw), ptr(pooled), int(N), int(T), Cw,
                                  stream()), "ta_ecapa_asp_pool")
    return out, aw, pooled


# ----------------------------------------------------------------------------- speaker clustering kernels (csrc/cluster.hip)
SPK_MIN_N, SPK_MAX_N, SPK_MAX_D, SPK_MAX_P, SPK_MAX_COLS = 6, 32768, 256, 32, 1024


def _mat(t):
    """A 2-D f32 matrix with unit column stride (a column slice of a wider one is fine) -> its leading dimension."""
    assert (t.is_cuda or _lib.DRY_RUN) and t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1], \
        "ta355 spk ops need 2-D f32 CUDA(HIP) tensors with contiguous rows"
    return t.stride(0)


def _ws(n, like):
    return torch.empty(max(int(n), 1), device=like.device, dtype=F32)


def spk_keep(n: int, pval: float) -> int:
    """Entries a row of the affinity keeps: the reference's ``int(max(pval, 6 / n) * n)``, at least 1 (tiny_audio/diarization.py:63-66)."""
    return max(1, int(max(pval, 6.0 / n) * n))


def spk_affinity(E, keep, *, out=None, deg=None, want_kept=False, phases=7):
    """ta_spk_affinity_f32: ``E`` f32 [N, D] -> (W f32 [N, N]: pruned, symmetrised cosine affinity with a zero diagonal; deg f32 [N]: its
    row sums; the survivors per row before symmetrisation int32 [N], or None).  ``out``: a [N, N] matrix (or column slice) to write;
    by default its rows are padded to a multiple of 4 floats, which is what lets ``spk_laplacian_matmul`` read 16 bytes per lane.
    ``phases``: 1 cosine, 2 pruning, 4 symmetrisation and degrees (each needs the ones before it to have run on ``out``)."""
    _req(E, F32)
    N, D = E.shape
    if N > SPK_MAX_N:
        raise ValueError(f"speaker clustering on the device takes at most {SPK_MAX_N} windows, got {N}")
    if out is None:
        out = torch.empty((N, (N + 3) // 4 * 4), device=E.device, dtype=F32)[:, :N]
    ld = _mat(out)
    assert out.shape == (N, N)
    deg = torch.empty(N, device=E.device, dtype=F32) if deg is None else _req(deg, F32)
    kept = torch.empty(N, device=E.device, dtype=torch.int32) if want_kept else None
    ws = _ws(lib().ta_spk_affinity_ws_floats(N, D), E)
    check(lib().ta_spk_affinity_f32(ptr(E), N, D, int(keep), ptr(out), ld, ptr(deg), ptr(kept), ptr(ws), int(phases), stream()),
          "ta_spk_affinity_f32")
    return out, deg, kept


def spk_laplacian_matmul(W, deg, X, *, out=None):
    """ta_spk_laplacian_matmul_f32: Y [N, p] = diag(deg) X - W X for ``X`` f32 [N, p <= 32]."""
    ldw, ldx = _mat(W), _mat(X)
    _req(deg, F32)
    N, p = X.shape
    assert W.shape == (N, N) and deg.numel() == N
    out = torch.empty((N, p), device=X.device, dtype=F32) if out is None else out
    ldy = _mat(out)
    assert out.shape == (N, p)
    ws = _ws(lib().ta_spk_lapmul_ws_floats(N, p), X)
    check(lib().ta_spk_laplacian_matmul_f32(ptr(W), ldw, ptr(deg), ptr(X), ldx, ptr(out), ldy, N, p, ptr(ws), stream()),
          "ta_spk_laplacian_matmul_f32")
    return out


def spk_panel_gram(A, B, *, out=None):
    """ta_spk_panel_gram_f32: C [a, b] = A^T B for ``A`` [N, a], ``B`` [N, b]."""
    lda, ldb = _mat(A), _mat(B)
    (N, a), b = A.shape, B.shape[1]
    assert B.shape[0] == N
    out = torch.empty((a, b), device=A.device, dtype=F32) if out is None else out
    ldc = _mat(out)
    assert out.shape == (a, b)
    ws = _ws(lib().ta_spk_gram_ws_floats(N, a, b), A)
    check(lib().ta_spk_panel_gram_f32(ptr(A), lda, a, ptr(B), ldb, b, N, ptr(out), ldc, ptr(ws), stream()), "ta_spk_panel_gram_f32")
    return out


def spk_panel_update(B, A, C):
    """ta_spk_panel_update_f32: ``B`` [N, b <= 32] -= ``A`` [N, a] ``C`` [a, b], in place.  -> B."""
    ldb, lda, ldc = _mat(B), _mat(A), _mat(C)
    (N, b), a = B.shape, A.shape[1]
    assert A.shape[0] == N and C.shape == (a, b)
    check(lib().ta_spk_panel_update_f32(ptr(B), ldb, b, ptr(A), lda, a, ptr(C), ldc, N, stream()), "ta_spk_panel_update_f32")
    return B


def spk_panel_combine(V, Z, *, out=None):
    """ta_spk_panel_combine_f32: Y [N, m <= 32] = ``V`` [N, c] ``Z`` [c, m]."""
    ldv, ldz = _mat(V), _mat(Z)
    (N, c), m = V.shape, Z.shape[1]
    assert Z.shape[0] == c
    out = torch.empty((N, m), device=V.device, dtype=F32) if out is None else out
    ldy = _mat(out)
    assert out.shape == (N, m)
    check(lib().ta_spk_panel_combine_f32(ptr(V), ldv, c, ptr(Z), ldz, m, ptr(out), ldy, N, stream()), "ta_spk_panel_combine_f32")
    return out

"""CPU float64 reference of the LM attention block that ``csrc/attention.hip`` and ``csrc/qkv_post.hip`` implement, and the per-row
metric the attention tests gate on.  A plain module (no fixtures): ``tests/test_attention_ref.py`` checks it on the host,
``tests/test_gpu_attention_grid.py`` compares every attention entry point of the library with it.

The operation, from the bf16 bits of ``qkv0 [B*L, (Hq + 2 Hkv) * 128]`` (the q | k | v GEMM output, token-major):
  per-head RMSNorm (eps 1e-6, weights qn_w / kn_w) or none -> RoPE in the rotate-half form with table row pos[b, l] or none ->
  scores * hd^-0.5 -> visibility  k <= q  and  kmask[b, k] != 0  and (packed rows) the same non-zero segment id -> softmax, rows
  with no visible key set to 0 -> P V with the GQA repeat.
Visibility is derived from ``segment_ids`` here, never from the library's ta_segment_table.

Two forms of the same function:
  exact           no intermediate rounding; the backward is torch autograd in float64 through ``forward``.
  rounding model  (``rounded=True``) rounds to bf16 (round to nearest even) exactly where the kernels do and nowhere else; its
                  backward (``backward_model``) restates the kernels' formulas by hand, because they recompute P from the saved
                  LSE and take Delta from the rounded O.  With ``rounded=False`` the same hand-written backward must equal autograd
                  (tests/test_attention_ref.py), which is what ties the two forms together.

Rounding points of the kernels (file:line of the instruction that rounds), all modelled below:
  R1  Q after norm / RoPE -> bf16         attention.hip:657-658 (fused forward, query fragments = the stored Q), qkv_post.hip:164
  R2  K after norm / RoPE -> bf16         attention.hip:574 (fused forward, in place in LDS and to Ko), qkv_post.hip:164
  R3  P~ = exp(s - rowmax) -> bf16        attention.hip:269 (pv_accumulate, every forward kernel): ``pack_p`` before P V.  The softmax
      denominator is accumulated by the SAME MFMA from a row of ones (:313, :590), so  l = sum_k bf16(P~)  -- the rounded values.
  R4  O = (sum_k bf16(P~) V) / l -> bf16  attention.hip:413-414 (tiled), :730-731 (fused)
      LSE = rowmax * scale + log(l), f32   attention.hip:417, :736 (1e30 on rows with no visible key)
  R5  backward: P = exp(s * scale - LSE) with the stored f32 LSE; dS = P (dP - Delta) scale; P and dS -> bf16 before the products
      dV += P^T dO, dK += dS^T Q, dQ += dS K      attention.hip:949 (dQ body), :1090-1091 (dK / dV body)
      Delta = rowsum(dO o O) over the bf16 O, f32  qkv_post.hip attn_bwd_prep_kernel
  R6  un-fused backward: dQ / dK / dV -> bf16    attention.hip:977 (dQ), :1126-1128 (dK, dV); ta_lm_qkv_post_bwd then works from
      those bf16 values and rounds d(qkv0) once more (qkv_post.hip, lm_qkv_post_bwd_kernel)
  R7  fused backward: RoPE^T and the RMSNorm backward run on the f32 accumulators, d(qkv0) -> bf16   attention.hip:845-846
rq / rk are f32.  Everything between two rounding points is f32 in the kernels and float64 here: fp32 accumulation contributes
~2^-24 * L, far below bf16's 2^-9.
"""
import torch

F64 = torch.float64
HD = 128
EPS = 1e-6


def rb(x):
    """Round to bf16 (nearest even), returned in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def rf(x):
    """Round to f32, returned in float64."""
    return x.to(torch.float32).to(F64)


def rope_tables(n, theta=1e6, hd=HD):
    """cos / sin f32 [n, hd / 2]: the table layout the library reads."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    f = torch.arange(n, dtype=torch.float32)[:, None] * inv[None]
    return f.cos().contiguous(), f.sin().contiguous()


def rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def visibility(B, L, kmask=None, segment_ids=None, causal=True):
    """bool [B, L(q), L(k)]:  k <= q (unless ``causal`` is off),  kmask[b, k] != 0,  and for packed rows the same non-zero segment id."""
    idx = torch.arange(L)
    vis = (idx[None, :] <= idx[:, None])[None].expand(B, L, L).clone() if causal else torch.ones(B, L, L, dtype=torch.bool)
    if kmask is not None:
        vis &= (kmask.cpu() != 0)[:, None, :]
    if segment_ids is not None:
        sid = segment_ids.cpu().long()
        vis &= (sid[:, :, None] == sid[:, None, :]) & (sid[:, :, None] != 0) & (sid[:, None, :] != 0)
    return vis


def segment_positions(segment_ids):
    """int32 [B, L]: positions restarting at 0 in every segment (0 on padding) -- what a packed batch passes as ``pos``."""
    sid = segment_ids.cpu().long()
    B, L = sid.shape
    pos = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        run = 0
        for l in range(L):
            run = run + 1 if (l > 0 and sid[b, l] == sid[b, l - 1] and sid[b, l] != 0) else 0
            pos[b, l] = run
    return pos.to(torch.int32)


def left_pad_positions(kmask):
    """HF's positions under left padding: cumsum(mask) - 1 clipped at 0."""
    return (kmask.cpu().long().cumsum(-1) - 1).clamp(min=0).to(torch.int32)


def qk_post(x, B, L, Hq, Hkv, qn_w=None, kn_w=None, cos=None, sin=None, pos=None, pos_q=None):
    """x: float64 [B*L, (Hq + 2 Hkv) * HD] -> q [B,Hq,L,HD], k, v [B,Hkv,L,HD], rq [B*L,Hq] / rk [B*L,Hkv] (None without the norm).
    ``pos_q``: positions for the query side only (test instrumentation: a one-sided table-row error)."""
    xs = x.reshape(B, L, Hq + 2 * Hkv, HD)
    q, k, v = xs[:, :, :Hq], xs[:, :, Hq:Hq + Hkv], xs[:, :, Hq + Hkv:]
    rq = rk = None
    if qn_w is not None:
        rq = torch.rsqrt((q * q).mean(-1, keepdim=True) + EPS)
        rk = torch.rsqrt((k * k).mean(-1, keepdim=True) + EPS)
        q, k = qn_w.to(F64) * (q * rq), kn_w.to(F64) * (k * rk)
        rq, rk = rq.reshape(B * L, Hq), rk.reshape(B * L, Hkv)
    if cos is not None:
        def table(p):
            p = torch.arange(L)[None].expand(B, L) if p is None else p.cpu().long().reshape(B, L)
            c, s = cos.cpu().to(F64)[p], sin.cpu().to(F64)[p]                       # [B, L, HD / 2]
            return torch.cat([c, c], -1)[:, :, None], torch.cat([s, s], -1)[:, :, None]
        ck, sk = table(pos)
        cq, sq = (ck, sk) if pos_q is None else table(pos_q)
        q, k = q * cq + rot_half(q) * sq, k * ck + rot_half(k) * sk
    return q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), rq, rk


def attend(q, k, v, vis, rounded=False):
    """q [B,Hq,L,HD], k / v [B,Hkv,L,HD] float64, vis bool [B,L,L] -> O [B*L, Hq*HD], LSE [B,Hq,L] (+inf on rows with no visible key)."""
    B, Hq, L, _ = q.shape
    g = Hq // k.shape[1]
    kr, vr = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    s = (q @ kr.transpose(-1, -2)) * HD ** -0.5
    allow = vis[:, None]
    s = s.masked_fill(~allow, float("-inf"))
    any_key = allow.any(-1, keepdim=True)
    m = torch.where(any_key, s.amax(-1, keepdim=True), torch.zeros((), dtype=F64)).detach()
    p = torch.exp(s - m)                                                     # masked entries: exp(-inf) = 0
    if rounded:
        p = rb(p)                                                            # R3 (the denominator sums the rounded values)
    l = p.sum(-1, keepdim=True)
    o = (p @ vr) / torch.where(any_key, l, torch.ones((), dtype=F64))
    lse = torch.where(any_key, m + torch.log(torch.where(any_key, l, torch.ones((), dtype=F64))), torch.full((), float("inf"), dtype=F64))
    o = o.transpose(1, 2).reshape(B * L, Hq * HD)
    if rounded:
        o, lse = rb(o), rf(lse)                                              # R4
    return o, lse.squeeze(-1)


def forward(qkv0, B, L, Hq, Hkv, qn_w=None, kn_w=None, cos=None, sin=None, pos=None, kmask=None, segment_ids=None, rounded=False,
            vis=None, pos_q=None, x=None):
    """The whole block.  ``qkv0``: bf16 (its bits are the input) or float64.  ``vis`` / ``pos_q`` override the visibility / the query
    side's positions (the host tests perturb them); ``x`` is a float64 leaf to differentiate through (exact form).
    Returns dict(Q, K, V, rq, rk, O, LSE, vis)."""
    x = qkv0.cpu().to(F64) if x is None else x
    q, k, v, rq, rk = qk_post(x, B, L, Hq, Hkv, qn_w, kn_w, cos, sin, pos, pos_q)
    if rounded:
        q, k = rb(q), rb(k)                                                  # R1, R2
        rq, rk = (None, None) if rq is None else (rf(rq), rf(rk))
    vis = visibility(B, L, kmask, segment_ids) if vis is None else vis
    o, lse = attend(q, k, v, vis, rounded)
    return dict(Q=q, K=k, V=v, rq=rq, rk=rk, O=o, LSE=lse, vis=vis)


def mask_dO(dO, kmask, B, L):
    """Zero dO on padded query rows (kmask[b, q] == 0): padded rows carry no gradient in the model."""
    dO = dO.cpu().to(F64)
    if kmask is None:
        return dO
    return dO * (kmask.cpu() != 0).reshape(B * L, 1).to(F64)


def backward_exact(qkv0, dO, B, L, Hq, Hkv, **kw):
    """Autograd in float64 through ``forward`` (exact form).  dO: [B*L, Hq*HD], already masked.  -> (fwd dict, dQ, dK, dV, d(qkv0))."""
    x = qkv0.cpu().to(F64).clone().requires_grad_(True)
    out = forward(None, B, L, Hq, Hkv, x=x, **kw)
    for n in ("Q", "K", "V"):
        out[n].retain_grad()
    (out["O"] * dO.cpu().to(F64)).sum().backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = (dict((n, t.detach() if torch.is_tensor(t) else t) for n, t in out.items()), z(out["Q"]), z(out["K"]), z(out["V"]), z(x))
    return res


def attn_backward_formulas(Q, K, V, dO, lse, delta, vis, rounded):
    """The kernels' backward from its operands: P from the saved LSE, dS = P (dP - Delta) scale, R5.  float64 in, (dQ, dK, dV) f64 out."""
    B, Hq, L, _ = Q.shape
    Hkv = K.shape[1]
    g = Hq // Hkv
    sc = HD ** -0.5
    kr, vr = K.repeat_interleave(g, 1), V.repeat_interleave(g, 1)
    dOh = dO.reshape(B, L, Hq, HD).transpose(1, 2)
    s = (Q @ kr.transpose(-1, -2)) * sc
    finite = torch.isfinite(lse)[..., None]
    p = torch.exp(s - torch.where(finite, lse[..., None], torch.zeros((), dtype=F64)))
    p = torch.where(vis[:, None] & finite, p, torch.zeros((), dtype=F64))
    ds = p * (dOh @ vr.transpose(-1, -2) - delta[..., None]) * sc
    if rounded:
        p, ds = rb(p), rb(ds)                                                # R5
    dQ = ds @ kr
    dK = (ds.transpose(-1, -2) @ Q).reshape(B, Hkv, g, L, HD).sum(2)
    dV = (p.transpose(-1, -2) @ dOh).reshape(B, Hkv, g, L, HD).sum(2)
    return dQ, dK, dV


def post_backward(dQ, dK, dV, qkv0, rq, rk, B, L, Hq, Hkv, qn_w=None, kn_w=None, cos=None, sin=None, pos=None):
    """RoPE^T, RMSNorm backward, head-major -> token-major: d(qkv0) float64 [B*L, (Hq + 2 Hkv) * HD] (the math of ta_lm_qkv_post_bwd)."""
    x = qkv0.cpu().to(F64).reshape(B, L, Hq + 2 * Hkv, HD)
    dq, dk, dv = dQ.transpose(1, 2), dK.transpose(1, 2), dV.transpose(1, 2)            # [B, L, H, HD]
    if cos is not None:
        p = torch.arange(L)[None].expand(B, L) if pos is None else pos.cpu().long().reshape(B, L)
        c, s = cos.cpu().to(F64)[p], sin.cpu().to(F64)[p]
        c, s = torch.cat([c, c], -1)[:, :, None], torch.cat([s, s], -1)[:, :, None]
        dq, dk = dq * c - rot_half(dq * s), dk * c - rot_half(dk * s)                   # transpose of  y = n c + rot_half(n) s
    if qn_w is not None:
        def nb(d, xh, r, w):
            d = d * w.to(F64)
            xhat = xh * r
            return r * (d - xhat * (d * xhat).mean(-1, keepdim=True))
        dq = nb(dq, x[:, :, :Hq], rq.reshape(B, L, Hq, 1), qn_w)
        dk = nb(dk, x[:, :, Hq:Hq + Hkv], rk.reshape(B, L, Hkv, 1), kn_w)
    return torch.cat([dq, dk, dv], 2).reshape(B * L, (Hq + 2 * Hkv) * HD)


def backward_model(qkv0, dO, B, L, Hq, Hkv, rounded=True, qn_w=None, kn_w=None, cos=None, sin=None, pos=None, kmask=None, segment_ids=None,
                   vis=None, pos_q=None):
    """The kernels' backward restated by hand with their rounding points.  Returns a dict:
      fwd                      the forward dict (rounded form: Q, K, O bf16 values, LSE / rq / rk f32 values)
      delta                    rowsum(dO o O) [B, Hq, L]
      dQ, dK, dV               head-major, rounded to bf16 (R6): what ta_attention_bwd(_seg) returns
      dqkv_fused               d(qkv0) from the unrounded accumulators, rounded once (R7): ta_attention_bwd_qkv(_seg)
      dqkv_unfused             d(qkv0) from the bf16 dQ / dK / dV, rounded again: ta_attention_bwd + ta_lm_qkv_post_bwd
    With rounded=False nothing is rounded and dqkv_fused == dqkv_unfused == autograd's d(qkv0)."""
    assert pos_q is None or not rounded
    kw = dict(qn_w=qn_w, kn_w=kn_w, cos=cos, sin=sin, pos=pos)
    f = forward(qkv0, B, L, Hq, Hkv, kmask=kmask, segment_ids=segment_ids, rounded=rounded, vis=vis, pos_q=pos_q, **kw)
    dO = dO.cpu().to(F64)
    delta = (dO * f["O"]).reshape(B, L, Hq, HD).sum(-1).transpose(1, 2)
    if rounded:
        delta = rf(delta)
    dQ, dK, dV = attn_backward_formulas(f["Q"], f["K"], f["V"], dO, f["LSE"], delta, f["vis"], rounded)
    r = rb if rounded else (lambda t: t)
    fused = r(post_backward(dQ, dK, dV, qkv0, f["rq"], f["rk"], B, L, Hq, Hkv, **kw))
    dQ, dK, dV = r(dQ), r(dK), r(dV)
    unfused = r(post_backward(dQ, dK, dV, qkv0, f["rq"], f["rk"], B, L, Hq, Hkv, **kw))
    return dict(fwd=f, delta=delta, dQ=dQ, dK=dK, dV=dV, dqkv_fused=fused, dqkv_unfused=unfused)


# ----------------------------------------------------------------------------- the metric
def rows_of(t, width=HD):
    """Any tensor whose last dimension is a multiple of ``width`` -> float64 [rows, width].  Attention: width = HD, one (b, head, token)
    vector per row; other users (tests/moe_ref.py) pass the row length of their own matrices."""
    t = t.detach().cpu().to(F64)
    return t.reshape(-1, width)


def row_errors(got, exact, width=HD):
    """e_r = |got_r - exact_r|_2 / (|exact_r|_2 + rho),  rho = 1e-2 * the median row norm of ``exact``."""
    g, e = rows_of(got, width), rows_of(exact, width)
    assert g.shape == e.shape, (g.shape, e.shape)
    n = e.norm(dim=-1)
    rho = 1e-2 * n.median()
    return (g - e).norm(dim=-1) / (n + rho)


def gate(got, exact, model, factor=2.0, width=HD):
    """(passes, ratio, worst row index):  max_r e_r <= factor * max_r m_r, the bound coming from the reference's two forms alone."""
    e, m = row_errors(got, exact, width), row_errors(model, exact, width)
    bound = float(m.max())
    worst = int(e.argmax())
    if not torch.isfinite(e).all():
        return False, float("inf"), int((~torch.isfinite(e)).nonzero()[0])
    ratio = float(e.max()) / bound if bound > 0 else (0.0 if float(e.max()) == 0 else float("inf"))
    return float(e.max()) <= factor * bound, ratio, worst


# ----------------------------------------------------------------------------- inputs shared by the host and the GPU tests
QK_SCALE = 0.7


def make_inputs(L, Hq, Hkv, B=2, seed=0, table_rows=512, qk_scale=QK_SCALE):
    """Seeded CPU inputs: qkv0 bf16 [B*L, (Hq + 2 Hkv) * HD] with q | k ~ N(0, qk_scale^2) and v ~ N(0, 1), norm weights
    qk_scale * (1 + 0.1 N(0, 1)) f32, RoPE tables f32 [table_rows, HD / 2] (theta 1e6), dO bf16 [B*L, Hq*HD] ~ N(0, 1).
    qk_scale sets the spread of the scores (std qk_scale^2 with or without the norm) -- see tests/test_attention_ref.py for why 0.7."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    qkv0 = torch.randn(B * L, Hq + 2 * Hkv, HD, generator=g)
    qkv0[:, :Hq + Hkv] *= qk_scale
    qkv0 = qkv0.reshape(B * L, -1).to(torch.bfloat16)
    qn_w = (qk_scale * (1 + 0.1 * torch.randn(HD, generator=g))).float()
    kn_w = (qk_scale * (1 + 0.1 * torch.randn(HD, generator=g))).float()
    dO = torch.randn(B * L, Hq * HD, generator=g).to(torch.bfloat16)
    cos, sin = rope_tables(table_rows)
    return dict(qkv0=qkv0, qn_w=qn_w, kn_w=kn_w, cos=cos, sin=sin, dO=dO)


def segment_ids_of(rows, L):
    """rows: one list of segment lengths per batch row (the rest of the row is padding) -> int32 [B, L] ids 1.. (0 = padding)."""
    sid = torch.zeros(len(rows), L, dtype=torch.int32)
    for b, lens in enumerate(rows):
        assert sum(lens) <= L
        at = 0
        for i, n in enumerate(lens):
            sid[b, at:at + n] = i + 1
            at += n
    return sid

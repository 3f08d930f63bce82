"""CPU float64 reference of the shared + sparse MoE projector that ``csrc/moe.hip`` implements, the inputs whose routing is known by
construction, and the gates the MoE tests use.  A plain module (no fixtures): ``tests/test_moe_ref.py`` checks it on the host,
``tests/test_gpu_moe_grid.py`` compares the library with it.  The metric (``row_errors`` / ``gate``) is tests/attention_ref.py's.

The operation, from the bf16 bits of ``x [B, S, enc_dim]`` and the f32 masters (names as in the module's state dict):
  frame-stack k (tail frames dropped when S % k != 0) -> RMSNorm (eps 1e-6) -> shared adapter (fc1 + bias, erf-GELU, fc2 + bias)
  + router: logits = xn Wr^T, optional multiplicative jitter, softmax, top-2 (first maximum wins a tie), renormalise by (sum + 1e-6)
  + the two routed adapters weighted by the renormalised top-2 weights;
  aux = coef * E * mean_e((pbar_e - 1/E)^2) + zcoef * mean_t(lse_t^2) in training, 0 otherwise.
The routing is derived here, never read from the library's tape.

Two forms of the same function:
  exact           no intermediate rounding; the backward (``backward_exact``) is float64 autograd of sum(dy * y) + d_aux * aux.
  rounding model  (``rounded=True``) rounds to bf16 (nearest even) exactly where the kernels do and nowhere else; its backward
                  (``backward_model``) restates the kernels' formulas by hand (moe_combine_bwd_kernel, moe_router_bwd_kernel,
                  moe_router_dw_kernel, moe_norm_bwd_kernel).  With ``rounded=False`` the same hand-written backward must equal autograd
                  (tests/test_moe_ref.py), which ties the two forms together.

Rounding points of the kernels (moe.hip:line of the instruction that rounds), all modelled below:
  R1  weight images W1, W2 and their transposes -> bf16     moe.hip:489-490 (row-major), :497-498 (transposed), moe_pack_w_kernel.
      Biases, norm.weight and router.weight stay f32.
  R2  xn = x * rstd * w -> bf16                              moe.hip:40 (moe_norm_kernel); rstd is f32
  R3  h = xn W1^T + b1 -> bf16 (GEMM output)                 moe.hip:546 (shared), :555 (grouped) / :557 (per expert)
  R4  act = gelu(h) -> bf16                                  moe.hip:191-192 (gelu_bf16_kernel)
  R5  dout -> bf16 (the shared adapter's upstream gradient)  moe.hip:242
  R6  dy_slot = bf16(dout * topw), from the f32 dout         moe.hip:238-241
  R7  dact = dy W2 -> bf16 (GEMM output)                     moe.hip:593 (shared), :612 / :613
  R8  dh = dact * gelu'(h) -> bf16                           moe.hip:201-202 (gelu_bwd_bf16_kernel)
y, y_e, dxn_sh, dxn_slot, logits, probabilities, top-2 weights, dtopw and dlogits are f32 in the kernels and float64 here; every
product accumulates in f32 there and in float64 here (~2^-24 * K, far below bf16's 2^-9).  The roundings are straight-through in
the backward, as in the kernels.
"""
import math

import torch

from tests.attention_ref import F64, gate, rb, row_errors  # noqa: F401  (gate / row_errors are re-exported to the tests)

EPS = 1e-6
SQRT2 = math.sqrt(2.0)


def ident(t):
    return t


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / SQRT2))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / SQRT2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def adapters(E):
    """Routed experts 0 .. E - 1, then the shared expert: the order of the library's pointer arrays."""
    return [f"experts.{e}." for e in range(E)] + ["shared_expert."]


def param_names(E):
    return ["norm.weight", "router.weight"] + [p + s for p in adapters(E) for s in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]


def frame_stack(x, k):
    """bf16 / float [B, S, enc] -> float64 [B * N, k * enc], N = (S - k) // k + 1 (the tail frames are dropped)."""
    B, S, C = x.shape
    N = (S - k) // k + 1
    return x.detach().cpu().to(F64)[:, :N * k].reshape(B * N, k * C)


def top2(p):
    """int64 [T, 2]: the first maximum, then the first maximum of the rest (the kernel's and torch.topk's tie order)."""
    E = p.shape[-1]
    idx = torch.arange(E)[None].expand_as(p)
    big = torch.full_like(idx, E)
    i0 = torch.where(p == p.amax(-1, keepdim=True), idx, big).amin(-1)
    q = p.masked_fill(idx == i0[:, None], float("-inf"))
    i1 = torch.where(q == q.amax(-1, keepdim=True), idx, big).amin(-1)
    return torch.stack([i0, i1], -1)


def aux_loss(probs, lse, E, coef, zcoef):
    pbar = probs.mean(0)
    return coef * E * ((pbar - 1.0 / E) ** 2).mean() + zcoef * (lse ** 2).mean()


def forward(x, W, k, E, training=False, noise=None, coef=0.01, zcoef=1e-4, rounded=False, P=None, inject=None):
    """The whole projector.  ``x``: bf16 [B, S, enc] (its bits are the input).  ``W``: {name: f32 master}.  ``P``: float64 leaves to
    differentiate through (exact form) instead of ``W``.  ``noise`` [T, E] is applied in training only, as in the library.
    ``inject`` (test instrumentation, see tests/test_moe_ref.py): planted single-site errors.
    Returns a dict with y [T, D], aux, and every intermediate the hand-written backward needs."""
    inj = inject or {}
    r_ = rb if rounded else ident
    P = {n: t.detach().cpu().to(F64) for n, t in W.items()} if P is None else P
    xs = frame_stack(x, k)
    T = xs.shape[0]
    rstd = torch.rsqrt((xs * xs).mean(-1, keepdim=True) + EPS)
    if "rstd_from_neighbour" in inj:                      # the tail token reads its neighbour's 1 / rms
        rstd = rstd.clone(); rstd[T - 1] = rstd[T - 2]
    pre = xs * rstd * P["norm.weight"]
    xn = r_(pre)                                                                                  # R2
    Wb = {n: r_(P[n]) for n in P if n.endswith(("fc1.weight", "fc2.weight"))}                       # R1

    def adapter(p, inp):
        h = r_(inp @ Wb[p + "fc1.weight"].T + P[p + "fc1.bias"])                                  # R3
        act = r_(gelu(h))                                                                         # R4
        return h, act, act @ Wb[p + "fc2.weight"].T + P[p + "fc2.bias"]

    h_s, act_s, y_s = adapter("shared_expert.", xn)
    nz = noise.detach().cpu().to(F64) if (training and noise is not None) else None
    logits = xn @ P["router.weight"].T
    if nz is not None:
        logits = logits * nz
    lse = torch.logsumexp(logits, -1)
    probs = torch.exp(logits - lse[:, None])
    topi = top2(probs.detach())
    if "third_expert" in inj:                             # one token's second choice replaced by its third
        t = inj["third_expert"]
        order = torch.argsort(-probs[t].detach(), stable=True)
        topi[t, 1] = order[2]
    raw = probs.gather(1, topi)
    topw = raw / (raw.sum(-1, keepdim=True) + 1e-6)
    if "no_renorm" in inj:                                # one token's weights left as the raw probabilities
        m = torch.zeros(T, 1, dtype=torch.bool); m[inj["no_renorm"]] = True
        topw = torch.where(m, raw, topw)
    y = y_s
    slots = {}
    for e in range(E):
        tok, kk = (topi == e).nonzero(as_tuple=True)      # in token order: the plan's stable sort
        if tok.numel() == 0:
            slots[e] = None
            continue
        h, act, ye = adapter(f"experts.{e}.", xn[tok])
        y = y.index_add(0, tok, ye * topw[tok, kk][:, None])
        slots[e] = dict(tok=tok, kk=kk, h=h, act=act, y=ye)
    aux = aux_loss(probs, lse, E, coef, zcoef) if training else torch.zeros((), dtype=F64)
    return dict(y=y, aux=aux, xs=xs, rstd=rstd, pre=pre, xn=xn, Wb=Wb, P=P, h_s=h_s, act_s=act_s, logits=logits, lse=lse, probs=probs,
                topi=topi, raw=raw, topw=topw, slots=slots, noise=nz, training=training, counts=torch.bincount(topi.flatten(), minlength=E))


def backward_exact(x, W, dy, d_aux, k, E, **kw):
    """Float64 autograd of sum(dy * y) + d_aux * aux through ``forward`` (exact form).  -> (forward dict, {name: gradient})."""
    P = {n: t.detach().cpu().to(F64).clone().requires_grad_(True) for n, t in W.items()}
    f = forward(x, W, k, E, rounded=False, P=P, **kw)
    ((f["y"] * dy.detach().cpu().to(F64).reshape(f["y"].shape)).sum() + d_aux * f["aux"]).backward()
    grads = {n: (torch.zeros_like(p) if p.grad is None else p.grad) for n, p in P.items()}
    f = {n: (t.detach() if torch.is_tensor(t) else t) for n, t in f.items()}
    return f, grads


def backward_model(x, W, dy, d_aux, k, E, rounded=True, coef=0.01, zcoef=1e-4, inject=None, **kw):
    """The kernels' backward restated by hand with their rounding points.  -> (forward dict, {name: gradient}).
    With rounded=False nothing is rounded and the gradients equal autograd's."""
    inj = inject or {}
    r_ = rb if rounded else ident
    with torch.no_grad():
        f = forward(x, W, k, E, rounded=rounded, coef=coef, zcoef=zcoef, inject=inject, **kw)
        P, Wb, xn, T = f["P"], f["Wb"], f["xn"], f["xn"].shape[0]
        dout = dy.detach().cpu().to(F64).reshape(f["y"].shape)
        g = {}

        def adapter_bwd(p, d, h, act, inp, keep=None):
            """d: the (rounded) upstream gradient rows of adapter p.  ``keep``: rows that enter this adapter's parameter gradients."""
            dk, ak = (d, act) if keep is None else (d[keep], act[keep])
            g[p + "fc2.bias"] = dk.sum(0)
            g[p + "fc2.weight"] = dk.T @ ak
            dact = r_(d @ Wb[p + "fc2.weight"])                                                   # R7
            dh = r_(dact * gelu_grad(h))                                                          # R8
            hk, ik = (dh, inp) if keep is None else (dh[keep], inp[keep])
            g[p + "fc1.bias"] = hk.sum(0)
            g[p + "fc1.weight"] = hk.T @ ik
            return dh @ Wb[p + "fc1.weight"]

        dxn = adapter_bwd("shared_expert.", r_(dout), f["h_s"], f["act_s"], xn)                   # R5
        dtopw = torch.zeros(T, 2, dtype=F64)
        for e in range(E):
            p, s = f"experts.{e}.", f["slots"][e]
            if s is None:
                for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
                    g[p + n] = torch.zeros_like(P[p + n])
                continue
            tok, kk = s["tok"], s["kk"]
            dtopw[tok, kk] = (dout[tok] * s["y"]).sum(-1)
            keep = None
            if inj.get("drop_last_slot") == e:            # the last slot of this expert's segment misses its parameter gradients
                keep = torch.arange(tok.numel() - 1)
            dxn = dxn.index_add(0, tok, adapter_bwd(p, r_(dout[tok] * f["topw"][tok, kk][:, None]), s["h"], s["act"], xn[tok], keep))   # R6
        # moe_router_bwd_kernel
        probs, raw, topi = f["probs"], f["raw"], f["topi"]
        den = raw.sum(-1, keepdim=True) + 1e-6
        common = (dtopw * raw).sum(-1, keepdim=True) / (den * den)
        dp = torch.zeros_like(probs).scatter(1, topi, dtopw / den - common)
        if "no_renorm" in inj:
            dp[inj["no_renorm"]] = torch.zeros(E, dtype=F64).scatter(0, topi[inj["no_renorm"]], dtopw[inj["no_renorm"]])
        dl = torch.zeros_like(probs)
        if f["training"]:
            pbar = probs.mean(0)
            share = torch.ones(T, 1, dtype=F64)
            if "no_aux_token" in inj:                     # one token's dlogits miss the share of the auxiliary losses
                share[inj["no_aux_token"]] = 0.0
            dp = dp + share * (d_aux * coef * 2.0 * (pbar - 1.0 / E) / T)[None]
            dl = dl + share * d_aux * zcoef * 2.0 * f["lse"][:, None] * probs / T
        dlogits = dl + probs * (dp - (dp * probs).sum(-1, keepdim=True))
        if f["noise"] is not None:
            dlogits = dlogits * f["noise"]
        g["router.weight"] = dlogits.T @ xn                                                       # moe_router_dw_kernel
        dxn = dxn + dlogits @ P["router.weight"]
        g["norm.weight"] = (dxn * f["xs"] * f["rstd"]).sum(0)                                     # moe_norm_bwd_kernel
        f["dlogits"] = dlogits
    return f, g


# ----------------------------------------------------------------------------- how far the kernel's logits can be from the model's
U24 = 2.0 ** -24


def logit_bound(f, W):
    """[T]: a bound on |kernel logit - rounding-model logit| per token, from the two ways they differ.
    (a) xn.  The kernel forms x * rstd * w in f32: rstd from a sum of In squares (8 * In / 512 sequential adds per lane, 6 butterfly
        levels: at most In / 64 + 6 roundings, relative), one division, one hardware rsqrt (1 ulp), two multiplications; halved
        through the inverse square root for the sum's share.  An element whose float64 value lies within that relative distance of a
        bf16 tie (the midpoint of two neighbouring bf16 values) may round the other way, which moves xn[c] by one bf16 ulp and logit e
        by ulp * |Wr[e, c]|.  The bound sums exactly those elements, per token, and takes the worst expert.
    (b) fp32 accumulation of the In-term dot product (In / 64 sequential fused multiply-adds per lane + 6 butterfly levels):
        (In / 64 + 6) * 2^-24 * sum_c |xn[c] Wr[e, c]|, the worst expert; + 2^-24 |logit| for the jitter multiplication.
    (c) The kernel compares PROBABILITIES, from the fast exponential (2 ulp) and a division (1 ulp): two logits closer than
        2^-20 could compare either way.  Added as an absolute term.
    Jitter scales (a) and (b) by |noise| (at most 1.01 here)."""
    pre, xn = f["pre"], f["xn"]
    In = pre.shape[1]
    wr = W["router.weight"].detach().cpu().to(F64).abs()
    rel = ((In / 64 + 6) / 2 + 1 + 1 + 2) * U24
    a = pre.abs()
    ulp = torch.where(a > 0, torch.exp2(torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))) - 7), torch.zeros_like(a))
    frac = torch.where(a > 0, torch.remainder(a / torch.where(a > 0, ulp, torch.ones_like(a)), 1.0), torch.zeros_like(a))
    tie = ((frac - 0.5).abs() * ulp <= rel * a) & (a > 0)
    b_tie = ((ulp * tie) @ wr.T).amax(-1)
    b_acc = (In / 64 + 6) * U24 * (xn.abs() @ wr.T).amax(-1) + U24 * f["logits"].abs().amax(-1)
    scale = 1.0 if f["noise"] is None else f["noise"].abs().amax(-1)
    return (b_tie + b_acc) * scale + 2.0 ** -20, tie.sum(-1)


def gap23(logits):
    """[T]: the gap between the 2nd and the 3rd largest final logit (+inf with two experts)."""
    s = logits.sort(-1, descending=True).values
    return s[:, 1] - s[:, 2] if s.shape[1] > 2 else torch.full((s.shape[0],), float("inf"), dtype=F64)


# ----------------------------------------------------------------------------- inputs whose routing is known by construction
def assign_pairs(counts, T, n_zero, g):
    """counts [E] (sum 2 T, each <= T) -> int64 [T, 2] (first choice, second choice) per token and the zero-frame token mask.
    Zero-frame tokens take (0, 1): every logit is exactly 0 and the lowest indices win the tie.  The rest: always the two experts
    with the most slots left (which meets any feasible target), shuffled."""
    E = len(counts)
    left = list(counts)
    assert sum(left) == 2 * T and max(left) <= T, (counts, T)
    left[0] -= n_zero; left[1] -= n_zero
    assert min(left) >= 0
    pairs = []
    for _ in range(T - n_zero):
        a, b = sorted(range(E), key=lambda e: (-left[e], e))[:2]
        assert left[a] > 0 and left[b] > 0, (counts, T)
        left[a] -= 1; left[b] -= 1
        pairs.append((a, b) if torch.rand((), generator=g) < 0.5 else (b, a))
    assert not any(left)
    order = torch.randperm(T, generator=g)
    zero = torch.zeros(T, dtype=torch.bool)
    zero[order[:n_zero]] = True
    out = torch.zeros(T, 2, dtype=torch.int64)
    out[zero] = torch.tensor([0, 1])
    out[order[n_zero:]] = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    return out, zero


def make_weights(E, In, H, D, g):
    """f32 masters: norm.weight 1 + 0.1 N, router.weight N(0, (3 / sqrt(In))^2), fc1 N(0, 1 / In), fc2 N(0, 1 / H), biases 0.1 N."""
    rn = lambda *s: torch.randn(*s, generator=g)
    W = {"norm.weight": 1 + 0.1 * rn(In), "router.weight": rn(E, In) * 3 / math.sqrt(In)}
    for p in adapters(E):
        W[p + "fc1.weight"], W[p + "fc1.bias"] = rn(H, In) / math.sqrt(In), 0.1 * rn(H)
        W[p + "fc2.weight"], W[p + "fc2.bias"] = rn(D, H) / math.sqrt(H), 0.1 * rn(D)
    return {n: t.float().contiguous() for n, t in W.items()}


def make_inputs(B, N, extra, enc, k, E, H, D, counts, n_zero=0, noise=False, seed=0):
    """Seeded CPU inputs of one case.  Token t with target pair (a, b) is
        x_t = z_perp + 0.05 z_par + alpha_t (u_a + c_t u_b),   alpha_t ~ U(0.8, 1.2),  c_t ~ U(0.4, 0.6),
    u_e the unit vector along norm.weight o router.weight[e] (what the logit of expert e contracts the normalised x with) and z ~ N(0, I)
    split into its parts inside and orthogonal to the span of the u_e: logit a is about 3 alpha, logit b about 3 alpha c, the others a few
    tenths, so the top-2 is (a, b) by construction while the token's energy sits in z.  Frames past N * k are random (they are dropped)."""
    g = torch.Generator(device="cpu").manual_seed(5000 + seed)
    In, T = enc * k, B * N
    W = make_weights(E, In, H, D, g)
    pairs, zero = assign_pairs(counts, T, n_zero, g)
    v = (W["norm.weight"] * W["router.weight"]).to(F64)
    u = v / v.norm(dim=-1, keepdim=True)
    Q, _ = torch.linalg.qr(v.T)                                            # [In, E] orthonormal basis of the span
    z = torch.randn(T, In, generator=g, dtype=F64)
    zpar = (z @ Q) @ Q.T
    alpha = 0.8 + 0.4 * torch.rand(T, 1, generator=g, dtype=F64)
    c = 0.4 + 0.2 * torch.rand(T, 1, generator=g, dtype=F64)
    xt = (z - zpar) + 0.05 * zpar + alpha * (u[pairs[:, 0]] + c * u[pairs[:, 1]])
    xt[zero] = 0.0
    x = torch.randn(B, N * k + extra, enc, generator=g, dtype=F64)
    x[:, :N * k] = xt.reshape(B, N * k, enc)
    nz = (1 + 0.01 * (2 * torch.rand(T, E, generator=g) - 1)).float() if noise else None
    dy = torch.randn(B, N, D, generator=g).float()
    return dict(x=x.to(torch.bfloat16), W=W, noise=nz, dy=dy, pairs=pairs, zero=zero)


def routing_conditions(fx, fm, W, counts, zero):
    """What a case's inputs must satisfy, from the reference alone: (1) the per-expert slot counts of the rounding model equal the
    targets; (2) on every token that is not built from all-zero frames, the gap between the 2nd and 3rd final logit of the rounding
    model exceeds twice ``logit_bound``; (3) the exact form chooses the same two experts for every token (so the two forms, whose
    logits differ by the bf16 rounding of xn, describe the same routing).  -> (ok, dict of figures)."""
    bound, n_tie = logit_bound(fm, W)
    gap = gap23(fm["logits"])
    live = ~zero
    margin = (gap / (2 * bound))[live]
    same = bool((fx["topi"].sort(-1).values == fm["topi"].sort(-1).values).all())
    got = fm["counts"].tolist()
    zero_ok = bool((fm["topi"][zero] == torch.tensor([0, 1])).all()) and bool((fm["logits"][zero] == 0).all())
    ok = got == list(counts) and same and zero_ok and (margin.numel() == 0 or float(margin.min()) > 1.0)
    return ok, dict(counts=got, same=same, min_margin=float(margin.min()) if margin.numel() else float("inf"),
                    max_bound=float(bound[live].max()) if live.any() else 0.0, ties=int(n_tie.sum()))


# ----------------------------------------------------------------------------- the scalar gate of the auxiliary loss
AUX_FACTOR = 2.0


def aux_f32(fm, E, coef, zcoef):
    """The formula evaluated in float32 arithmetic from the rounding model's f32 probabilities and lse."""
    return float(aux_loss(fm["probs"].float(), fm["lse"].float(), E, torch.tensor(coef), torch.tensor(zcoef)))


def gate_aux(got, exact, model, f32_eval):
    """Scalar gate: |got - exact| <= AUX_FACTOR * |model - exact|; where the model's deviation is zero, the reference's own f32-vs-f64
    evaluation of the formula stands in for it.  AUX_FACTOR is 2, the factor of every tensor gate: the library works from the same bf16
    xn as the model, so its deviation IS the model's plus f32 noise (T atomic adds, fast exp / log: ~1e-7 relative) -- measured ratios
    are in profiles/moe_grid.md.  -> (passes, ratio)."""
    dev = abs(model - exact)
    if dev == 0.0:
        dev = abs(f32_eval - model)
    err = abs(got - exact)
    ratio = err / dev if dev > 0 else (0.0 if err == 0 else float("inf"))
    return err <= AUX_FACTOR * dev, ratio


# ----------------------------------------------------------------------------- the case grid (shared by the host and the GPU tests)
ENC, K = 128, 4                                              # In = 512: the smallest the library accepts
COEF, ZCOEF = 0.01, 1e-4
SEED_TRIES = 20


def _case(cid, B, N, extra, E, H, counts, mode, d_aux, D=128, n_zero=0):
    """mode: 'eval', 'train' (no jitter) or 'noise' (training with jitter).  T = B * N tokens, S = N * k + extra frames per clip."""
    from types import SimpleNamespace
    assert sum(counts) == 2 * B * N and len(counts) == E, cid
    return cid, SimpleNamespace(id=cid, B=B, N=N, T=B * N, extra=extra, S=N * K + extra, E=E, H=H, D=D, counts=tuple(counts), mode=mode,
                                training=mode != "eval", noise=mode == "noise", d_aux=float(d_aux), n_zero=n_zero)


# T: 1, 3, 5 (the router's four tokens per wave and its clamp), 63 / 64 / 65 (one 64-slot tile), 511 / 512 / 513 (2T around the plan's
# 1024-slot chunk) and 1100 (three chunks: the carried run[e]).  Counts: 0, 1, 63, 64, 65, 128 slots, one pair only, near-uniform.
CASES = dict([
    _case("T1-E2-eval", 1, 1, 0, 2, 64, [1, 1], "eval", 0),
    _case("T3-E3-train", 3, 1, 1, 3, 64, [3, 2, 1], "train", 3),
    _case("T5-E4-noise", 1, 5, 3, 4, 128, [5, 4, 1, 0], "noise", 3),
    _case("T63-E4-onepair-eval", 3, 21, 0, 4, 64, [0, 63, 0, 63], "eval", 0),
    _case("T64-E8-train", 2, 32, 2, 8, 64, [64, 0, 63, 0, 1, 0, 0, 0], "train", 0),
    _case("T65-E4-noise", 5, 13, 0, 4, 128, [65, 64, 1, 0], "noise", 3),
    _case("T65-E4-zeroframes", 5, 13, 1, 4, 64, [40, 30, 35, 25], "train", 3, n_zero=4),
    _case("T511-E8-uniform-train", 7, 73, 1, 8, 64, [128, 128, 128, 128, 128, 128, 127, 127], "train", 3),
    _case("T512-E8-noise", 2, 256, 0, 8, 64, [512, 128, 65, 64, 63, 1, 0, 191], "noise", 0),
    _case("T513-E3-train", 3, 171, 3, 3, 128, [513, 449, 64], "train", 3),
    _case("T1100-E4-uniform-noise", 4, 275, 2, 4, 64, [550, 550, 550, 550], "noise", 3),
    _case("T1100-E8-skew-train", 4, 275, 0, 8, 64, [779, 0, 1, 63, 64, 65, 128, 1100], "train", 3),
    _case("T1100-E2-eval", 4, 275, 1, 2, 64, [1100, 1100], "eval", 0),
    # llm_dim % 64 != 0: the row tails of ta_moe_pack_images.  Forward only -- the backward's products contract over llm_dim, and the
    # library's GEMM takes K in multiples of 64 (the backward answers TA_ERR_ARG there).
    _case("T65-E4-D196-train", 5, 13, 0, 4, 128, [33, 32, 33, 32], "train", 3, D=196),
])
ALL = list(CASES)
_REFS = {}


def build_case(cid, seed):
    from types import SimpleNamespace
    c = CASES[cid]
    I = make_inputs(c.B, c.N, c.extra, ENC, K, c.E, c.H, c.D, c.counts, n_zero=c.n_zero, noise=c.noise, seed=seed)
    kw = dict(training=c.training, noise=I["noise"], coef=COEF, zcoef=ZCOEF)
    fx, gx = backward_exact(I["x"], I["W"], I["dy"], c.d_aux, K, c.E, **kw)
    fm, gm = backward_model(I["x"], I["W"], I["dy"], c.d_aux, K, c.E, rounded=True, **kw)
    ok, fig = routing_conditions(fx, fm, I["W"], c.counts, I["zero"])
    return SimpleNamespace(c=c, seed=seed, I=I, kw=kw, fx=fx, gx=gx, fm=fm, gm=gm, ok=ok, fig=fig)


def ref(cid):
    """The case's inputs, exact reference and rounding model at the first seed of  index, index + 100, ...  whose routing meets
    ``routing_conditions``; computed once, never modified.  ``tries`` records how many seeds were drawn."""
    if cid not in _REFS:
        for n in range(SEED_TRIES):
            r = build_case(cid, ALL.index(cid) + 100 * n)
            if r.ok:
                r.tries = n + 1
                _REFS[cid] = r
                break
        else:
            raise AssertionError(f"{cid}: no input seed in {SEED_TRIES} tries meets the routing conditions ({r.fig})")
    return _REFS[cid]


def width_of(name, t):
    """Rows of a weight gradient are the rows of the matrix; a bias / norm gradient is one row."""
    return t.shape[-1] if (name.endswith("weight") and t.dim() == 2) else t.numel()

"""CPU float64 reference of the row-wise kernels around the GEMMs -- csrc/norm.hip (LayerNorm, RMSNorm and its backward forms), the
LayerNorm(z * keep + res) pair of csrc/nn_prims.hip, csrc/loss.hip (shifted labels, cross-entropy) and csrc/optim.hip (sum g^2, AdamW)
-- and the gates the tests put on them.  A plain module (no fixtures): ``tests/test_rowwise_ref.py`` checks it on the host,
``tests/test_gpu_rowwise_grid.py`` compares every exported entry point with it.  The row metric (``rb``, ``rf``, ``row_errors``,
``gate``) is the one of tests/attention_ref.py, imported, not copied.

Every operation is ONE function evaluated in two arithmetics (``model=False`` / ``model=True``):
  exact   float64 from the bf16 / f32 bits the kernel gets (hyper-parameters: their f32 bits), no intermediate rounding.  Backward
          formulas are written out by hand and tests/test_rowwise_ref.py ties them to float64 autograd.
  model   what a correct f32 kernel of this kind may deviate by, stated without looking at any kernel's output: the same formula in
          float32 tensors, so every elementwise operation is rounded to f32; every reduction is accumulated strictly left to right in
          f32 (``lsum``: numpy's add.accumulate in float32 -- torch's CPU cumsum accumulates float32 in double and would not do);
          exp, log, rsqrt, erf are the correctly rounded f32 functions (evaluated in float64, rounded once); a bf16 output is the
          f32 value rounded to nearest even by the caller (``rb``).  The functions return the values BEFORE that last rounding.
          Left to right is the most error-prone order, so it dominates the kernels' (a float4 per lane, 64 strided lanes, an xor
          tree): tests/test_rowwise_ref.py emulates that order with a 1-ulp rsqrt and finds it within 2x the model on every case.

One term is added to the rule above, from the specification of the instruction and not from any output:
  rsqrt   rsqrtf compiles to the hardware's v_rsq_f32, which the HIP math API documents as accurate to 1 ulp, not correctly rounded.
          rstd feeds every element of its row and IS an output, and with the planted rows the rstd vector is dominated by one or two
          deterministic values (the zero row: rsqrt(eps)), whose correctly rounded result may by chance sit within 0.03 ulp of the
          exact one (it does at eps = 1e-6): a bound made of that luck would reject a hardware result that is inside its
          specification.  Size: 1 ulp_f32 = 2^-23 relative on rstd.  The model therefore takes the correctly rounded rsqrt PLUS ONE ulp:
          its error is (1 + d) ulp with |d| <= 1/2, so any result within 1 ulp of the exact value stays within 2x of it.

Measured on the MI355X (profiles/rowwise_grid.md), a second term had to be added, again from the arithmetic and not from the figures:
  last place   where ONE element carries an output -- a spike row's y (its norm is that element's), a vector of M = 1, dw of one row,
          the scalars loss and sum g^2 -- the model's error is a single sample of a handful of f32 roundings, and these can cancel
          (the loss of 31 rows of V = 3 came out 0.14 ulp from the exact sum) while a correct kernel's do not: the kernel is free to
          contract a * b + c into an fma, to associate d * rstd * w the other way and to add in another order, and each choice moves
          the element by up to 1/2 ulp.  Size: two such roundings, 1 ulp_f32 of the element.  ``last_place`` moves every element of the
          model's f32 value (before a bf16 rounding) by LAST_PLACE_ULP = 1 ulp_f32 away from the exact value, so m_r never falls below
          one f32 ulp of the row; elements that are exactly 0 in both forms stay 0.  Every gate of the GPU tests applies it.

  unordered    dw of ta_rmsnorm_bwd and ta_rmsnorm_dw, dgamma / dbeta of ta_layernorm_bwd and the loss of ta_cross_entropy without an nll
          buffer are accumulated with float atomics: the n rows are added in whatever order the waves and workgroups finish, which
          differs from run to run, and ONE left-to-right sample does not bound an arbitrary order.  Size: each of the n additions
          rounds by at most ulp / 2 of its partial sum, the partial sums are of the size of the largest entry of the result, and
          independent roundings add in quadrature: sqrt(n) / 2 ulp_f32(max |exact|).  ``unordered`` moves the model by that much away
          from the exact value (n = the number of rows added, times the number of calls for the loss).  It still stands ~1e5 below
          the effect of one row left out or added twice.

Gates (no element and no row is excluded from any):
  rows      ``gate(got, exact, model, factor=2, width=H)``: max_r e_r <= 2 max_r m_r.  A vector (rstd, nll, dw, dgamma) is one row.
  scalars   ``scalar_gate``: |got - exact| <= 2 |model - exact| (loss, sum g^2); the case must make the model's deviation non-zero.
  bf16      ``elem_gate``: |got - exact| <= ulp_bf16(max(|got|, |exact|)) / 2 + 2 a_r, a_r the largest |model - exact| of that row
            before the bf16 rounding.  This is the gate that tells nearest-even from truncation.
  exact     outputs the operation defines exactly are compared with ==: a zero row through RMSNorm, rowscale = 0 rows, the dlogits
            row of an invalid target, dlogits columns >= V, dw of an all-zero dy.

Inputs (``rows_input``): seeded N(0, 1) rows plus planted rows at fixed indices, in this order while a random row is left:
  row 0 zero; row M-1 a spike (one element 1e3, the rest N(0, 1)) at column H-1; row 1 scaled 1e-4 (eps-dominated for RMSNorm at
  eps 1e-6); row 2 scaled 1e3; row 3 a spike at column 0; row 4 a spike at column 256 (H / 2 if H <= 256); LayerNorms only: row 5
  with mean 30 and std 1 (it separates a two-pass variance from a one-pass one).  M = 1 has no room: its row is random.
A NON-ZERO CONSTANT row is deliberately not planted into a LayerNorm: its exact result is 0 * rstd while f32 gives rounding noise times
eps^-1/2 (1e6 at the Q-Former's eps = 1e-12), so it would measure nothing.  gamma = 1 + 0.1 N(0, 1) and beta = 0.5 N(0, 1) differ in
every column, so a column shift cannot pass.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests.attention_ref import F64, gate, rb, rf, row_errors  # noqa: F401  (re-exported: the tests take the metric from here)

F32, BF16 = torch.float32, torch.bfloat16
RSQRT_ULP = 1
LAST_PLACE_ULP = 1
INV_SQRT2 = 0.70710678118654752
INV_SQRT_2PI = 0.3989422804014327


def f32v(v):
    """The value a C ``float`` argument carries."""
    return float(np.float32(v))


def lsum(x, dim=-1):
    """Sum of a float32 tensor along ``dim``, accumulated strictly left to right in float32."""
    a = np.add.accumulate(x.contiguous().numpy(), axis=dim, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.take(a, -1, axis=dim)))


class _Arith:
    """The arithmetic a formula below is evaluated in.  ``t``: the bits of an input in that arithmetic."""

    def __init__(self, model):
        self.model, self.dt = model, (F32 if model else F64)

    def t(self, x):
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.tensor(np.float32(x))                                   # a float argument of the C ABI
        return x.detach().cpu().to(self.dt)

    def sum(self, x, dim=-1):
        return lsum(x, dim) if self.model else x.sum(dim)

    def _fn(self, f, x):
        return f(x.to(F64)).to(self.dt)                                      # model: correctly rounded f32

    def rsqrt_cr(self, x): return self._fn(torch.rsqrt, x)

    def rsqrt(self, x):
        """Model: the correctly rounded value plus RSQRT_ULP ulp (see the module docstring)."""
        r = self.rsqrt_cr(x)
        return (r.view(torch.int32) + RSQRT_ULP).view(F32) if self.model else r

    def exp(self, x): return self._fn(torch.exp, x)
    def log(self, x): return self._fn(torch.log, x)
    def erf(self, x): return self._fn(torch.erf, x)
    def sqrt(self, x): return self._fn(torch.sqrt, x)

    def c(self, v):
        """A constant: the f32 literal in the model, the full double in the exact form."""
        return torch.tensor(v, dtype=self.dt)


def _out(**kw):
    return {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}


# ----------------------------------------------------------------------------- LayerNorm
def layernorm(x, w, b, eps, rowscale=None, model=False):
    """ta_layernorm_f32 / ta_layernorm_bf16: y = ((x - mean) * rstd * w + b) * rowscale.  -> y [M, H]."""
    A = _Arith(model)
    x, w, b = A.t(x), A.t(w), A.t(b)
    H = x.shape[-1]
    d = x - (A.sum(x) / H)[:, None]
    rstd = A.rsqrt(A.sum(d * d) / H + f32v(eps))
    y = d * rstd[:, None] * w + b
    if rowscale is not None:
        y = y * A.t(rowscale)[:, None]
    return _out(y=y, rstd=rstd)


def layernorm_res(z, keep, res, res_rows, gamma, beta, eps, model=False, leaf=None):
    """ta_layernorm_res_fwd: LayerNorm(u), u = z * keep + res[row % res_rows].  -> xhat, rstd, y.  ``leaf``: a float64 u to
    differentiate through (exact form only)."""
    A = _Arith(model)
    z, g, b = A.t(z), A.t(gamma), A.t(beta)
    M, H = z.shape
    u = z
    if keep is not None:
        u = u * A.t(keep)
    if res is not None:
        rr = int(res_rows) if res_rows and res_rows > 0 else M
        u = u + A.t(res)[torch.arange(M) % rr]
    if leaf is not None:
        u = leaf
    d = u - (A.sum(u) / H)[:, None]
    rstd = A.rsqrt(A.sum(d * d) / H + f32v(eps))
    xhat = d * rstd[:, None]
    return _out(xhat=xhat, rstd=rstd, y=xhat * g + b, u=u)


def layernorm_bwd(dy, xhat, rstd, gamma, keep, dgamma0, dbeta0, model=False):
    """ta_layernorm_bwd from the f32 xhat / rstd it is given: du = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma;
    dz = du * keep (bf16 in the library: round with rb); dgamma = dgamma0 + sum_rows dy xhat; dbeta = dbeta0 + sum_rows dy."""
    A = _Arith(model)
    dy, xh, r, w = A.t(dy), A.t(xhat), A.t(rstd), A.t(gamma)
    H = dy.shape[-1]
    g = dy * w
    m1, m2 = A.sum(g) / H, A.sum(g * xh) / H
    du = r[:, None] * (g - m1[:, None] - xh * m2[:, None])
    dz = du if keep is None else du * A.t(keep)
    return _out(du=du, dz=dz, dgamma=A.t(dgamma0) + A.sum(dy * xh, 0), dbeta=A.t(dbeta0) + A.sum(dy, 0))


# ----------------------------------------------------------------------------- RMSNorm
def _gelu(A, n):
    return (0.5 * n) * (1.0 + A.erf(n * A.c(INV_SQRT2)))


def _gelu_grad(A, n):
    return 0.5 * (1.0 + A.erf(n * A.c(INV_SQRT2))) + (n * A.c(INV_SQRT_2PI)) * A.exp((-0.5 * n) * n)


def rmsnorm_fwd(x, w, eps, gelu=False, model=False):
    """ta_rmsnorm_fwd / ta_rmsnorm_fwd_bf16: rstd = (mean(x^2) + eps)^-1/2, y = x * rstd * w, optionally erf-GELU(y)."""
    A = _Arith(model)
    x, w = A.t(x), A.t(w)
    H = x.shape[-1]
    rstd = A.rsqrt(A.sum(x * x) / H + f32v(eps))
    y = x * rstd[:, None] * w
    if gelu:
        y = _gelu(A, y)
    return _out(y=y, rstd=rstd)


def rmsnorm_bwd(dy, x, rstd, w, dres=None, gelu=False, dw0=None, model=False):
    """The five exported backward forms (the dtypes of dy, x and dres say which bits come in), from the f32 rstd they are given:
    xh = x rstd; d = dy * gelu'(xh w) (GELU form); dw = dw0 + sum_rows d xh; dn = d w; dx = rstd (dn - xh mean(dn xh)) + dres."""
    A = _Arith(model)
    dy, x, r, w = A.t(dy), A.t(x), A.t(rstd), A.t(w)
    H = x.shape[-1]
    xh = x * r[:, None]
    d = dy * _gelu_grad(A, xh * w) if gelu else dy
    dn = d * w
    dx = r[:, None] * (dn - xh * (A.sum(dn * xh) / H)[:, None])
    if dres is not None:
        dx = dx + A.t(dres)
    out = _out(dx=dx)
    if dw0 is not None:
        out.update(_out(dw=A.t(dw0) + A.sum(d * xh, 0)))
    return out


def rmsnorm_dw(dy, x, rstd, dw0, model=False):
    """ta_rmsnorm_dw: dw = dw0 + sum_rows dy * x * rstd."""
    A = _Arith(model)
    return _out(dw=A.t(dw0) + A.sum(A.t(dy) * A.t(x) * A.t(rstd)[:, None], 0))


# ----------------------------------------------------------------------------- labels and cross-entropy
def label_rows(labels):
    """labels: B lists of L Python integers.  The target of position (b, l) is labels[b][l + 1]; -100 and every row's last position
    carry none.  -> (rows, targets, n): flat positions b * L + l in increasing order, plain integers."""
    rows, targets = [], []
    for b, seq in enumerate(labels):
        L = len(seq)
        for l in range(L - 1):
            if seq[l + 1] != -100:
                rows.append(b * L + l)
                targets.append(int(seq[l + 1]))
    return rows, targets, len(rows)


def cross_entropy(logits, rows, targets, V, scale, ldd, model=False):
    """ta_cross_entropy.  logits [R, ldl] (only columns < V are ever read), rows: list of row indices or None, targets: list of n
    integers (valid: 0 <= t < V).  -> nll [n] (0 on invalid rows), loss = sum_i nll_i * scale in row order, dlogits [n, ldd] =
    (softmax - onehot) * scale before the bf16 rounding: rows of invalid targets and columns >= V are exactly 0."""
    A = _Arith(model)
    n = len(targets)
    idx = torch.arange(n) if rows is None else torch.tensor(rows, dtype=torch.long)
    z = A.t(logits)[idx][:, :V]
    t = torch.tensor(targets, dtype=torch.long)
    valid = (t >= 0) & (t < V)
    tc = torch.where(valid, t, torch.zeros_like(t))
    sc = A.t(scale)
    m = z.amax(-1)
    lse = m + A.log(A.sum(A.exp(z - m[:, None])))
    nll = torch.where(valid, lse - z.gather(1, tc[:, None])[:, 0], torch.zeros((), dtype=A.dt))
    loss = A.sum(nll * sc, 0)
    d = A.exp(z - lse[:, None]) * sc
    d[torch.arange(n), tc] -= sc
    d = d * valid[:, None].to(A.dt)
    dl = torch.zeros(n, ldd, dtype=A.dt)
    dl[:, :min(V, ldd)] = d[:, :min(V, ldd)]
    return _out(nll=nll, loss=loss, dlogits=dl, valid=valid)


# ----------------------------------------------------------------------------- optimizer
def sqnorm(g, acc0=0.0, model=False):
    """ta_grad_sqnorm: acc0 + sum g^2."""
    A = _Arith(model)
    g = A.t(g).reshape(-1)
    return (A.t(acc0) + A.sum(g * g, 0)).to(F64)


def clip_coef(sq, max_norm, grad_scale, denom, model=False):
    """optim.hip: grad_scale /= max(denom, 1) if denom is given; coef = grad_scale; if sq is given and max_norm > 0:
    coef *= min(1, max_norm / (sqrt(sq) * |grad_scale| + 1e-6))."""
    A = _Arith(model)
    gs = A.t(grad_scale)
    if denom is not None:
        gs = gs / torch.maximum(A.t(denom), A.c(1.0))
    coef = gs
    if sq is not None and max_norm > 0:
        total = A.sqrt(A.t(sq)) * gs.abs()
        coef = coef * torch.minimum(A.c(1.0), A.t(max_norm) / (total + A.t(1e-6)))
    return coef


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, sq=None, max_norm=0.0, grad_scale=1.0, denom=None, model=False):
    """One ta_adamw_step (lr, wd scalars) or ta_adamw_step_multi (lr, wd per element: seg_lr * lr_mult and seg_wd spread over their
    segments).  bias corrections 1 - beta^step: computed in f32 on the host in the library.  -> (p, m, v) float64."""
    A = _Arith(model)
    p, g, m, v = A.t(p), A.t(g), A.t(m), A.t(v)
    lr, wd, b1, b2, eps = A.t(lr), A.t(wd), A.t(beta1), A.t(beta2), A.t(eps)
    one = A.c(1.0)
    if model:
        bc1 = torch.tensor(np.float32(1) - np.float32(f32v(beta1) ** step))
        bc2 = torch.tensor(np.float32(1) - np.float32(f32v(beta2) ** step))
    else:
        bc1, bc2 = one - b1 ** step, one - b2 ** step
    gi = g * clip_coef(sq, max_norm, grad_scale, denom, model)
    pi = p * (one - lr * wd)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    pi = pi - lr * (mi / bc1) / (A.sqrt(vi / bc2) + eps)
    return pi.to(F64), mi.to(F64), vi.to(F64)


# ----------------------------------------------------------------------------- the gates
def ulp_bf16(x):
    """The spacing of bf16 at |x| (float64 in, float64 out); the smallest normal's below it."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 1 - 7)


def ulp_f32(x):
    """The spacing of f32 at |x| (float64 in and out); the smallest normal's below it."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 1 - 23)


def last_place(model, exact):
    """The model's f32 value moved LAST_PLACE_ULP ulp_f32 away from the exact one (module docstring); 0 == 0 stays."""
    m, e = torch.as_tensor(model, dtype=F64), torch.as_tensor(exact, dtype=F64)
    s = torch.where(m >= e, 1.0, -1.0).to(F64) * ((m != 0) | (e != 0)).to(F64)
    return m + s * LAST_PLACE_ULP * ulp_f32(m)


def unordered(model, exact, n):
    """The model of a sum whose n terms are added in an unspecified order (module docstring).  0 == 0 stays."""
    m, e = torch.as_tensor(model, dtype=F64), torch.as_tensor(exact, dtype=F64)
    s = torch.where(m >= e, 1.0, -1.0).to(F64) * ((m != 0) | (e != 0)).to(F64)
    return m + s * (0.5 * float(n) ** 0.5) * ulp_f32(e.abs().max())


def trunc_bf16(x):
    """f32 -> bf16 by dropping the low 16 bits (toward zero): the store a correct kernel must NOT do.  float64 out."""
    i = x.to(F32).contiguous().view(torch.int32) & -65536
    return i.view(F32).to(F64)


def elem_gate(got, exact, pre, width):
    """The element-wise gate of a bf16 output.  ``pre``: the model before its bf16 rounding.  -> (passes, worst |err| / limit, flat index)."""
    g, e, p = (t.detach().cpu().to(F64).reshape(-1, width) for t in (got, exact, pre))
    a = (p - e).abs().amax(-1, keepdim=True)
    lim = 0.5 * ulp_bf16(torch.maximum(g.abs(), e.abs())) + 2.0 * a
    err = (g - e).abs()
    if not torch.isfinite(err).all():
        return False, float("inf"), int((~torch.isfinite(err)).reshape(-1).nonzero()[0])
    r = torch.where(err > 0, err / lim, torch.zeros_like(err))
    return bool((err <= lim).all()), float(r.max()), int(r.argmax())


def scalar_gate(got, exact, model, factor=2.0):
    """|got - exact| <= factor |model - exact|.  -> (passes, ratio)."""
    dev, err = abs(float(model) - float(exact)), abs(float(got) - float(exact))
    assert dev > 0, "the case must make the model's deviation non-zero"
    return err <= factor * dev, err / dev


# ----------------------------------------------------------------------------- inputs shared by the host and the GPU tests
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def planted(M, H, layernorm_rows):
    """{row index: kind} in the order of the module docstring, as long as one random row is left."""
    mid = 256 if H > 256 else H // 2
    order = [(0, ("zero",)), (M - 1, ("spike", H - 1)), (1, ("scale", 1e-4)), (2, ("scale", 1e3)), (3, ("spike", 0)), (4, ("spike", mid))]
    if layernorm_rows:
        order.append((5, ("mean", 30.0)))
    out = {}
    for r, kind in order:
        if 0 <= r < M and r not in out and len(out) + 1 < M:
            out[r] = kind
    return out


def rows_input(M, H, seed, layernorm_rows=False, plant=True):
    """f32 [M, H]: N(0, 1) rows with the planted rows of ``planted``."""
    x = torch.randn(M, H, generator=_gen(M, H, seed))
    if plant:
        for r, kind in planted(M, H, layernorm_rows).items():
            if kind[0] == "zero": x[r] = 0.0
            elif kind[0] == "scale": x[r] *= kind[1]
            elif kind[0] == "spike": x[r, kind[1]] = 1e3
            elif kind[0] == "mean": x[r] += kind[1]
    return x


def gamma_beta(H, seed):
    g = _gen(H, seed, 77)
    return (1 + 0.1 * torch.randn(H, generator=g)).float(), (0.5 * torch.randn(H, generator=g)).float()


def rowscale_pattern(M):
    """0 on rows 1, 4, 7, ..., 1 elsewhere."""
    return ((torch.arange(M) % 3) != 1).float()


HS_FWD = (4, 252, 256, 260, 512, 768, 1024, 1028, 1280, 1536, 1792, 2048, 2052, 2304, 5120)
HS_BWD = (4, 128, 260, 768, 1024, 1028, 1792, 2048, 2052, 5120)
HS_LNRES = (4, 252, 260, 1024, 1028, 2048)
LN_EPS, RMS_EPS = 1e-5, 1e-6
CAP_M = 2049 + 4 * 512 + 3            # ta_rmsnorm_bwd with dw: 512 blocks of 4 rows, every block strides, the last group ragged
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
MULTI_N = 4096 * 1024 + 1028

CASES = dict(
    layernorm=dict(H=HS_FWD, M=(1, 3, 9, 37), walk_H=(256, 1280), walk_M=(4095, 4097, 8191, 8193, 8194, 8195), eps=LN_EPS),
    rmsnorm_fwd=dict(H=HS_FWD, M=(1, 7, 9, 37), eps=RMS_EPS),
    rmsnorm_bwd=dict(H=HS_BWD, M=(1, 9, 37), cap=(CAP_M, 128)),
    rmsnorm_dw=dict(MH=((1, 4), (31, 252), (33, 260), (65, 1024))),
    layernorm_res=dict(H=HS_LNRES, M=(1, 33, 70), eps=(1e-5, 1e-12), res_rows=(0, "M", 7)),
    label_rows=dict(BL=((1, 1), (3, 50), (1, 1024), (1, 1025), (4, 256), (5, 300), (2, 1500)), kinds=("none", "all", "chunk_last", "pos0", "random")),
    cross_entropy=dict(V_ldl=((3, 4), (4, 4), (255, 256), (1003, 1024), (1024, 1024), (2051, 2052)), n=37,
                       values=("normal3", "dominant_target", "dominant_other", "shift-3000", "bf16x5")),
    adamw=dict(n=(1, 3, 4, 10007, 2048 * 256 + 259), multi_n=MULTI_N, clip=("none", "max_norm0", "inactive", "active"),
               denom=(None, 4.0, 0.25), wd=(0.0, 0.1), steps=3),
)


@functools.lru_cache(maxsize=None)
def ln_case(H, M, in_bf16, rowscale, seed=0):
    x = rows_input(M, H, seed, layernorm_rows=True)
    x = x.to(BF16) if in_bf16 else x
    w, b = gamma_beta(H, seed)
    rs = rowscale_pattern(M) if rowscale else None
    return SimpleNamespace(x=x, w=w, b=b, rs=rs, eps=LN_EPS, exact=layernorm(x, w, b, LN_EPS, rs), model=layernorm(x, w, b, LN_EPS, rs, model=True))


@functools.lru_cache(maxsize=None)
def rms_case(H, M, in_bf16, gelu, seed=1):
    x = rows_input(M, H, seed)
    x = x.to(BF16) if in_bf16 else x
    w, _ = gamma_beta(H, seed)
    return SimpleNamespace(x=x, w=w, eps=RMS_EPS, exact=rmsnorm_fwd(x, w, RMS_EPS, gelu), model=rmsnorm_fwd(x, w, RMS_EPS, gelu, model=True))


def rms_bwd_inputs(H, M, seed=2):
    """x (planted), dy (random, row M // 2 zero when M >= 3), dres, w, a non-zero dw start, and the f32 rstd of the model's forward."""
    x = rows_input(M, H, seed)
    dy = rows_input(M, H, seed + 50, plant=False)
    if M >= 3:
        dy[M // 2] = 0.0
    dres = rows_input(M, H, seed + 60, plant=False)
    w, dw0 = gamma_beta(H, seed)
    return SimpleNamespace(x=x, dy=dy, dres=dres, w=w, dw0=dw0)


def rstd_of(x, eps=RMS_EPS):
    """The f32 rstd a backward kernel is handed: the model's forward on the bits of x."""
    return rmsnorm_fwd(x, torch.ones(x.shape[-1]), eps, model=True)["rstd"].float()


@functools.lru_cache(maxsize=None)
def lnres_case(H, M, with_keep_res, res_rows, eps, seed=3):
    g = _gen(H, M, seed, 5)
    z = rows_input(M, H, seed, layernorm_rows=True)
    gamma, beta = gamma_beta(H, seed)
    keep = res = None
    if with_keep_res:
        keep = (torch.rand(M, H, generator=g) > 0.2).float() * 1.25
        res = torch.randn(res_rows if res_rows > 0 else M, H, generator=g)
    fx = layernorm_res(z, keep, res, res_rows, gamma, beta, eps)
    fm = layernorm_res(z, keep, res, res_rows, gamma, beta, eps, model=True)
    dy = rows_input(M, H, seed + 50, plant=False)
    if M >= 3:
        dy[M // 2] = 0.0
    dg0, db0 = gamma_beta(H, seed + 9)
    xhat, rstd = fm["xhat"].float(), fm["rstd"].float()                        # the f32 bits the backward is handed
    bx = layernorm_bwd(dy, xhat, rstd, gamma, keep, dg0, db0)
    bm = layernorm_bwd(dy, xhat, rstd, gamma, keep, dg0, db0, model=True)
    return SimpleNamespace(z=z, keep=keep, res=res, res_rows=res_rows, gamma=gamma, beta=beta, eps=eps, fx=fx, fm=fm, dy=dy, dg0=dg0,
                           db0=db0, xhat=xhat, rstd=rstd, bx=bx, bm=bm)


def make_labels(B, L, kind, seed=4):
    """B lists of L integers.  none: all -100; all: every label valid; chunk_last: only the label that makes flat position 1023 (or
    the last position that has a target) valid; pos0: a valid label at every row's position 0 only; random: about half valid."""
    g = _gen(B, L, seed)
    val = torch.randint(0, 50000, (B, L), generator=g)
    lab = torch.full((B, L), -100, dtype=torch.long)
    if kind == "all":
        lab = val
    elif kind == "random":
        lab = torch.where(torch.rand(B, L, generator=g) < 0.5, val, lab)
    elif kind == "pos0":
        lab[:, 0] = val[:, 0]
    elif kind == "chunk_last":
        flat = lab.reshape(-1)
        cand = [p for p in range(B * L) if p % L + 1 < L and p <= 1023]
        if cand:
            flat[cand[-1] + 1] = val.reshape(-1)[cand[-1] + 1]
    return lab.tolist()


def ce_targets(n, V, ldl, seed=5):
    """n targets: column 0, column V-1, one in the V % 4 tail (or V-2), the invalid -100, V and ldl-1 (valid when ldl-1 < V), random."""
    g = _gen(n, V, seed)
    t = torch.randint(0, V, (n,), generator=g).tolist()
    fixed = {0: 0, 1: V - 1, 2: (V - V % 4 if V % 4 else max(V - 2, 0)), 3: -100, 4: V, 5: ldl - 1, n - 1: V - 1}
    for i, v in fixed.items():
        if i < n:
            t[i] = v
    return t


def ce_logits(R, V, ldl, kind, bf16, seed=6):
    """[R, ldl] logits, NaN in the padding columns.  kind: normal3 N(0, 3); dominant_target / dominant_other: one logit +40 above the
    rest (the caller places the target); shift-3000: all logits shifted by -3000; bf16x5: N(0, 1) * 5 rounded to bf16."""
    g = _gen(R, V, ldl, seed)
    z = torch.randn(R, ldl, generator=g) * (5.0 if kind == "bf16x5" else 3.0 if kind == "normal3" else 1.0)
    if kind.startswith("dominant"):
        z[torch.arange(R), torch.arange(R) % V] += 40.0
    if kind == "shift-3000":
        z -= 3000.0
    z[:, V:] = float("nan")
    return z.to(BF16) if bf16 else z

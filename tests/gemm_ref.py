"""CPU float64 reference of the matrix products of csrc/gemm.hip / csrc/gemm_common.h (``ta_gemm_bf16_nt_opt``) and csrc/gemm_tn.hip
(``ta_gemm_bf16_tn``), the inputs of the gates the tests put on them, and the case table.  A plain module (no fixtures):
``tests/test_gemm_ref.py`` checks it on the host, ``tests/test_gpu_gemm_grid.py`` compares every tile variant of the library with it.
The metric (``rb``, ``rf``, ``row_errors``, ``gate``, ``elem_gate``, ``last_place``, ``trunc_bf16``) is the one of tests/rowwise_ref.py,
imported, not copied.

Every operation is ONE function evaluated in two arithmetics (``model=False`` / ``model=True``):
  exact   float64 from the bf16 / f32 bits the kernel is given, no intermediate rounding.
  model   what a correct f32-accumulating kernel may deviate by, stated without looking at any output:
            * a product of two bf16 values is exact in f32 (8 x 8 mantissa bits);
            * the K sum is accumulated strictly left to right in f32, one k at a time (``ksum``); the K extension's columns come after K;
            * split-K: every slab (K tiles [nkt z / splits, nkt (z + 1) / splits) of 64 columns, gemm_common.h tile_ctx) is such a sum
              from zero, and the slabs are added in slab order onto the f32 residual (splitk_reduce_kernel);
            * the epilogue steps are rounded to f32 one by one in the kernel's order (epilogue_strip): bias, activation, residual,
              store;
            * a bf16 residual with act 0 and a bf16 output (no split-K) is not an epilogue addend but the START VALUE of the K sum
              (gemm_common.h residual_is_start): fl(..fl(fl(r + a0 w0) + a1 w1)..) + bias;
            * a bf16 output is the f32 value rounded to nearest even by the caller (``rb``): the functions return the value BEFORE it.
          Left to right over single k is the most error-prone order: the MFMA adds 32 products per instruction (tests/test_gemm_ref.py
          emulates that order -- every 32-wide k block summed exactly, one f32 rounding into the accumulator -- and finds it at
          0.27 - 0.33 of the model on the plain and bias forms, against the gate's factor 2; the MI355X measures 0.46 there,
          profiles/gemm_grid.md, so the instruction rounds more often than once per 32 products and less often than once per product).
  Every gate applies ``last_place`` (rowwise_ref: 1 ulp_f32 per element away from the exact value) to the model: a zero row of A
  with a bias, or a row of M = 1 products, is carried by single roundings the kernel is free to make differently (fma contraction in
  the rope and chord arithmetic).

erf-GELU: the operation IS the 1024-chord table of csrc/gelu_lut.h (y = a_i x + b_i, i = floor(clamp(64 x + 512, 0, 1023))), rebuilt
here from the formula of scripts/gen_gelu_lut.py (``gelu_chords``).  exact = the f32 chord coefficients applied in float64 with the
index of the exact pre-activation; model = the same in f32 with the index of the model's own f32 value.  The chords interpolate the
function at the segment ends, so they are continuous up to the f32 rounding of their coefficients (``chord_jump``: < 1e-6, about
one f32 ulp of the values there): an index that differs between the two forms next to a segment end moves an element by that.
How far the table is from erf-GELU (<= 2.5e-5, gemm_common.h) is checked once on the host, not gated per launch.

The a-priori bound (``apriori_bound``; the ``walk`` shapes, where a one-k-at-a-time loop over 2 x 10^7 outputs would take the host
seconds per form): for ANY order of f32 additions of n exactly representable terms t_i,  |fl(sum) - sum| <= g sum |t_i|,
g = (n - 1) u / (1 - (n - 1) u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 4.4).  The terms are the K
products, the bias and the start value.  Through the chord table: |chord(x^) - chord(x)| <= max |a_i| |x^ - x| + ``chord_jump`` (the
chords are piecewise linear and continuous up to that jump), plus two f32 roundings of the evaluation, each at most
u (|a x| + |y|) with |x| <= sum |t_i|, plus the index taken from fl(64 x + 512) < 1024, which is off by at most 2^-15, i.e. 2^-21
in x, times the largest slope step between neighbouring chords.  A residual added in the epilogue: one more rounding,
u (|y| + |r|).  A bf16 output: half a bf16 ulp of the larger of |got| and |exact|.  None of these figures comes from a kernel's
output; the f32 part of the bound stands four orders of magnitude below a dropped 32-wide k block, the bf16 half ulp two, and
unwritten memory is NaN.

Inputs (``nt_inputs``): seeded A ~ N(0, 1) and W ~ N(0, 1 / K) (A2 ~ N(0, 1), W2 ~ N(0, 1 / K2)), bias ~ N(0, 1) -- different in
every column, so a column shift cannot pass --, residual ~ N(0, 1), and planted rows of A (and A2) so that a normalisation over the
whole matrix would hide what the row gate sees: row 0 zero; row 1 scaled 1e-3; row 2 scaled 1e3 (it also drives GELU past both ends
of the table); row M-1 a spike of 1e3 at column K-1 (the last k of the last K tile).  ``tn_inputs`` plants the same in the COLUMNS of
Y, which are the rows of out = Y^T X.

CASES: the shapes of the grid, each with the code path it is the smallest shape for.
"""
import functools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

from tests.rowwise_ref import (F64, _gen, elem_gate, gate, last_place, rb, rf, row_errors, trunc_bf16, ulp_bf16)  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
BK = 64
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the chord table
@functools.lru_cache(maxsize=None)
def gelu_chords():
    """f32 [1024, 2] (slope, intercept): scripts/gen_gelu_lut.py's formula in float64 erf, written as that script writes it (the
    literal "%.8e", 9 significant digits) and rounded to f32 as the compiler reads the literal.  (41 of the 2048 numbers sit one f32
    ulp from the directly rounded double: the decimal step rounds first.)"""
    n, lo, hi = 1024, -8.0, 8.0
    h = (hi - lo) / n
    g = lambda x: 0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731
    rows = []
    for i in range(n):
        x0, x1 = lo + i * h, lo + (i + 1) * h
        a = (g(x1) - g(x0)) / h
        b = g(x0) - a * x0
        if i == 0:
            a, b = 0.0, 0.0
        if i == n - 1:
            a, b = 1.0, 0.0
        rows.append((float("%.8e" % a), float("%.8e" % b)))
    return torch.tensor(np.array(rows, dtype=np.float64).astype(np.float32))


def gelu_lut_header():
    """f32 [1024, 2]: the numbers of csrc/gelu_lut.h, read as text (each literal rounded to f32 as the compiler does)."""
    text = open(os.path.join(ROOT, "tiny_audio_amd", "csrc", "gelu_lut.h")).read()
    body = text[text.index("kGeluLut"):]
    vals = [np.float32(float(a)) for pair in re.findall(r"\{([^{}]+)\}", body) for a in pair.replace("f", "").split(",")]
    return torch.tensor(np.array(vals, dtype=np.float32).reshape(-1, 2))


def gelu_table(x, model=False):
    """The chord table at x (float64 tensor holding exact or f32 values)."""
    tab = gelu_chords()
    if model:
        xf = x.to(F32)
        t = (xf * 64.0 + 512.0).clamp(0.0, 1023.0)                          # fmaf: 64 x is exact, one rounding either way
        i = t.to(torch.int64)
        return (tab[i, 0] * xf + tab[i, 1]).to(F64)
    i = (x * 64.0 + 512.0).clamp(0.0, 1023.0).to(torch.int64)
    t64 = tab.to(F64)
    return t64[i, 0] * x + t64[i, 1]


@functools.lru_cache(maxsize=None)
def chord_jump():
    """The largest step between neighbouring chords at their common segment end (0 in exact arithmetic; the coefficients are f32)."""
    t = gelu_chords().to(F64)
    ends = (torch.arange(1, 1024, dtype=F64) - 512) / 64
    return float(((t[:-1, 0] * ends + t[:-1, 1]) - (t[1:, 0] * ends + t[1:, 1])).abs().max())


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ----------------------------------------------------------------------------- pieces of the operation
def ksum(acc, A, W, k0=0, k1=None):
    """acc (f32 [M, N], changed in place) += sum_{k0 <= k < k1} A[:, k] W[:, k]^T, one k at a time, left to right, in f32."""
    Af, Wt = A.to(F32), W.to(F32).t().contiguous()
    k1 = A.shape[1] if k1 is None else k1
    for k in range(k0, k1):
        acc += Af[:, k:k + 1] * Wt[k:k + 1]                                  # the product is exact in f32; the add rounds
    return acc


def mfma_sum(acc, A, W, k0=0, k1=None):
    """The order of v_mfma_f32_16x16x32_bf16: every 32-wide k block summed exactly, then one f32 rounding into the accumulator."""
    A64, W64 = A.to(F64), W.to(F64)
    k1 = A.shape[1] if k1 is None else k1
    assert (k1 - k0) % 32 == 0
    for k in range(k0, k1, 32):
        acc = (acc.to(F64) + A64[:, k:k + 32] @ W64[:, k:k + 32].t()).to(F32)
    return acc


def split_ranges(K, splits):
    """The K ranges of the slabs (gemm_common.h tile_ctx); the entry point clamps splits to the K tile count."""
    nkt = K // BK
    s = max(1, min(int(splits), nkt))
    return [((nkt * z) // s * BK, (nkt * (z + 1)) // s * BK) for z in range(s)]


def rope_il(v, tab, rope_rows, rope_cols, row_of=None, col_limit=True):
    """act 2: heads of 64 columns, the first 32 hold the 16 rotation pairs interleaved (pair i = columns 2i, 2i+1); tab
    [rope_rows, 16, 2] = (cos, sin) of pair i at position (row % rope_rows); columns >= rope_cols are left alone.  Works in the
    dtype of v (every product and sum rounded when that is f32).  ``row_of`` / ``col_limit``: test instrumentation (the mutants)."""
    M, N = v.shape
    rows = (torch.arange(M) % rope_rows) if row_of is None else row_of
    n = torch.arange(N)
    sel = ((n & 63) < 32) & ((n < rope_cols) if col_limit else torch.ones(N, dtype=torch.bool))
    ev = sel & ((n & 1) == 0)
    cols = n[ev]
    pair = (cols & 63) >> 1
    t = tab.to(v.dtype)[rows][:, pair]                                      # [M, n_pairs, 2]
    c, s = t[..., 0], t[..., 1]
    a0, a1 = v[:, cols], v[:, cols + 1]
    out = v.clone()
    out[:, cols] = a0 * c - a1 * s
    out[:, cols + 1] = a1 * c + a0 * s
    return out


def is_start(act, res, out_bf16, splits=1):
    return res is not None and res.dtype == BF16 and act == 0 and out_bf16 and splits == 1


def epilogue(acc, bias=None, act=0, res=None, rope=None, start=False, model=False, mut=None):
    """acc -> the value before the store's rounding: bias, activation, residual (unless it was the start value).  ``mut``: the host
    test's mutants (bias_shift, rope_row, rope_col, res_twice)."""
    dt = F32 if model else F64
    mut = mut or {}
    v = acc.to(dt)
    if bias is not None:
        b = bias.to(dt)
        v = v + (torch.roll(b, mut["bias_shift"]) if "bias_shift" in mut else b)
    if act == 1:
        v = gelu_table(v.to(F64), model).to(dt)
    elif act == 2:
        tab, rr, rc = rope
        rc = rc if rc > 0 else v.shape[1]
        v = rope_il(v, tab, rr, rc, row_of=(torch.arange(v.shape[0]) % tab.shape[0]) if mut.get("rope_row") else None,
                    col_limit=not mut.get("rope_col"))
    if res is not None and not start:
        v = v + res.to(dt)
        if "res_twice" in mut:
            r0 = mut["res_twice"]
            v[r0:r0 + 16] = v[r0:r0 + 16] + res.to(dt)[r0:r0 + 16]
    return v.to(F64)


def gemm_nt(A, W, bias=None, act=0, res=None, rope=None, A2=None, W2=None, splits=1, out_bf16=False, model=False, summer=None,
            mut=None):
    """ta_gemm_bf16_nt_opt on A [M, K] (the rows the row map reads, in logical order), W [N, K] (plain layout): the float64 value
    before the store's rounding.  res: f32 or bf16 [M, N]; rope = (tab, rope_rows, rope_cols).  ``summer``: the K-sum of the model
    form (default ``ksum``; tests/test_gemm_ref.py passes ``mfma_sum``).  ``mut``: mutants, see ``epilogue`` (+ drop_slab)."""
    M, K = A.shape
    N = W.shape[0]
    start = is_start(act, res, out_bf16, splits)
    mut = mut or {}
    if not model:
        acc = A.to(F64) @ W.to(F64).t()
        if A2 is not None:
            acc = acc + A2.to(F64) @ W2.to(F64).t()
        if start:
            acc = acc + res.to(F64)
        return epilogue(acc, bias, act, res, rope, start, False)
    summer = summer or ksum
    if splits > 1 and len(split_ranges(K, splits)) > 1:
        assert A2 is None and bias is None and act == 0 and (res is None or res.dtype == F32)
        total = res.to(F32).clone() if res is not None else torch.zeros(M, N, dtype=F32)
        for z, (k0, k1) in enumerate(split_ranges(K, splits)):
            if mut.get("drop_slab") == z:
                continue
            total = total + summer(torch.zeros(M, N, dtype=F32), A, W, k0, k1)
        return total.to(F64)
    acc = res.to(F32).clone() if start else torch.zeros(M, N, dtype=F32)
    acc = summer(acc, A, W)
    if A2 is not None:
        acc = summer(acc, A2, W2)
    return epilogue(acc, bias, act, res, rope, start, True, mut)


def gemm_tn(Y, X, start=None, model=False):
    """ta_gemm_bf16_tn: out [Ny, Nx] = (start or 0) + Y[M, Ny]^T X[M, Nx].  Model: the M products of an element added one row at a
    time, left to right, onto the start value (the kernel adds 32 rows per MFMA into row-chunk slabs and the slabs in order)."""
    if not model:
        out = Y.to(F64).t() @ X.to(F64)
        return out + start.to(F64) if start is not None else out
    acc = start.to(F32).clone() if start is not None else torch.zeros(Y.shape[1], X.shape[1], dtype=F32)
    return ksum(acc, Y.t(), X.t()).to(F64)


def pack_w_blocked(W):
    """[N, K] -> [N/64][K/64][64][64] blocks (ta_gemm_opts.w_blocked), flat."""
    N, K = W.shape
    return W.view(N // 64, 64, K // 64, 64).permute(0, 2, 1, 3).contiguous().reshape(-1)


def unpack_w_blocked(Wb, N, K):
    return Wb.view(N // 64, K // 64, 64, 64).permute(0, 2, 1, 3).contiguous().reshape(N, K)


def map_rows(buf, M, K, ld, rpb, bs):
    """The A rows a row map reads: logical row m starts at element (m // rpb) * bs + (m % rpb) * ld of the flat buffer."""
    m = torch.arange(M)
    off = (m // rpb) * bs + (m % rpb) * ld if rpb > 0 else m * ld
    return buf.reshape(-1)[off[:, None] + torch.arange(K)[None]]


def map_out_rows(M, ld, rpb, bs, off):
    """The first element of every logical output row under C's row map."""
    m = torch.arange(M)
    return off + ((m // rpb) * bs + (m % rpb) * ld if rpb > 0 else m * ld)


def apriori_bound(exact, absprod, K, bias=None, act=0, res=None, start=False, out_bf16=False, got=None):
    """Element-wise bound on |got - exact| for any f32 summation order (module docstring).  absprod = |A| |W|^T (float64), K the
    number of products per element."""
    S, n = absprod.clone(), K
    if start:
        S, n = S + res.to(F64).abs(), n + 1
    if bias is not None:
        S, n = S + bias.to(F64).abs()[None], n + 1
    g = (n - 1) * U / (1 - (n - 1) * U)
    b = g * S
    if act == 1:
        tab = gelu_chords().to(F64)
        amax, astep = float(tab[:, 0].abs().max()), float((tab[1:, 0] - tab[:-1, 0]).abs().max())
        b = amax * b + chord_jump() + 2.0 ** -21 * astep + 2 * U * (amax * S + exact.abs())            # two roundings, each of at most |a x| + |y|, |x| <= S
    if res is not None and not start:
        b = b + U * (exact.abs() + res.to(F64).abs())
    if out_bf16:
        b = b + 0.5 * ulp_bf16(torch.maximum(got.to(F64).abs(), exact.abs()) if got is not None else exact.abs())
    return b


# ----------------------------------------------------------------------------- the gates (host test and GPU test alike)
def gates(got, exact, pre, width, out_bf16):
    """The checks one output gets: [(name, passes, ratio, worst row)].  ``pre``: the model before the store's rounding.
    rows: max_r e_r <= 2 max_r m_r with ``last_place`` applied to the model; bf16 outputs: also ``elem_gate``."""
    got = got.detach().cpu().to(F64)
    pre = last_place(pre, exact)
    model = rb(pre) if out_bf16 else pre
    bound = float(row_errors(model, exact, width).max())
    assert 0 < bound < float("inf"), "the model does not deviate"
    ok, ratio, w = gate(got, exact, model, factor=2.0, width=width)
    out = [("rows", ok, ratio, w)]
    if out_bf16:
        ok, ratio, w = elem_gate(got, exact, pre, width)
        out.append(("elem", ok, ratio, w // width))
    return out


# ----------------------------------------------------------------------------- inputs
def plant(A):
    """The planted rows (module docstring), in place, while a random row is left."""
    M, K = A.shape
    if M >= 5:
        A[0] = 0.0
        A[1] *= 1e-3
        A[2] *= 1e3
        A[M - 1, K - 1] = 1e3
    return A


@functools.lru_cache(maxsize=None)
def nt_inputs(M, N, K, K2=0, seed=0):
    g = _gen(M, N, K, K2, seed)
    A = plant(torch.randn(M, K, generator=g)).to(BF16)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF16)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    out = SimpleNamespace(M=M, N=N, K=K, K2=K2, A=A, W=W, bias=bias, res=res, resb=res.to(BF16), A2=None, W2=None)
    if K2:
        out.A2 = plant(torch.randn(M, K2, generator=g)).to(BF16)
        out.W2 = (torch.randn(N, K2, generator=g) / math.sqrt(K2)).to(BF16)
    return out


@functools.lru_cache(maxsize=None)
def rope_table(rows, theta=10000.0):
    """f32 [rows, 16, 2] (cos, sin): the GLM-ASR partial rotary table (rotary dim 32)."""
    inv = 1.0 / (theta ** (torch.arange(0, 32, 2, dtype=F32) / 32))
    f = torch.arange(rows, dtype=F32)[:, None] * inv[None]
    return torch.stack([f.cos(), f.sin()], -1).contiguous()


def il_perm():
    """column p of a head <- head dim (the interleaved rotary layout of ta_gemm_opts.rope_tab)."""
    p = torch.arange(64)
    return torch.where(p < 32, (p >> 1) + 16 * (p & 1), p)


@functools.lru_cache(maxsize=None)
def conv_inputs(B=3, T=37, Cin=128, Cout=256, seed=7):
    """Conv1d(k = 3, pad = 1) as a row-mapped GEMM over a zero-padded time-major buffer xp [B, T + 2, Cin]; planted FRAMES: clip 1's
    frames 0..2 zero (output row t = 1 of clip 1 is a zero row of A at stride 1), clip 0's frame 5 scaled 1e-3, frame 9 scaled 1e3."""
    g = _gen(B, T, Cin, Cout, seed)
    x = torch.randn(B, T, Cin, generator=g)
    x[1, 0:3] = 0.0
    x[0, 5] *= 1e-3
    x[0, 9] *= 1e3
    xp = torch.zeros(B, T + 2, Cin, dtype=BF16)
    xp[:, 1:T + 1] = x.to(BF16)
    w = (torch.randn(Cout, Cin, 3, generator=g) / math.sqrt(3 * Cin))
    wp = w.permute(0, 2, 1).reshape(Cout, 3 * Cin).to(BF16).contiguous()
    bias = torch.randn(Cout, generator=g)
    return SimpleNamespace(B=B, T=T, Cin=Cin, Cout=Cout, xp=xp, wp=wp, bias=bias)


def conv_map(c, stride):
    """(M, a_map = (lda, a_rpb, a_bs)) of the convolution at ``stride``."""
    S = (c.T + 2 - 3) // stride + 1
    return c.B * S, (stride * c.Cin, S, (c.T + 2) * c.Cin)


@functools.lru_cache(maxsize=None)
def tn_inputs(M, Ny, Nx, seed=11):
    g = _gen(M, Ny, Nx, seed)
    Y = torch.randn(max(M, 1), Ny, generator=g)[:M]
    X = torch.randn(max(M, 1), Nx, generator=g)[:M]
    Y[:, 0] = 0.0
    Y[:, 1] *= 1e-3
    Y[:, 2] *= 1e3
    return SimpleNamespace(Y=Y.to(BF16).contiguous(), X=X.to(BF16).contiguous(), start=torch.randn(Ny, Nx, generator=g))


# ----------------------------------------------------------------------------- the forms of the grid
def F(name, **kw):
    d = dict(bias=False, act=0, res=None, inplace=False, out_bf16=False, K2=0, splits=1, rope_cols=None, blocked=False)
    d.update(kw)
    return SimpleNamespace(name=name, **d)


def _both(name, **kw):
    return [F(name + "-f32", out_bf16=False, **kw), F(name + "-bf16", out_bf16=True, **kw)]


EDGE_FORMS = (
    _both("plain") + _both("bias", bias=True) + _both("bias+gelu", bias=True, act=1)
    + [F("bias+resf32-f32", bias=True, res="f32"), F("bias+resf32-inplace-f32", bias=True, res="f32", inplace=True),
       F("resf32-bf16", res="f32", out_bf16=True),
       F("resbf16-inplace-bf16", res="bf16", inplace=True, out_bf16=True),          # the start value
       F("resbf16-f32", res="bf16"),
       F("gelu+resbf16-bf16", act=1, res="bf16", out_bf16=True)]
    + [f for k2 in (64, 128) for f in (F(f"kext{k2}-f32", K2=k2), F(f"kext{k2}+resf32-f32", K2=k2, res="f32"),
                                       F(f"kext{k2}-bf16", K2=k2, out_bf16=True))]
    + [F(f"splitk{s}{'+resf32' if r else ''}-{'bf16' if ob else 'f32'}", splits=s, res=r, out_bf16=ob)
       for s in (2, 3, 5) for r in (None, "f32") for ob in (False, True)]
)
ROPE_FORMS = [F("rope-all", bias=True, act=2, out_bf16=True, rope_cols=0), F("rope-128", bias=True, act=2, out_bf16=True, rope_cols=128),
              F("blocked-f32", blocked=True), F("blocked-bf16", blocked=True, out_bf16=True),
              F("blocked+bias-f32", blocked=True, bias=True), F("blocked+bias-bf16", blocked=True, bias=True, out_bf16=True)]
FULL_FORMS = _both("bias", bias=True) + _both("bias+gelu", bias=True, act=1) + [F("resbf16-inplace-bf16", res="bf16", inplace=True, out_bf16=True)]
WALK_FORMS = [F("bias-bf16", bias=True, out_bf16=True), F("resbf16-inplace-bf16", res="bf16", inplace=True, out_bf16=True),
              F("bias+gelu-bf16", bias=True, act=1, out_bf16=True)]
VARIANTS = (None, 0, 3, 4, 5, 10, 12)
TILES = {0: (128, 128), 3: (256, 256), 4: (256, 320), 5: (96, 128), 10: (192, 128), 12: (192, 256)}

CASES = dict(
    # every tile has a partial last row strip (203 = 192 + 11) and a partial column tile; N % 8 = 4: narrow bf16 stores, N % 8 = 0:
    # wide ones with an 8-column last tile for 256x320; 3 and 2 K tiles (odd / even stage parity; splits = 5 clamps to 2 at K = 128)
    edge=dict(shapes=((203, 332, 192), (203, 328, 128)), forms=EDGE_FORMS),
    # m % rope_rows wraps four times and ends mid-period; N % 64 == 0 as act 2 and blocked W require
    rope=dict(shapes=((203, 384, 128),), rope_rows=50, forms=ROPE_FORMS),
    # 768 / 1280 are common multiples of all tile heights / widths: full tiles (epilogue_tile_full in the persistent kernel) and
    # partial edge tiles in one launch; ONE K tile: the epilogue constants ride behind the only K tile
    full=dict(shapes=((773, 1288, 64),), forms=FULL_FORMS),
    # more tiles than CUs, fewer than twice as many, for the persistent variants: the tile-to-tile transition of gemm_nt_kernel_v4,
    # stage parity staying (K = 128) and flipping (K = 64); 17 row tiles leave a last tile-order group of one row tile
    walk=dict(M=4100, N={3: 4096, 12: 4096, 4: 5120}, K=(64, 128), forms=WALK_FORMS),
    maps=dict(B=3, T=37, strides=(1, 2)),
    # the second batch's rows start 2^32 bytes into A: V_FAR_A
    far=dict(M=256, N=136, K=128, a_rpb=128, a_bs=2 ** 31),
    tn=dict(M=(1, 31, 32, 33, 64, 65, 97, 300), NyNx=((8, 8), (136, 264), (128, 256))),
)


@functools.lru_cache(maxsize=None)
def nt_case(M, N, K, form_name, forms_key, rope_rows=0):
    """Inputs, exact and model (before the store's rounding) of one (shape, form); shared by every variant."""
    f = next(x for x in CASES[forms_key]["forms"] if x.name == form_name)
    i = nt_inputs(M, N, K, f.K2)
    res = None if f.res is None else (i.res if f.res == "f32" else i.resb)
    rope = (rope_table(256), rope_rows, f.rope_cols) if f.act == 2 else None        # (only the first rope_rows rows may be read)
    kw = dict(bias=i.bias if f.bias else None, act=f.act, res=res, rope=rope, A2=i.A2, W2=i.W2, splits=f.splits, out_bf16=f.out_bf16)
    return SimpleNamespace(f=f, i=i, res=res, rope=rope, kw=kw, exact=gemm_nt(i.A, i.W, **kw), pre=gemm_nt(i.A, i.W, model=True, **kw))

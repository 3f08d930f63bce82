"""-m gpu: the row-wise kernels around the GEMMs -- csrc/norm.hip, the LayerNorm(z * keep + res) pair of csrc/nn_prims.hip,
csrc/loss.hip and csrc/optim.hip -- against the float64 reference of tests/rowwise_ref.py, row by row, at the smallest shapes that
reach each code path (rowwise_ref.CASES) and over the planted rows of rowwise_ref.rows_input.

Gates (rowwise_ref): every floating output  max_r e_r <= 2 max_r m_r  (a vector is one row), every bf16 output also element by element
(|got - exact| <= ulp_bf16 / 2 + 2 a_r: nearest-even against truncation), scalars |got - exact| <= 2 |model - exact|, integers and
the outputs the operation defines exactly with ==.  No element and no row is excluded.  The model every gate uses carries the three
derived terms of rowwise_ref's docstring: the 1-ulp rsqrt, ``last_place`` and, for outputs accumulated with float atomics, ``unordered``.
Every entry point is called through the C ABI so that the outputs can be prepared: pre-filled with 0xFF bytes (NaN as bf16 and f32,
-1 as an integer), per-row outputs with 8 extra rows and per-column outputs with 8 extra columns holding 7.0, which must still hold
7.0 afterwards.  Every check prints  ``ROWGRID <entry point> <case> <tensor> e/m=<ratio> worst=<row>``; a test reports all of its
failed checks at its end.  The measured table is profiles/rowwise_grid.md.
"""
import ctypes as C

import pytest
import torch

from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OK, ERR_ARG = 0, 1
OUTS = ("bf16", "f32", "both")


def lib():
    return _lib.lib()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_KEEP = []


@pytest.fixture(autouse=True)
def _inputs_stay_alive():
    """Device copies made by ``dev`` live until the end of the test: their pointers are handed to asynchronous launches."""
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(t, dtype=None):
    if t is None:
        return None
    _KEEP.append((t.to(dtype) if dtype is not None else t).to(DEV).contiguous())
    return _KEEP[-1]


class Guarded:
    """An output of ``n`` rows (or, 1-D, n elements) followed by 8 guard rows (elements) of 7.0.  ``start``: initial contents (an
    accumulated or aliased output); otherwise 0xFF bytes."""

    def __init__(self, n, width=None, dtype=F32, start=None):
        shape = (n + 8,) if width is None else (n + 8, width)
        self.n, self.full = n, torch.full(shape, 7.0 if dtype.is_floating_point else 7, device=DEV, dtype=dtype)
        if start is not None:
            self.full[:n] = start.to(DEV).to(dtype)
        else:
            self.full[:n].view(torch.uint8).fill_(0xFF)

    @property
    def p(self):
        return ptr(self.full)

    def get(self):
        """The output on the host; asserts the guard."""
        torch.cuda.synchronize()
        assert bool((self.full[self.n:] == 7).all()), "guard rows / columns overwritten"
        return self.full[:self.n].cpu()


class Checks:
    def __init__(self, ep):
        self.ep, self.bad = ep, []

    def rows(self, case, name, got, exact, pre, width, bf16=False, unordered=0):
        """The row gate; for a bf16 output (``pre``: the model before its rounding) also the element gate.  ``unordered``: the number
        of rows an atomically accumulated output adds in an unspecified order."""
        got, pre = got.detach().cpu().to(F64), R.last_place(pre, exact)
        if unordered:
            pre = R.unordered(pre, exact, unordered)
        model = R.rb(pre) if bf16 else pre
        bound = float(R.row_errors(model, exact, width).max())
        assert bound > 0 and bound < float("inf"), (self.ep, case, name, "the model does not deviate")
        ok, ratio, w = R.gate(got, exact, model, factor=2.0, width=width)
        print(f"ROWGRID {self.ep} {case} {name} e/m={ratio:.3f} worst={w}")
        if not ok:
            self.bad.append((case, name, "rows", ratio, w))
        if bf16:
            ok, ratio, w = R.elem_gate(got, exact, pre, width)
            print(f"ROWGRID {self.ep} {case} {name}.elem e/m={ratio:.3f} worst={w // width}")
            if not ok:
                self.bad.append((case, name, "elem", ratio, w))

    def scalar(self, case, name, got, exact, model, unordered=0):
        model = R.last_place(model, exact)
        if unordered:
            model = R.unordered(model, exact, unordered)
        ok, ratio = R.scalar_gate(got, exact, float(model))
        print(f"ROWGRID {self.ep} {case} {name} e/m={ratio:.3f} worst=0")
        if not ok:
            self.bad.append((case, name, "scalar", ratio, float(got), float(exact), float(model)))

    def equal(self, case, name, cond):
        if not cond:
            self.bad.append((case, name, "=="))

    def done(self):
        assert not self.bad, (self.ep, self.bad)


def call(fn, *args, expect=OK):
    st = getattr(lib(), fn)(*args)
    assert st == expect, (fn, st)


def outs_of(M, H, outs, start_b=None):
    yb = Guarded(M, H, BF16, start_b) if outs in ("bf16", "both") else None
    yf = Guarded(M, H, F32) if outs in ("f32", "both") else None
    return yb, yf


def p_(g):
    return None if g is None else g.p


# ----------------------------------------------------------------------------- LayerNorm
def run_ln(ck, c, M, H, bf, outs, case):
    fn = "ta_layernorm_bf16" if bf else "ta_layernorm_f32"
    x, w, b, rs = dev(c.x), dev(c.w), dev(c.b), dev(c.rs)
    yb, yf = outs_of(M, H, outs)
    call(fn, ptr(x), ptr(w), ptr(b), p_(yb), p_(yf), ptr(rs), M, H, c.eps, stream())
    for y, is_b in ((yb, True), (yf, False)):
        if y is None:
            continue
        got = y.get()
        ck.rows(case, "y_bf16" if is_b else "y_f32", got, c.exact["y"], c.model["y"], H, bf16=is_b)
        if c.rs is not None:
            ck.equal(case, "rowscale=0 rows", not got[c.rs == 0].float().any())


@pytest.mark.parametrize("H", R.HS_FWD)
def test_layernorm(H):
    for bf in (False, True):
        ck = Checks("ta_layernorm_bf16" if bf else "ta_layernorm_f32")
        for M in R.CASES["layernorm"]["M"]:
            for rs in (False, True):
                c = R.ln_case(H, M, bf, rs)
                for outs in OUTS:
                    run_ln(ck, c, M, H, bf, outs, f"H{H}-M{M}-{'rs' if rs else 'nors'}-{outs}")
        ck.done()


@pytest.mark.parametrize("M", R.CASES["layernorm"]["walk_M"])
def test_layernorm_half_wave_walk(M):
    """2 rows per half wave from M = 4096 and 4 from M = 8192: walks that end in the middle of a half wave's rows."""
    for H, rs in ((256, True), (1280, False)):
        for bf in (False, True):
            ck = Checks("ta_layernorm_bf16" if bf else "ta_layernorm_f32")
            c = R.ln_case.__wrapped__(H, M, bf, rs)                          # (not cached: 8195 x 1280 in float64)
            run_ln(ck, c, M, H, bf, "bf16", f"walk-H{H}-M{M}-{'rs' if rs else 'nors'}")
            ck.done()


def test_layernorm_argument_errors():
    M = 3
    for fn, dt in (("ta_layernorm_f32", F32), ("ta_layernorm_bf16", BF16)):
        x = torch.zeros(M, 5124, device=DEV, dtype=dt)
        w = torch.ones(5124, device=DEV)
        yb, yf = Guarded(M, 5124, BF16), Guarded(M, 5124, F32)
        for H, ob, of in ((6, yb, yf), (5124, yb, yf), (256, None, None)):
            call(fn, ptr(x), ptr(w), ptr(w), p_(ob), p_(of), None, M, H, 1e-5, stream(), expect=ERR_ARG)
        assert bool((yb.get().view(torch.int16) == -1).all()) and bool((yf.get().view(torch.int32) == -1).all())


# ----------------------------------------------------------------------------- RMSNorm forward
@pytest.mark.parametrize("H", R.HS_FWD)
def test_rmsnorm_fwd(H):
    for bf, gelu in ((False, False), (False, True), (True, False)):
        fn = "ta_rmsnorm_fwd_bf16" if bf else "ta_rmsnorm_fwd"
        ck = Checks(fn)
        for M in R.CASES["rmsnorm_fwd"]["M"]:
            c = R.rms_case(H, M, bf, gelu)
            x, w = dev(c.x), dev(c.w)
            for outs in OUTS + ("bf16-norstd",):
                case = f"H{H}-M{M}-{'gelu' if gelu else 'lin'}-{outs}"
                yb, yf = outs_of(M, H, outs.split("-")[0])
                rstd = None if outs.endswith("norstd") else Guarded(M)
                tail = (M, H, c.eps) + ((int(gelu),) if not bf else ()) + (stream(),)
                call(fn, ptr(x), ptr(w), p_(yb), p_(yf), p_(rstd), *tail)
                for y, is_b in ((yb, True), (yf, False)):
                    if y is not None:
                        got = y.get()
                        ck.rows(case, "y_bf16" if is_b else "y_f32", got, c.exact["y"], c.model["y"], H, bf16=is_b)
                        if M > 1:
                            ck.equal(case, "zero row", not got[0].float().any())
                if rstd is not None:
                    ck.rows(case, "rstd", rstd.get(), c.exact["rstd"], c.model["rstd"], M)
        ck.done()


# ----------------------------------------------------------------------------- RMSNorm backward
def bwd_outs(ck, case, dxb, dxf, e, m, H):
    if dxb is not None:
        ck.rows(case, "dx_bf16", dxb.get(), e["dx"], m["dx"], H, bf16=True)
    if dxf is not None:
        ck.rows(case, "dx_f32", dxf.get(), e["dx"], m["dx"], H)


def refs(*a, **kw):
    return R.rmsnorm_bwd(*a, **kw), R.rmsnorm_bwd(*a, model=True, **kw)


@pytest.mark.parametrize("H", R.HS_BWD)
def test_rmsnorm_bwd(H):
    cks = {n: Checks(n) for n in ("ta_rmsnorm_bwd", "ta_rmsnorm_bwd_bf16", "ta_rmsnorm_bwd_bf16s", "ta_rmsnorm_bwd_dyb")}
    for M in R.CASES["rmsnorm_bwd"]["M"]:
        I = R.rms_bwd_inputs(H, M)
        xf, xb, dyf, dyb = I.x, I.x.to(BF16), I.dy, I.dy.to(BF16)
        dresf, dresb = I.dres, I.dres.to(BF16)
        rf_, rb_ = R.rstd_of(xf), R.rstd_of(xb)
        w = dev(I.w)
        D = {id(t): dev(t) for t in (xf, xb, dyf, dyb, dresf, dresb, rf_, rb_)}
        d = lambda t: None if t is None else D[id(t)]
        # ta_rmsnorm_bwd: f32 everywhere, GELU, dw accumulated onto a non-zero start
        ck = cks["ta_rmsnorm_bwd"]
        for gelu in (False, True):
            for dres in (None, dresf):
                e, m = refs(dyf, xf, rf_, I.w, dres, gelu, I.dw0)
                for outs in OUTS:
                    case = f"H{H}-M{M}-{'gelu' if gelu else 'lin'}-{'dres' if dres is not None else 'nodres'}-{outs}"
                    dxb, dxf = outs_of(M, H, outs)
                    dw = Guarded(H, None, F32, I.dw0)
                    call("ta_rmsnorm_bwd", ptr(d(dyf)), ptr(d(xf)), ptr(d(rf_)), ptr(w), ptr(d(dres)), p_(dxf), p_(dxb), dw.p, M, H, int(gelu), stream())
                    bwd_outs(ck, case, dxb, dxf, e, m, H)
                    ck.rows(case, "dw", dw.get(), e["dw"], m["dw"], H, unordered=M)
        dxf, dw = Guarded(M, H, F32), Guarded(H, None, F32, I.dw0)               # an all-zero dy: dw keeps its start exactly
        zero = dev(torch.zeros(M, H))
        call("ta_rmsnorm_bwd", ptr(zero), ptr(d(xf)), ptr(d(rf_)), ptr(w), None, dxf.p, None, dw.p, M, H, 0, stream())
        ck.equal(f"H{H}-M{M}-zero-dy", "dw", torch.equal(dw.get(), I.dw0) and not dxf.get().any())
        # ta_rmsnorm_bwd_bf16: x bf16, dy f32 / bf16, dres f32
        ck = cks["ta_rmsnorm_bwd_bf16"]
        for dy in (dyf, dyb):
            for dres in (None, dresf):
                e, m = refs(dy, xb, rb_, I.w, dres)
                for outs in OUTS:
                    case = f"H{H}-M{M}-dy{'b' if dy is dyb else 'f'}-{'dres' if dres is not None else 'nodres'}-{outs}"
                    dxb, dxf = outs_of(M, H, outs)
                    call("ta_rmsnorm_bwd_bf16", ptr(d(dy)), int(dy is dyb), ptr(d(xb)), ptr(d(rb_)), ptr(w), ptr(d(dres)), p_(dxf), p_(dxb), M, H, stream())
                    bwd_outs(ck, case, dxb, dxf, e, m, H)
        # ta_rmsnorm_bwd_bf16s: dres bf16, possibly the bf16 output itself
        ck = cks["ta_rmsnorm_bwd_bf16s"]
        for dy in (dyf, dyb):
            for dres in ("none", "given", "aliased"):
                e, m = refs(dy, xb, rb_, I.w, None if dres == "none" else dresb)
                for outs in (OUTS if dres != "aliased" else ("bf16", "both")):
                    case = f"H{H}-M{M}-dy{'b' if dy is dyb else 'f'}-dres-{dres}-{outs}"
                    dxb, dxf = outs_of(M, H, outs, start_b=dresb if dres == "aliased" else None)
                    pd = None if dres == "none" else (dxb.p if dres == "aliased" else ptr(d(dresb)))
                    call("ta_rmsnorm_bwd_bf16s", ptr(d(dy)), int(dy is dyb), ptr(d(xb)), ptr(d(rb_)), ptr(w), pd, p_(dxf), p_(dxb), M, H, stream())
                    bwd_outs(ck, case, dxb, dxf, e, m, H)
        # ta_rmsnorm_bwd_dyb: x f32, dy bf16, dres f32
        ck = cks["ta_rmsnorm_bwd_dyb"]
        for dres in (None, dresf):
            e, m = refs(dyb, xf, rf_, I.w, dres)
            for outs in OUTS:
                case = f"H{H}-M{M}-{'dres' if dres is not None else 'nodres'}-{outs}"
                dxb, dxf = outs_of(M, H, outs)
                call("ta_rmsnorm_bwd_dyb", ptr(d(dyb)), ptr(d(xf)), ptr(d(rf_)), ptr(w), ptr(d(dres)), p_(dxf), p_(dxb), M, H, stream())
                bwd_outs(ck, case, dxb, dxf, e, m, H)
    for ck in cks.values():
        ck.done()


@pytest.mark.parametrize("gelu", [False, True])
def test_rmsnorm_bwd_dw_block_cap(gelu):
    """With dw the grid is capped at 512 blocks of 4 rows: at M = 4100 every block strides and the last group of rows is ragged."""
    M, H = R.CASES["rmsnorm_bwd"]["cap"]
    I = R.rms_bwd_inputs(H, M)
    r = R.rstd_of(I.x)
    e, m = refs(I.dy, I.x, r, I.w, I.dres, gelu, I.dw0)
    ck = Checks("ta_rmsnorm_bwd")
    dxb, dxf, dw = Guarded(M, H, BF16), Guarded(M, H, F32), Guarded(H, None, F32, I.dw0)
    call("ta_rmsnorm_bwd", ptr(dev(I.dy)), ptr(dev(I.x)), ptr(dev(r)), ptr(dev(I.w)), ptr(dev(I.dres)), dxf.p, dxb.p, dw.p, M, H, int(gelu), stream())
    case = f"cap-H{H}-M{M}-{'gelu' if gelu else 'lin'}"
    bwd_outs(ck, case, dxb, dxf, e, m, H)
    ck.rows(case, "dw", dw.get(), e["dw"], m["dw"], H, unordered=M)
    ck.done()


def test_rmsnorm_dw():
    ck = Checks("ta_rmsnorm_dw")
    for M, H in R.CASES["rmsnorm_dw"]["MH"]:
        I = R.rms_bwd_inputs(H, M, seed=7)
        for dyb in (False, True):
            for xb in (False, True):
                x, dy = (I.x.to(BF16) if xb else I.x), (I.dy.to(BF16) if dyb else I.dy)
                r = R.rstd_of(x)
                e, m = R.rmsnorm_dw(dy, x, r, I.dw0), R.rmsnorm_dw(dy, x, r, I.dw0, model=True)
                dw = Guarded(H, None, F32, I.dw0)
                call("ta_rmsnorm_dw", ptr(dev(dy)), int(dyb), ptr(dev(x)), int(xb), ptr(dev(r)), dw.p, M, H, stream())
                ck.rows(f"M{M}-H{H}-dy{'b' if dyb else 'f'}-x{'b' if xb else 'f'}", "dw", dw.get(), e["dw"], m["dw"], H, unordered=M)
        dw = Guarded(H, None, F32, I.dw0)
        zero, r = dev(torch.zeros(M, H)), dev(R.rstd_of(I.x))
        call("ta_rmsnorm_dw", ptr(zero), 0, ptr(dev(I.x)), 0, ptr(r), dw.p, M, H, stream())
        ck.equal(f"M{M}-H{H}-zero-dy", "dw", torch.equal(dw.get(), I.dw0))
    ck.done()


# ----------------------------------------------------------------------------- LayerNorm(z * keep + res) and its backward
@pytest.mark.parametrize("H", R.HS_LNRES)
def test_layernorm_res_fwd_bwd(H):
    cf, cb = Checks("ta_layernorm_res_fwd"), Checks("ta_layernorm_bwd")
    for M in R.CASES["layernorm_res"]["M"]:
        for kr, rr in ((False, 0), (True, 0), (True, M)) + (((True, 7),) if M == 70 else ()):
            for eps in R.CASES["layernorm_res"]["eps"]:
                c = R.lnres_case(H, M, kr, rr if rr != M else 0, eps)
                case = f"H{H}-M{M}-{'keepres' if kr else 'plain'}-rr{rr}-eps{eps:g}"
                gamma, beta = dev(c.gamma), dev(c.beta)
                xhat, rstd, yf, yb = Guarded(M, H), Guarded(M), Guarded(M, H), Guarded(M, H, BF16)
                call("ta_layernorm_res_fwd", ptr(dev(c.z)), ptr(dev(c.keep)), ptr(dev(c.res)), rr, ptr(gamma), ptr(beta), eps, xhat.p, rstd.p,
                     yf.p, yb.p, M, H, stream())
                cf.rows(case, "xhat", xhat.get(), c.fx["xhat"], c.fm["xhat"], H)
                cf.rows(case, "rstd", rstd.get(), c.fx["rstd"], c.fm["rstd"], M)
                cf.rows(case, "y_f32", yf.get(), c.fx["y"], c.fm["y"], H)
                cf.rows(case, "y_bf16", yb.get(), c.fx["y"], c.fm["y"], H, bf16=True)
                for want in ("du+dz", "du", "dz"):
                    du = Guarded(M, H) if "du" in want else None
                    dz = Guarded(M, H, BF16) if "dz" in want else None
                    dg, db = Guarded(H, None, F32, c.dg0), Guarded(H, None, F32, c.db0)
                    call("ta_layernorm_bwd", ptr(dev(c.dy)), ptr(dev(c.xhat)), ptr(dev(c.rstd)), ptr(gamma), ptr(dev(c.keep)), p_(du), p_(dz),
                         dg.p, db.p, M, H, stream())
                    if du is not None:
                        cb.rows(f"{case}-{want}", "du", du.get(), c.bx["du"], c.bm["du"], H)
                    if dz is not None:
                        cb.rows(f"{case}-{want}", "dz", dz.get(), c.bx["dz"], c.bm["dz"], H, bf16=True)
                    cb.rows(f"{case}-{want}", "dgamma", dg.get(), c.bx["dgamma"], c.bm["dgamma"], H, unordered=M)
                    cb.rows(f"{case}-{want}", "dbeta", db.get(), c.bx["dbeta"], c.bm["dbeta"], H, unordered=M)
    cf.done(); cb.done()


def test_layernorm_res_argument_errors():
    M, H = 3, 2052
    z, g = torch.zeros(M, H, device=DEV), torch.ones(H, device=DEV)
    xhat, rstd, du = Guarded(M, H), Guarded(M), Guarded(M, H)
    call("ta_layernorm_res_fwd", ptr(z), None, None, 0, ptr(g), ptr(g), 1e-5, xhat.p, rstd.p, None, None, M, H, stream(), expect=ERR_ARG)
    call("ta_layernorm_bwd", ptr(z), ptr(z), ptr(g), ptr(g), None, du.p, None, None, None, M, H, stream(), expect=ERR_ARG)
    for t in (xhat, rstd, du):
        assert bool((t.get().view(torch.int32) == -1).all())


# ----------------------------------------------------------------------------- labels
def test_label_rows():
    for B, L in R.CASES["label_rows"]["BL"]:
        for kind in R.CASES["label_rows"]["kinds"]:
            lab = R.make_labels(B, L, kind)
            rows_e, tg_e, n_e = R.label_rows(lab)
            labels = torch.tensor(lab, dtype=torch.int64, device=DEV)
            rows, tg, n = Guarded(B * L, None, torch.int32), Guarded(B * L, None, torch.int64), Guarded(1, None, torch.int32)
            call("ta_label_rows", ptr(labels), B, L, rows.p, tg.p, n.p, stream())
            got_n, got_r, got_t = int(n.get()[0]), rows.get().tolist(), tg.get().tolist()
            print(f"ROWGRID ta_label_rows B{B}-L{L}-{kind} n={got_n} expected={n_e}")
            assert got_n == n_e, (B, L, kind, got_n, n_e)
            assert got_r[:n_e] == rows_e and got_t[:n_e] == tg_e, (B, L, kind)
            assert all(v == -1 for v in got_r[n_e:]) and all(v == -1 for v in got_t[n_e:]), (B, L, kind, "entries beyond n were written")


# ----------------------------------------------------------------------------- cross-entropy
def run_ce(ck, case, z, rows, t, V, ldl, ldd, scale, with_nll, with_dl=True, acc0=0.0, calls=1):
    n = len(t)
    e, m = R.cross_entropy(z, rows, t, V, scale, ldd), R.cross_entropy(z, rows, t, V, scale, ldd, model=True)
    zd, td = dev(z), torch.tensor(t, dtype=torch.int64, device=DEV)
    rd = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    nll = Guarded(n) if with_nll else None
    dl = Guarded(n, ldd, BF16) if with_dl else None
    loss = Guarded(1, None, F32, torch.tensor([acc0]))
    for _ in range(calls):
        call("ta_cross_entropy", ptr(zd), int(z.dtype == BF16), ldl, ptr(rd), ptr(td), n, V, scale, p_(nll), loss.p, p_(dl), ldd, stream())
    if nll is not None:
        got = nll.get()
        ck.rows(case, "nll", got, e["nll"], m["nll"], n)
        ck.equal(case, "nll of invalid targets", not got[~e["valid"]].any())
    ex_l, mo_l = acc0 + calls * float(e["loss"]), float(torch.tensor(acc0, dtype=F32))
    for _ in range(calls):
        mo_l = float(torch.tensor(mo_l, dtype=F32) + m["loss"].float())
    ck.scalar(case, "loss", float(loss.get()[0]), ex_l, mo_l, unordered=0 if with_nll else calls * int(e["valid"].sum()))
    if dl is not None:
        got = dl.get()
        ck.rows(case, "dlogits", got, e["dlogits"], m["dlogits"], ldd, bf16=True)
        ck.equal(case, "dlogits of invalid targets", not got[~e["valid"]].float().any())
        ck.equal(case, "dlogits columns >= V", not got[:, V:].float().any())


def ce_rows(n, R_):
    rows = [(7 * i + 3) % R_ for i in range(n)]
    rows[5] = rows[2]                                                       # non-monotonic, one row twice
    return rows


@pytest.mark.parametrize("V,ldl", R.CASES["cross_entropy"]["V_ldl"])
def test_cross_entropy_shapes(V, ldl):
    n, scale, ck = R.CASES["cross_entropy"]["n"], 0.37, Checks("ta_cross_entropy")
    t = R.ce_targets(n, V, ldl)
    for bf in (False, True):
        for rows in (None, ce_rows(n, 50)):
            z = R.ce_logits(n if rows is None else 50, V, ldl, "normal3", bf)
            for ldd in (ldl, (V + 3) // 4 * 4, ldl + 8):
                for with_nll in (True, False):
                    case = f"V{V}-ldl{ldl}-{'bf16' if bf else 'f32'}-{'rows' if rows else 'norows'}-ldd{ldd}-{'nll' if with_nll else 'atomic'}"
                    run_ce(ck, case, z, rows, t, V, ldl, ldd, scale, with_nll)
            run_ce(ck, f"V{V}-ldl{ldl}-{'bf16' if bf else 'f32'}-nodlogits", z, rows, t, V, ldl, ldl, scale, True, with_dl=False)
    ck.done()


def test_cross_entropy_values():
    V, ldl, n, scale, ck = 1003, 1024, 37, 0.37, Checks("ta_cross_entropy")
    for kind in R.CASES["cross_entropy"]["values"]:
        bf = kind == "bf16x5"
        z = R.ce_logits(n, V, ldl, kind, bf)
        t = R.ce_targets(n, V, ldl)
        if kind == "dominant_target":
            t = [i % V for i in range(n)]
        elif kind == "dominant_other":
            t = [(i + 1) % V for i in range(n)]
        run_ce(ck, f"{kind}-nll", z, None, t, V, ldl, ldl, scale, True)
        run_ce(ck, f"{kind}-atomic", z, None, t, V, ldl, ldl, scale, False)
    z, t = R.ce_logits(n, V, ldl, "normal3", False), R.ce_targets(n, V, ldl)
    run_ce(ck, "atomic-twice", z, None, t, V, ldl, ldl, scale, False, calls=2)       # loss_accum is added to, not overwritten
    run_ce(ck, "nll-onto-1.5", z, None, t, V, ldl, ldl, scale, True, acc0=1.5)
    ck.done()


def test_cross_entropy_argument_errors():
    """V > ldl, and ldd < V with dlogits: TA_ERR_ARG, nothing written.  (The buffers are large enough for a library without the check.)"""
    n, ldl = 4, 8
    z = torch.zeros(n + 4, ldl, device=DEV)
    t = torch.zeros(n, dtype=torch.int64, device=DEV)
    nll, loss, dl = Guarded(n), Guarded(1, None, F32, torch.zeros(1)), Guarded(n + 4, 16, BF16)
    call("ta_cross_entropy", ptr(z), 0, ldl, None, ptr(t), n, 12, 1.0, nll.p, loss.p, dl.p, 16, stream(), expect=ERR_ARG)       # V > ldl
    call("ta_cross_entropy", ptr(z), 0, ldl, None, ptr(t), n, 8, 1.0, nll.p, loss.p, dl.p, 4, stream(), expect=ERR_ARG)         # ldd < V
    assert float(loss.get()[0]) == 0.0 and bool((nll.get().view(torch.int32) == -1).all())
    call("ta_cross_entropy", ptr(z), 0, ldl, None, ptr(t), n, 8, 1.0, nll.p, loss.p, None, 4, stream())                         # no dlogits: ldd unused
    assert bool((dl.get().view(torch.int16) == -1).all())
    assert abs(float(loss.get()[0]) - n * 2.0794415) < 1e-4 and bool((nll.get() > 2.0).all())     # (the accepted call ran: log 8 per row)


# ----------------------------------------------------------------------------- optimizer
def grads_of(n, clip, seed):
    """p ~ N(0, 1) and a gradient of norm 0.5 (clip inactive: 0.5 * grad_scale / denom < 1) or 8 (> 1 even after denom = 4)."""
    g = R._gen(n, seed, 11)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr = gr / gr.double().norm().float() * (0.5 if clip == "inactive" else 8.0)
    return p, gr


def clip_args(gr, clip):
    if clip == "none":
        return None, 1.0
    sq = R.sqnorm(gr, model=True).float().reshape(1)                         # the f32 scalar the step is handed
    return sq, (0.0 if clip == "max_norm0" else 1.0)


def gate_state(ck, case, got, exact, model):
    pad = lambda t: torch.cat([t.detach().cpu().to(F64).reshape(-1), torch.zeros(-t.numel() % 1024, dtype=F64)])
    for name, g, e, m in zip("pmv", got, exact, model):
        ck.rows(case, name, pad(g), pad(e), pad(m), 1024)


@pytest.mark.parametrize("clip", R.CASES["adamw"]["clip"])
@pytest.mark.parametrize("n", R.CASES["adamw"]["n"])
def test_adamw_step(n, clip):
    ck = Checks("ta_adamw_step")
    p0, gr = grads_of(n, clip, 0)
    sq, max_norm = clip_args(gr, clip)
    for denom in R.CASES["adamw"]["denom"]:
        for wd in R.CASES["adamw"]["wd"]:
            z = torch.zeros(n)
            P, Mm, Vv = Guarded(n, None, F32, p0), Guarded(n, None, F32, z), Guarded(n, None, F32, z)
            gd, sqd = dev(gr), dev(sq)
            dd = None if denom is None else torch.tensor([denom], device=DEV)
            ex, mo = (p0, z, z), (p0, z, z)
            for step in range(1, R.CASES["adamw"]["steps"] + 1):
                call("ta_adamw_step", P.p, ptr(gd), Mm.p, Vv.p, n, R.ADAM["lr"], R.ADAM["beta1"], R.ADAM["beta2"], R.ADAM["eps"], wd, step,
                     ptr(sqd), max_norm, 1.0, ptr(dd), stream())
                kw = dict(wd=wd, step=step, sq=sq, max_norm=max_norm, grad_scale=1.0, denom=denom, **R.ADAM)
                ex, mo = R.adamw(ex[0], gr, ex[1], ex[2], **kw), R.adamw(mo[0].float(), gr, mo[1].float(), mo[2].float(), model=True, **kw)
            gate_state(ck, f"n{n}-{clip}-denom{denom}-wd{wd}", (P.get(), Mm.get(), Vv.get()), ex, mo)
    if clip == "active":                                                      # the settings do what their names say
        assert float(R.clip_coef(sq, 1.0, 1.0, 4.0)) < 0.25 and float(R.clip_coef(sq, 1.0, 1.0, 0.25)) < 1.0
    if clip == "inactive":
        assert float(R.clip_coef(sq, 1.0, 1.0, None)) == 1.0
    ck.done()


@pytest.mark.parametrize("clip", R.CASES["adamw"]["clip"])
@pytest.mark.parametrize("denom", R.CASES["adamw"]["denom"])
def test_adamw_step_multi(clip, denom):
    """4096 blocks x 256 threads x 4 elements = 4096 * 1024 elements per pass: the last 1028 are the grid's second pass.  Segments end
    at 4, at 5004 (no multiple of 1024), at the element where the grid wraps, and at n; they alternate weight decay 0 / 0.1."""
    n, ck = R.CASES["adamw"]["multi_n"], Checks("ta_adamw_step_multi")
    ends, seg_lr, seg_wd, lr_mult = [4, 5004, 4096 * 1024, n], [1e-2, 2e-2, 5e-3, 1e-2], [0.0, 0.1, 0.0, 0.1], 0.5
    p0, gr = grads_of(n, clip, 1)
    sq, max_norm = clip_args(gr, clip)
    lens = torch.tensor([ends[0]] + [b - a for a, b in zip(ends, ends[1:])])
    lr = torch.repeat_interleave(torch.tensor(seg_lr, dtype=F32).double() * R.f32v(lr_mult), lens)
    wd = torch.repeat_interleave(torch.tensor(seg_wd, dtype=F32), lens)
    z = torch.zeros(n)
    P, Mm, Vv = Guarded(n, None, F32, p0), Guarded(n, None, F32, z), Guarded(n, None, F32, z)
    gd, sqd = dev(gr), dev(sq)
    dd = None if denom is None else torch.tensor([denom], device=DEV)
    se, sl, sw = torch.tensor(ends, dtype=torch.int64, device=DEV), torch.tensor(seg_lr, device=DEV), torch.tensor(seg_wd, device=DEV)
    ex, mo = (p0, z, z), (p0, z, z)
    hp = {k: v for k, v in R.ADAM.items() if k != "lr"}
    for step in range(1, R.CASES["adamw"]["steps"] + 1):
        call("ta_adamw_step_multi", P.p, ptr(gd), Mm.p, Vv.p, n, ptr(se), ptr(sl), ptr(sw), len(ends), lr_mult, hp["beta1"], hp["beta2"],
             hp["eps"], step, ptr(sqd), max_norm, 1.0, ptr(dd), stream())
        kw = dict(lr=lr, wd=wd, step=step, sq=sq, max_norm=max_norm, grad_scale=1.0, denom=denom, **hp)
        ex, mo = R.adamw(ex[0], gr, ex[1], ex[2], **kw), R.adamw(mo[0].float(), gr, mo[1].float(), mo[2].float(), model=True, **kw)
    gate_state(ck, f"n{n}-{clip}-denom{denom}", (P.get(), Mm.get(), Vv.get()), ex, mo)
    ck.done()


def test_grad_sqnorm():
    ck = Checks("ta_grad_sqnorm")
    for n in R.CASES["adamw"]["n"]:
        gr = 1.7 * torch.randn(n, generator=R._gen(n, 12))
        for acc0 in (0.0, 2.5):
            acc, scratch = Guarded(1, None, F32, torch.tensor([acc0])), Guarded(1024)
            call("ta_grad_sqnorm", ptr(dev(gr)), n, acc.p, scratch.p, stream())
            scratch.get()
            ck.scalar(f"n{n}-acc{acc0}", "sqnorm", float(acc.get()[0]), float(R.sqnorm(gr, acc0)), float(R.sqnorm(gr, acc0, model=True)))
    ck.done()

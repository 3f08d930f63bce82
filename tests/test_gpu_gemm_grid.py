"""-m gpu: every tile variant of csrc/gemm.hip (``ta_gemm_bf16_nt_opt``) and csrc/gemm_tn.hip (``ta_gemm_bf16_tn``) against the float64
reference of tests/gemm_ref.py, row by row, at the smallest shapes that reach each code path (gemm_ref.CASES) and over the planted
rows of gemm_ref.nt_inputs.

Gates (gemm_ref.gates, no element and no row excluded): rows  max_r e_r <= 2 max_r m_r  with ``last_place`` applied to the model; a
bf16 output also element by element (``elem_gate``: nearest-even against truncation); the ``walk`` shapes, whose one-k-at-a-time
model would cost the host seconds per form, the a-priori bound of gemm_ref.apriori_bound element by element; values the operation
defines exactly with ==: a zero row of A under a form with no bias and no residual, an empty contraction (``gemm_tn`` with M = 0),
the untouched pad rows of a mapped output.

Every launch goes through the C ABI after ``ops.sync_gemm_knobs()``, onto an output prepared for it: 0xFF bytes (NaN as bf16 and f32)
or, for an aliased residual, the residual; 8 guard rows of 7.0 behind it and guard columns of 7.0 through ldc > N (ldc = N + 8 keeps
the wide bf16 store, ldc = N + 4 forces the narrow one; split-K requires ldc = N), all of which must still hold 7.0.  Every launch
runs under ``ta_profile_gemm(2)`` and, when a variant is forced, asserts fields 20 (tile variant as launched) and 23 (persistent)
of its log row against ``launched`` below.

Bit equality: for every case and form the output bits of each variant (the automatic choice included) equal those of variant 0 --
gemm_common.h: "a GEMM's result must not depend on the tile the launch-time model picks".

Every check prints  ``GEMMGRID <form> <case> <variant> e/m=<ratio> worst=<row>``; a test reports all of its failed checks at its
end.  The measured table is profiles/gemm_grid.md.
"""
import contextlib
import ctypes as C
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib, ops

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OK = 0
VARIANTS = G.VARIANTS
VID = [("auto" if v is None else f"v{v}") for v in VARIANTS]


def lib():
    return _lib.lib()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launched(forced, kext=False, blocked=False, far=False):
    """(field 20, field 23) of the log row of a launch under TA355_GEMM_VARIANT = forced (gemm.hip kVariants): 10 has no form for
    blocked W or far row-mapped A and goes to 5; 12 exists in the persistent form only, so the K extension and far A send it to 3;
    field 23 says which form 3 / 4 take (persistent unless the launch has a K extension or far A) and is 0 for every other row."""
    v = forced
    if forced == 10 and (blocked or far):
        v = 5
    if forced == 12 and (kext or far):
        v = 3
    return v, int(v in (3, 4) and not (kext or far))


@contextlib.contextmanager
def variant(v):
    old = os.environ.get("TA355_GEMM_VARIANT")
    if v is None:
        os.environ.pop("TA355_GEMM_VARIANT", None)
    else:
        os.environ["TA355_GEMM_VARIANT"] = str(v)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        if old is None:
            os.environ.pop("TA355_GEMM_VARIANT", None)
        else:
            os.environ["TA355_GEMM_VARIANT"] = old
        ops.sync_gemm_knobs()


_DEV = {}


def dev(t):
    """The device copy of a host input (kept for the session: the same seeded inputs serve every variant)."""
    if t is None:
        return None
    k = id(t)
    if k not in _DEV:
        _DEV[k] = (t, t.to(DEV).contiguous())
    return _DEV[k][1]


_PACKED = {}


def packed(W):
    if id(W) not in _PACKED:
        _PACKED[id(W)] = (W, G.pack_w_blocked(W))
    return _PACKED[id(W)][1]


class Out:
    """[M, N] inside a [M + 8, ldc] buffer of 7.0: 0xFF bytes, or ``start`` (an aliased residual)."""

    def __init__(self, M, N, ldc, dtype, start=None):
        self.M, self.N = M, N
        self.full = torch.full((M + 8, ldc), 7.0, device=DEV, dtype=dtype)
        if start is not None:
            self.full[:M, :N] = start.to(DEV).to(dtype)
        else:
            self.full.view(torch.int16 if dtype == BF16 else torch.int32)[:M, :N] = -1

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.full[self.M:] == 7).all()) and bool((self.full[:self.M, self.N:] == 7).all()), "guard rows / columns overwritten"
        return self.full[:self.M, :self.N]


def strided(t, ldc):
    """A residual that is not the output, in the output's row layout (columns >= N hold 7.0)."""
    M, N = t.shape
    buf = torch.full((M, ldc), 7.0, device=DEV, dtype=t.dtype)
    buf[:, :N] = t.to(DEV)
    return buf


def nt_launch(A, W, C_, M, N, K, *, ldc, a_map=None, c_map=None, bias=None, res=None, act=0, out_bf16=False, splits=1, ws=None,
              A2=None, W2=None, rope=None, blocked=False, expect=None):
    """One ta_gemm_bf16_nt_opt launch under the launch log.  -> the log rows (lists of 24 integers)."""
    L = lib()
    opts = _lib.GemmOpts()
    opts.w_blocked = int(blocked)
    if res is not None and res.dtype == BF16:
        opts.residual_bf16 = ptr(res)
    if A2 is not None:
        opts.a2, opts.w2, opts.k2, opts.lda2 = ptr(A2), ptr(W2), W2.shape[1], A2.shape[1]
    if rope is not None:
        opts.rope_tab, opts.rope_rows, opts.rope_cols = ptr(rope[0]), int(rope[1]), int(rope[2])
    lda, a_rpb, a_bs = a_map or (K, 0, 0)
    c_rpb, c_bs, c_off = c_map or (0, 0, 0)
    ops.sync_gemm_knobs()
    L.ta_profile_gemm(2)
    try:
        st = L.ta_gemm_bf16_nt_opt(ptr(A), ptr(W), ptr(C_), M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off, ptr(bias),
                                   ptr(res) if (res is not None and res.dtype == F32) else None, act, int(out_bf16), splits, ptr(ws),
                                   None, None, None, C.addressof(opts), stream())
        n = L.ta_profile_gemm_log(None, 0)
        buf = (C.c_long * (max(n, 1) * 24))()
        L.ta_profile_gemm_log(C.cast(buf, C.c_void_p), n)
    finally:
        L.ta_profile_gemm(0)
    assert st == OK, ("ta_gemm_bf16_nt_opt", st)
    rows = [list(buf[i * 24:(i + 1) * 24]) for i in range(n)]
    assert len(rows) == 1, rows
    if expect is not None:
        assert (rows[0][20], rows[0][23]) == expect, ("launched variant / persistent", rows[0][20], rows[0][23], "expected", expect)
    return rows[0]


class Checks:
    def __init__(self):
        self.bad = []

    def gates(self, form, case, v, got, exact, pre, width, out_bf16, row):
        vn = "auto" if v is None else v
        for name, ok, ratio, w in G.gates(got, exact, pre, width, out_bf16):
            print(f"GEMMGRID {form}{'' if name == 'rows' else '.' + name} {case} {vn} e/m={ratio:.3f} worst={w} launched={row[20]} persistent={row[23]}")
            if not ok:
                self.bad.append((form, case, vn, name, ratio, w))

    def equal(self, form, case, v, what, cond):
        if not cond:
            self.bad.append((form, case, "auto" if v is None else v, what))

    def done(self):
        assert not self.bad, self.bad


_BITS = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_device_tensors_end_with_the_module():
    """The inputs, walk references and variant-0 outputs shared across the variants (about 3 GB) are released behind the last test."""
    yield
    for d in (_DEV, _PACKED, _BITS, _WALK):
        d.clear()
    torch.cuda.empty_cache()


def bits_check(ck, form, case, v, key, got, rerun0):
    """The output's bits against variant 0's (computed once per key by ``rerun0``)."""
    if v == 0:
        _BITS.setdefault(key, got.clone())
        return
    if key not in _BITS:
        with variant(0):
            _BITS[key] = rerun0().clone()
    same = torch.equal(got.view(torch.int16 if got.dtype == BF16 else torch.int32), _BITS[key].view(torch.int16 if got.dtype == BF16 else torch.int32))
    print(f"GEMMGRID {form}.bits {case} {'auto' if v is None else v} equal={int(same)}")
    ck.equal(form, case, v, "bits differ from variant 0", same)


# ----------------------------------------------------------------------------- edge / rope / blocked / full
def run_form(c, v, ldc):
    """One launch of case ``c`` (gemm_ref.nt_case) -> (output [M, N] on the device, log row)."""
    f, i = c.f, c.i
    M, N, K = i.M, i.N, i.K
    dt = BF16 if f.out_bf16 else F32
    res = None
    if f.res is not None:
        if f.inplace:
            out = Out(M, N, ldc, dt, start=c.res)
            res = out.full
        else:
            out = Out(M, N, ldc, dt)
            res = strided(c.res, ldc)
    else:
        out = Out(M, N, ldc, dt)
    ws = wsn = None
    if f.splits > 1:
        wsn = lib().ta_gemm_splitk_ws_bytes(M, N, f.splits) // 4
        ws = torch.full((wsn + 64,), 7.0, device=DEV, dtype=F32)
    W = dev(packed(i.W)) if f.blocked else dev(i.W)
    rope = (dev(c.rope[0]), c.rope[1], c.rope[2]) if c.rope else None
    expect = None if v is None else launched(v, kext=f.K2 > 0, blocked=f.blocked)
    row = nt_launch(dev(i.A), W, out.full, M, N, K, ldc=ldc, bias=dev(i.bias) if f.bias else None, res=res, act=f.act,
                    out_bf16=f.out_bf16, splits=f.splits, ws=ws, A2=dev(i.A2) if f.K2 else None, W2=dev(i.W2) if f.K2 else None,
                    rope=rope, blocked=f.blocked, expect=expect)
    got = out.get()
    if ws is not None:
        assert bool((ws[wsn:] == 7).all()), "split-K workspace overrun"
    return got, row


def run_case_group(key, v, rope_rows=0):
    ck = Checks()
    with variant(v):
        for (M, N, K) in G.CASES[key]["shapes"]:
            for f in G.CASES[key]["forms"]:
                c = G.nt_case(M, N, K, f.name, key, rope_rows)
                ldcs = [N] if f.splits > 1 else [N + 8] + ([N + 4] if (f.out_bf16 and N % 8 == 0 and key == "edge") else [])
                for ldc in ldcs:
                    case = f"{key}-{M}x{N}x{K}-ldc{ldc}"
                    got, row = run_form(c, v, ldc)
                    ck.gates(f.name, case, v, got.cpu(), c.exact, c.pre, N, f.out_bf16, row)
                    if not f.bias and f.res is None:
                        ck.equal(f.name, case, v, "zero row of A", bool((got[0] == 0).all()))
                    bits_check(ck, f.name, case, v, (key, M, N, K, f.name, ldc), got, lambda: run_form(c, 0, ldc)[0])
    ck.done()


@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_edge(v):
    run_case_group("edge", v)


@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_rope_and_blocked(v):
    run_case_group("rope", v, G.CASES["rope"]["rope_rows"])


@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_full(v):
    run_case_group("full", v)


# ----------------------------------------------------------------------------- walk: more tiles than CUs
_WALK = {}


def walk_case(N, K, f):
    """Inputs, exact and |A| |W|^T on the device, computed once per (shape, form) on the host."""
    M = G.CASES["walk"]["M"]
    key = (N, K, f.name)
    if key not in _WALK:
        i = G.nt_inputs(M, N, K)
        if ("abs", N, K) not in _WALK:
            _WALK[("abs", N, K)] = (i.A.to(F64).abs() @ i.W.to(F64).abs().t()).to(DEV)
        res = i.resb if f.res else None
        exact = G.gemm_nt(i.A, i.W, bias=i.bias if f.bias else None, act=f.act, res=res, out_bf16=True)
        _WALK[key] = (i, res, exact.to(DEV))
    return _WALK[key] + (_WALK[("abs", N, K)],)


def run_walk(i, f, res, v):
    M, N, K = i.M, i.N, i.K
    out = Out(M, N, N + 8, BF16, start=res)
    row = nt_launch(dev(i.A), dev(i.W), out.full, M, N, K, ldc=N + 8, bias=dev(i.bias) if f.bias else None,
                    res=out.full if res is not None else None, act=f.act, out_bf16=True, expect=None if v is None else launched(v))
    return out.get(), row


@pytest.mark.parametrize("K", G.CASES["walk"]["K"])
@pytest.mark.parametrize("N", sorted(set(G.CASES["walk"]["N"].values())))
@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_walk(v, N, K):
    M = G.CASES["walk"]["M"]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count       # what the library reads (hipDeviceAttributeMultiprocessorCount)
    if v in G.CASES["walk"]["N"] and G.CASES["walk"]["N"][v] == N:
        bm, bn = G.TILES[v]
        tiles = -(-M // bm) * -(-N // bn)
        assert ncu < tiles < 2 * ncu, (tiles, ncu)                          # every persistent workgroup walks to a second tile, not a third
    ck = Checks()
    with variant(v):
        for f in G.CASES["walk"]["forms"]:
            i, res, exact, absprod = walk_case(N, K, f)
            case = f"walk-{M}x{N}x{K}"
            got, row = run_walk(i, f, res, v)
            bound = G.apriori_bound(exact, absprod, K, dev(i.bias) if f.bias else None, f.act, dev(res), G.is_start(f.act, res, True), True, got)
            err = (got.to(F64) - exact).abs()
            finite = bool(torch.isfinite(err).all())
            ratio = float((err / bound).max()) if finite else float("inf")
            w = int((err / bound).argmax()) // N if finite else int((~torch.isfinite(err)).reshape(-1).nonzero()[0]) // N
            print(f"GEMMGRID {f.name}.bound {case} {'auto' if v is None else v} e/m={ratio:.3f} worst={w} launched={row[20]} persistent={row[23]}")
            if not (finite and ratio <= 1.0):
                ck.bad.append((f.name, case, v, "bound", ratio, w))
            bits_check(ck, f.name, case, v, ("walk", N, K, f.name), got, lambda: run_walk(i, f, res, 0)[0])
    ck.done()


# ----------------------------------------------------------------------------- the Conv1d row maps
def run_conv(c, v, stride, bias):
    """The convolution at ``stride`` through A's row map, f32 out.  -> (output on the device, log row)"""
    M, a_map = G.conv_map(c, stride)
    out = Out(M, c.Cout, c.Cout + 8, F32)
    row = nt_launch(dev(c.xp), dev(c.wp), out.full, M, c.Cout, 3 * c.Cin, ldc=c.Cout + 8, a_map=a_map, bias=dev(bias),
                    expect=None if v is None else launched(v))
    return out.get(), row


def run_conv_mapped(c, v, dt):
    """Stride 1 with the output mapped one row inside a padded [B, T + 2, Cout] buffer.  -> (output rows, log row, pad rows kept)"""
    N = c.Cout
    M, a_map = G.conv_map(c, 1)
    buf = torch.full((c.B * (c.T + 2) + 8, N), 7.0, device=DEV, dtype=dt)
    rows = (G.map_out_rows(M, N, c.T, (c.T + 2) * N, N) // N).to(DEV)
    buf.view(torch.int16 if dt == BF16 else torch.int32)[rows] = -1
    row = nt_launch(dev(c.xp), dev(c.wp), buf, M, N, 3 * c.Cin, ldc=N, a_map=a_map, c_map=(c.T, (c.T + 2) * N, N), bias=dev(c.bias),
                    out_bf16=dt == BF16, expect=None if v is None else launched(v))
    torch.cuda.synchronize()
    pad = torch.ones(buf.shape[0], dtype=torch.bool, device=DEV)
    pad[rows] = False
    return buf[rows], row, bool((buf[pad] == 7).all())


@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_maps(v):
    c = G.conv_inputs()
    K, N = 3 * c.Cin, c.Cout
    ck = Checks()
    with variant(v):
        for stride in G.CASES["maps"]["strides"]:
            M, a_map = G.conv_map(c, stride)
            A = G.map_rows(c.xp, M, K, *a_map)
            for bias in (None, c.bias):
                exact, pre = G.gemm_nt(A, c.wp, bias=bias), G.gemm_nt(A, c.wp, bias=bias, model=True)
                got, row = run_conv(c, v, stride, bias)
                form, case = f"conv-s{stride}{'+bias' if bias is not None else ''}-f32", f"maps-{M}x{N}x{K}"
                ck.gates(form, case, v, got.cpu(), exact, pre, N, False, row)
                if bias is None and stride == 1:
                    ck.equal(form, case, v, "zero row of A", bool((got[c.T + 1] == 0).all()))      # clip 1, t = 1: frames 0..2 are zero
                bits_check(ck, form, case, v, ("maps", stride, bias is None), got, lambda: run_conv(c, 0, stride, bias)[0])
        M, a_map = G.conv_map(c, 1)
        A = G.map_rows(c.xp, M, K, *a_map)
        exact, pre = G.gemm_nt(A, c.wp, bias=c.bias, out_bf16=True), G.gemm_nt(A, c.wp, bias=c.bias, out_bf16=True, model=True)
        for dt in (BF16, F32):
            got, row, kept = run_conv_mapped(c, v, dt)
            form, case = f"conv-mapped-{'bf16' if dt == BF16 else 'f32'}", f"maps-{M}x{N}x{K}"
            ck.equal(form, case, v, "pad rows keep the fill", kept)
            ck.gates(form, case, v, got.cpu(), exact, pre, N, dt == BF16, row)
            bits_check(ck, form, case, v, ("maps", "mapped", dt), got, lambda: run_conv_mapped(c, 0, dt)[0])
    ck.done()


# ----------------------------------------------------------------------------- far A: row-mapped A beyond 32-bit byte offsets
@pytest.mark.parametrize("v", VARIANTS, ids=VID)
def test_far_a(v):
    """The second batch's rows start 2^32 bytes into A (V_FAR_A): 10 goes to 5, 12 to 3, 3 / 4 to their one-tile-per-workgroup form.
    Bit-equal to the same product from a compact A, and inside the gates."""
    d = G.CASES["far"]
    M, N, K, rpb, bs = d["M"], d["N"], d["K"], d["a_rpb"], d["a_bs"]
    i = G.nt_inputs(M, N, K)
    ck = Checks()
    big = torch.empty(bs + rpb * K, device=DEV, dtype=BF16)                 # 4 GiB + 32 KiB; only the 256 rows that are read are written
    try:
        big[:rpb * K] = dev(i.A)[:rpb].reshape(-1)
        big[bs:bs + rpb * K] = dev(i.A)[rpb:].reshape(-1)
        with variant(v):
            for ob in (False, True):
                dt = BF16 if ob else F32
                exact, pre = G.gemm_nt(i.A, i.W, bias=i.bias, out_bf16=ob), G.gemm_nt(i.A, i.W, bias=i.bias, out_bf16=ob, model=True)
                far, near = Out(M, N, N + 8, dt), Out(M, N, N + 8, dt)
                row = nt_launch(big, dev(i.W), far.full, M, N, K, ldc=N + 8, a_map=(K, rpb, bs), bias=dev(i.bias), out_bf16=ob,
                                expect=None if v is None else launched(v, far=True))
                assert not (row[18] & 256), "the far launch must not be logged with an identity A row map"
                nt_launch(dev(i.A), dev(i.W), near.full, M, N, K, ldc=N + 8, bias=dev(i.bias), out_bf16=ob,
                          expect=None if v is None else launched(v))
                got = far.get()
                form, case = f"bias-{'bf16' if ob else 'f32'}", f"far-{M}x{N}x{K}"
                ck.gates(form, case, v, got.cpu(), exact, pre, N, ob, row)
                ck.equal(form, case, v, "far A differs from compact A", torch.equal(got.view(torch.int16 if ob else torch.int32),
                                                                                 near.get().view(torch.int16 if ob else torch.int32)))
    finally:
        torch.cuda.synchronize()
        del big
        torch.cuda.empty_cache()
    ck.done()


# ----------------------------------------------------------------------------- gemm_tn
def tn_launch(Y, X, out, M, Ny, Nx, accumulate):
    """Exactly ws_bytes of workspace, followed by a guard."""
    L = lib()
    nb = L.ta_gemm_bf16_tn_ws_bytes(M, Ny, Nx)
    ws = torch.full((nb + 64,), 7, device=DEV, dtype=torch.uint8)
    st = L.ta_gemm_bf16_tn(ptr(Y), ptr(X), ptr(out), M, Ny, Nx, accumulate, ptr(ws) if nb else None, nb, stream())
    assert st == OK, ("ta_gemm_bf16_tn", st)
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 7).all()), "workspace overrun"


@pytest.mark.parametrize("M", G.CASES["tn"]["M"])
def test_gemm_tn(M):
    ck = Checks()
    for Ny, Nx in G.CASES["tn"]["NyNx"]:
        t = G.tn_inputs(M, Ny, Nx)
        for acc in (0, 1):
            start = t.start if acc else None
            exact, pre = G.gemm_tn(t.Y, t.X, start), G.gemm_tn(t.Y, t.X, start, model=True)
            runs = []
            for _ in range(2):
                out = Out(Ny, Nx, Nx, F32, start=start)
                tn_launch(dev(t.Y), dev(t.X), out.full, M, Ny, Nx, acc)
                runs.append(out.get().clone())
            form, case = f"tn-acc{acc}", f"tn-M{M}-{Ny}x{Nx}"
            for name, ok, ratio, w in G.gates(runs[0].cpu(), exact, pre, Nx, False):
                print(f"GEMMGRID {form} {case} tn e/m={ratio:.3f} worst={w}")
                if not ok:
                    ck.bad.append((form, case, name, ratio, w))
            ck.equal(form, case, "tn", "two runs differ", torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)))
            if not acc:
                ck.equal(form, case, "tn", "zero column of Y", bool((runs[0][0] == 0).all()))
    ck.done()


def test_gemm_tn_empty_contraction():
    """M = 0: zeros without ``accumulate``, ``out`` left alone with it."""
    Ny, Nx = 136, 264
    t = G.tn_inputs(0, Ny, Nx)
    Y, X = torch.zeros(8, Ny, device=DEV, dtype=BF16), torch.zeros(8, Nx, device=DEV, dtype=BF16)
    out = Out(Ny, Nx, Nx, F32)
    tn_launch(Y, X, out.full, 0, Ny, Nx, 0)
    assert bool((out.get() == 0).all())
    out = Out(Ny, Nx, Nx, F32, start=t.start)
    tn_launch(Y, X, out.full, 0, Ny, Nx, 1)
    assert torch.equal(out.get().cpu(), t.start)

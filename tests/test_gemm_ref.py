"""Host checks of tests/gemm_ref.py (no GPU): the reference against independent forms of the same operations, the order of a correct
MFMA kernel inside the gates on every case of the table, and mutants of that output, each of which the gates must reject."""
import numpy as np
import pytest
import torch

from oracle import encoder as OE
from tests import gemm_ref as G

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EDGE = G.CASES["edge"]["shapes"]
ROPE_SHAPE, ROPE_ROWS = G.CASES["rope"]["shapes"][0], G.CASES["rope"]["rope_rows"]


# ----------------------------------------------------------------------------- the reference against independent forms
def test_exact_is_the_einsum_with_the_epilogue_written_out():
    M, N, K = EDGE[0]
    i = G.nt_inputs(M, N, K, 128)
    A, W, A2, W2 = (t.to(F64) for t in (i.A, i.W, i.A2, i.W2))
    p = torch.einsum("mk,nk->mn", A, W)
    p2 = torch.einsum("mk,nk->mn", A2, W2)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)  # noqa: E731
    assert close(G.gemm_nt(i.A, i.W), p)
    assert close(G.gemm_nt(i.A, i.W, bias=i.bias, res=i.res), p + i.bias.to(F64) + i.res.to(F64))
    assert close(G.gemm_nt(i.A, i.W, A2=i.A2, W2=i.W2, res=i.resb, out_bf16=True), p + p2 + i.resb.to(F64))
    assert close(G.gemm_nt(i.A, i.W, splits=3, res=i.res), p + i.res.to(F64))
    g = G.gemm_nt(i.A, i.W, bias=i.bias, act=1, res=i.resb)
    assert float((g - (G.gelu_erf(p + i.bias.to(F64)) + i.resb.to(F64))).abs()[3:].max()) <= 2.5e-5
    # the model is the same function: it differs from the exact form by f32 roundings only
    m = G.gemm_nt(i.A, i.W, bias=i.bias, res=i.res, model=True)
    e = G.gemm_nt(i.A, i.W, bias=i.bias, res=i.res)
    assert 0 < float(G.row_errors(m, e, N).max()) < K * 2.0 ** -24
    t = G.tn_inputs(97, 136, 264)
    assert close(G.gemm_tn(t.Y, t.X, t.start), torch.einsum("my,mx->yx", t.Y.to(F64), t.X.to(F64)) + t.start.to(F64))
    assert G.split_ranges(192, 2) == [(0, 64), (64, 192)] and G.split_ranges(128, 5) == [(0, 64), (64, 128)]
    assert G.split_ranges(192, 3) == [(0, 64), (64, 128), (128, 192)]


@pytest.mark.parametrize("rope_cols", [0, 128])
def test_rope_form_is_the_oracles_rotate_half_rope_under_il_perm(rope_cols):
    M, N, K = ROPE_SHAPE
    i = G.nt_inputs(M, N, K)
    nh = N // 64
    y = i.A.to(F64) @ i.W.to(F64).t() + i.bias.to(F64)                                  # plain head-dim order
    cos, sin = OE.rope_tables(ROPE_ROWS, 32, 10000.0)                                   # [rows, 32] = cat(freqs, freqs)
    pos = np.arange(M) % ROPE_ROWS
    ref = OE.apply_rope(y.reshape(1, M, nh, 64).permute(0, 2, 1, 3).numpy(), cos[pos].astype(np.float64), sin[pos].astype(np.float64))
    ref = torch.from_numpy(ref).permute(0, 2, 1, 3)[..., G.il_perm()].reshape(M, N)
    lim = rope_cols if rope_cols else N
    ref[:, lim:] = y.reshape(M, nh, 64)[..., G.il_perm()].reshape(M, N)[:, lim:]
    rows = (torch.arange(nh)[:, None] * 64 + G.il_perm()[None]).reshape(-1)             # W's rows in the interleaved order
    tab = torch.from_numpy(np.stack([cos[:, :16], sin[:, :16]], -1).copy())
    got = G.gemm_nt(i.A, i.W[rows].contiguous(), bias=i.bias[rows], act=2, rope=(tab, ROPE_ROWS, rope_cols), out_bf16=True)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert float((G.rope_table(ROPE_ROWS) - tab).abs().max()) < 1e-6                    # the tests' own table is that table


@pytest.mark.parametrize("stride", [1, 2])
def test_row_maps_are_conv1d(stride):
    c = G.conv_inputs()
    M, (lda, rpb, bs) = G.conv_map(c, stride)
    A = G.map_rows(c.xp, M, 3 * c.Cin, lda, rpb, bs)
    got = G.gemm_nt(A, c.wp, bias=c.bias)
    ref = torch.nn.functional.conv1d(c.xp[:, 1:c.T + 1].to(F64).transpose(1, 2), c.wp.to(F64).reshape(c.Cout, 3, c.Cin).permute(0, 2, 1),
                                     c.bias.to(F64), stride=stride, padding=1).transpose(1, 2).reshape(M, c.Cout)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    rows = G.map_out_rows(c.B * c.T, c.Cout, c.T, (c.T + 2) * c.Cout, c.Cout)           # the mapped output skips one pad row per side
    assert rows[0] == c.Cout and rows[c.T] == (c.T + 2) * c.Cout + c.Cout and len(set(rows.tolist())) == c.B * c.T


def test_blocked_w_packer_round_trip():
    N, K = 384, 192
    W = torch.arange(N * K, dtype=F32).reshape(N, K)
    Wb = G.pack_w_blocked(W)
    assert torch.equal(G.unpack_w_blocked(Wb, N, K), W)
    blk = Wb.view(N // 64, K // 64, 64, 64)
    assert torch.equal(blk[2, 1], W[128:192, 64:128])                                   # 64 rows x one K tile, contiguous
    assert Wb.view(-1)[((2 * (K // 64) + 1) << 12) + (5 << 6) + 3] == W[128 + 5, 64 + 3]   # gemm_common.h w_tile_off


def test_chords_are_the_header_and_within_their_bound_of_erf_gelu():
    tab = G.gelu_chords()
    assert torch.equal(tab, G.gelu_lut_header())
    x = torch.cat([torch.linspace(-12, 12, 2_000_001, dtype=F64), torch.tensor([-1e4, 1e4, 0.0, -8.0, 8.0 - 2.0 ** -20], dtype=F64)]).to(F32).to(F64)
    for model in (False, True):
        err = (G.gelu_table(x, model) - G.gelu_erf(x)).abs()
        assert float(err.max()) <= 2.5e-5, float(err.max())
    # continuity at the segment ends, up to the f32 rounding of the coefficients (|b| < 4: ulp 2.4e-7, |a x| < 8: 4.8e-7, twice):
    # what lets the two forms take their index from different values
    assert G.chord_jump() < 1e-6


# ----------------------------------------------------------------------------- a correct kernel's order stays inside the gate
def emulate(c, mut=None):
    """The MFMA order through the model's epilogue: (value before the store's rounding, value as stored)."""
    pre = G.gemm_nt(c.i.A, c.i.W, model=True, summer=G.mfma_sum, mut=mut, **c.kw)
    return pre, (G.rb(pre) if c.f.out_bf16 else G.rf(pre))


def passes(got, c):
    return all(ok for _, ok, _, _ in G.gates(got, c.exact, c.pre, c.i.N, c.f.out_bf16))


def all_cases():
    out = [("edge", s, f.name, 0) for s in EDGE for f in G.CASES["edge"]["forms"]]
    out += [("rope", ROPE_SHAPE, f.name, ROPE_ROWS) for f in G.CASES["rope"]["forms"]]
    out += [("full", G.CASES["full"]["shapes"][0], f.name, 0) for f in G.CASES["full"]["forms"]]
    return out


@pytest.mark.parametrize("key", ["edge", "rope", "full"])
def test_mfma_order_passes_every_case(key):
    bad = []
    for k, (M, N, K), name, rr in all_cases():
        if k != key:
            continue
        c = G.nt_case(M, N, K, name, k, rr)
        _, got = emulate(c)
        for gname, ok, ratio, w in G.gates(got, c.exact, c.pre, N, c.f.out_bf16):
            print(f"GEMMREF {name} {M}x{N}x{K} {gname} e/m={ratio:.3f} worst={w}")
            if not ok:
                bad.append((name, (M, N, K), gname, ratio, w))
    assert not bad, bad


def test_mfma_order_passes_maps_and_tn():
    c = G.conv_inputs()
    for stride in (1, 2):
        M, (lda, rpb, bs) = G.conv_map(c, stride)
        A = G.map_rows(c.xp, M, 3 * c.Cin, lda, rpb, bs)
        exact, pre = G.gemm_nt(A, c.wp, bias=c.bias), G.gemm_nt(A, c.wp, bias=c.bias, model=True)
        got = G.gemm_nt(A, c.wp, bias=c.bias, model=True, summer=G.mfma_sum)
        assert all(ok for _, ok, _, _ in G.gates(got, exact, pre, c.Cout, False))
        assert all(ok for _, ok, _, _ in G.gates(G.rb(got), exact, pre, c.Cout, True))
    for M in G.CASES["tn"]["M"]:
        for Ny, Nx in G.CASES["tn"]["NyNx"]:
            t = G.tn_inputs(M, Ny, Nx)
            pad = (-M) % 32                                                            # the kernel zero-fills the last 32-row step
            Yp, Xp = (torch.cat([a, torch.zeros(pad, a.shape[1], dtype=BF16)]) for a in (t.Y, t.X))
            for start in (None, t.start):
                acc = start.clone() if start is not None else torch.zeros(Ny, Nx)
                got = G.mfma_sum(acc, Yp.t(), Xp.t()).to(F64)
                res = G.gates(got, G.gemm_tn(t.Y, t.X, start), G.gemm_tn(t.Y, t.X, start, model=True), Nx, False)
                assert all(ok for _, ok, _, _ in res), (M, Ny, Nx, start is not None, res)


@pytest.mark.parametrize("K", G.CASES["walk"]["K"])
def test_mfma_order_passes_the_a_priori_bound_of_the_walk_shapes(K):
    """The walk shapes' gate at their K (the bound does not depend on M and N: 300 rows keep the host test short)."""
    for f in G.CASES["walk"]["forms"]:
        i = G.nt_inputs(300, 384, K)
        res = i.resb if f.res else None
        kw = dict(bias=i.bias if f.bias else None, act=f.act, res=res, out_bf16=True)
        exact = G.gemm_nt(i.A, i.W, **kw)
        pre = G.gemm_nt(i.A, i.W, model=True, summer=G.mfma_sum, **kw)
        absprod = i.A.to(F64).abs() @ i.W.to(F64).abs().t()
        bound = lambda got: G.apriori_bound(exact, absprod, K, kw["bias"], f.act, res, G.is_start(f.act, res, True), True, got)  # noqa: E731
        got = G.rb(pre)
        assert bool(((got - exact).abs() <= bound(got)).all()), f.name
        bad = G.trunc_bf16(pre)
        assert not bool(((bad - exact).abs() <= bound(bad)).all()), f.name
        lost = got.clone()
        lost[7, 9] = G.rb(G.gemm_nt(i.A[:, :K - 32], i.W[:, :K - 32], model=True, summer=G.mfma_sum, **kw))[7, 9]
        assert not bool(((lost - exact).abs() <= bound(lost)).all()), f.name


# ----------------------------------------------------------------------------- mutants must be rejected
def case(name, shape=0, key="edge"):
    M, N, K = (EDGE[shape] if key == "edge" else G.CASES[key]["shapes"][0])
    return G.nt_case(M, N, K, name, key, ROPE_ROWS if key == "rope" else 0)


def mutants():
    out = []

    def add(label, form, fn, shape=0, key="edge"):
        out.append(pytest.param(form, shape, key, fn, id=f"{label}-{form}-{shape}"))

    def lose32(r, col):
        def fn(c, pre, got):
            K = c.i.K
            short = G.gemm_nt(c.i.A[:, :K - 32], c.i.W[:, :K - 32], model=True, summer=G.mfma_sum, **c.kw)
            got[r, col] = (G.rb(short) if c.f.out_bf16 else short)[r, col]
            return got
        return fn
    for form in ("plain-f32", "plain-bf16", "bias-f32", "bias-bf16"):
        if form != "bias-bf16":                                            # (a bf16 bias of O(1) swallows the whole 1e-3 row)
            add("lose32-row1", form, lose32(1, 7))
        add("lose32-row100", form, lose32(100, 200), shape=1)

    def other_seed(c, pre, got):
        o = G.nt_inputs(c.i.M, c.i.N, c.i.K, c.f.K2, seed=1)
        alt = G.gemm_nt(o.A, o.W, model=True, summer=G.mfma_sum, **c.kw)
        got[0:16, 32:48] = (G.rb(alt) if c.f.out_bf16 else alt)[0:16, 32:48]
        return got
    for form in ("plain-bf16", "bias-f32"):
        add("fragment-other-seed", form, other_seed)
    for form in ("bias-f32", "bias-bf16", "bias+gelu-bf16"):
        add("bias-shift4", form, lambda c, pre, got: emulate(c, dict(bias_shift=4))[1])
    for f in G.CASES["edge"]["forms"]:
        if f.out_bf16:
            add("truncation", f.name, lambda c, pre, got: G.trunc_bf16(pre))
    add("rope-row-m", "rope-all", lambda c, pre, got: emulate(c, dict(rope_row=True))[1], key="rope")
    add("rope-past-cols", "rope-128", lambda c, pre, got: emulate(c, dict(rope_col=True))[1], key="rope")
    for form in ("bias+resf32-f32", "resf32-bf16", "resbf16-f32", "gelu+resbf16-bf16"):
        add("residual-twice", form, lambda c, pre, got: emulate(c, dict(res_twice=32))[1])

    def start_twice(c, pre, got):                                          # the start-value form: the strip starts from 2 r
        i = c.i
        alt = G.gemm_nt(i.A, i.W, res=(2 * i.resb.to(F32)).to(BF16), out_bf16=True, model=True, summer=G.mfma_sum)
        got[32:48] = G.rb(alt)[32:48]
        return got
    add("residual-twice", "resbf16-inplace-bf16", start_twice)
    for form in ("splitk2-f32", "splitk3-bf16", "splitk3+resf32-f32", "splitk5+resf32-bf16"):
        add("slab-dropped", form, lambda c, pre, got: emulate(c, dict(drop_slab=1))[1])

    def transposed(c, pre, got):
        got[16:32, 16:32] = got[16:32, 16:32].t().clone()
        return got

    def last4_group(c, pre, got):
        got[:, -4:] = got[:, -8:-4].clone()
        return got

    def last4_column(c, pre, got):
        got[:, -3:] = got[:, -4:-3].clone()
        return got
    for form in ("plain-f32", "bias-bf16"):
        add("fragment-transposed", form, transposed)
    for form in ("plain-bf16", "bias-f32", "bias+gelu-bf16"):
        for shape in (0, 1):
            add("last4-from-the-group-before", form, last4_group, shape=shape)
            add("last4-from-column-N-4", form, last4_column, shape=shape)
    return out


@pytest.mark.parametrize("form,shape,key,fn", mutants())
def test_gates_reject_the_mutant(form, shape, key, fn):
    c = case(form, shape, key)
    pre, got = emulate(c)
    assert passes(got, c), "the unmutated emulation must pass"
    bad = fn(c, pre.clone(), got.clone())
    assert not torch.equal(bad, got), "the mutation changed nothing"
    assert not passes(bad, c)
